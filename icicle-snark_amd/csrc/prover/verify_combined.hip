// verify_combined.hip — a batch of Groth16 proofs of one key decided by ONE randomised pairing equation, and the pairing
// product primitive it is built from (the arithmetic is pairing29.h's, on the lazy radix-2^29 field).
//
//   icicle_snark_pairing_product     out = Πᵢ e(p[i], q[i]): Miller loops, a product reduction, one final exponentiation
//   groth16_verify_batch_combined    Πᵢ e(−zᵢ·Aᵢ, Bᵢ) · e(Σ zᵢ·cpubᵢ, γ₂) · e(Σ zᵢ·Cᵢ, δ₂) · e((Σ zᵢ)·α₁, β₂) = 1 for 128-bit zᵢ
//                                    derived from a secret seed.  Per live proof one lane: the endomorphism subgroup test of B,
//                                    [zᵢ](−Aᵢ), one single-pair Miller loop.  The lanes' values are multiplied together on the
//                                    device, Σ zᵢ·Cᵢ is the library's G1 MSM over 128-bit scalars, the signal sums Σ zᵢ·sᵢⱼ run on
//                                    the worker pool, and the three fixed-G2 pairs and the final exponentiation are paid once, on
//                                    the host.  Any subgroup failure or a failed equation sends the live items through the
//                                    per-item stage of groth16_verify_batch (verify_batch.hip), so the verdicts are its verdicts.
#include <chrono>
#include <errno.h>
#include <stdio.h>
#include <string.h>
#include <sys/random.h>
#include <vector>

#include "../../../include/groth16_prover.h"
#include "../common.h"
#include "../pairing29.h"
#include "../workers.h"
#include "sha256.h"
#include "verify_batch.h"

using namespace bn254;

namespace {

constexpr uint32_t CHUNK = 1u << 16; // live proofs per launch, as groth16_verify_batch
constexpr int WG = 64;
constexpr uint32_t PRODUCT_LANES = 1u << 14; // lanes (and Fq12 scratch slots) of icicle_snark_pairing_product, whatever n is

// lane i < m: f[i] = the Miller value of ([zᵢ](−Aᵢ), Bᵢ) (1 for an identity A or B), ok[i] = 0 when Bᵢ is outside the subgroup
__global__ __launch_bounds__(WG) void combined_lane_kernel(const isnark::vb::VbItem* __restrict__ items, const uint32_t* __restrict__ z, uint32_t m,
                                                           p29::F12* __restrict__ f, uint8_t* __restrict__ ok)
{
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= m) return;
  const isnark::vb::VbItem it = items[i];
  p29::F12 v;
  ok[i] = p29::combined_lane(it.a, it.b, z + 4 * (size_t)i, v) ? 1 : 0;
  f[i] = v;
}

// lane i < lanes: f[i] = Π of the Miller values of the pairs i, i + lanes, i + 2·lanes, … below n (identity inputs: 1)
__global__ __launch_bounds__(WG) void miller_strided_kernel(const fe* __restrict__ p, const fe2* __restrict__ q, uint64_t n, uint32_t lanes,
                                                            p29::F12* __restrict__ f)
{
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= lanes) return;
  p29::F12 acc = p29::f12_one();
  for (uint64_t k = i; k < n; k += lanes) {
    const fe px = p[2 * k], py = p[2 * k + 1];
    const fe2 qx = q[2 * k], qy = q[2 * k + 1];
    const bool pz = p29::std_is_zero(px) && p29::std_is_zero(py);
    const bool qz = p29::std_is_zero(qx.c0) && p29::std_is_zero(qx.c1) && p29::std_is_zero(qy.c0) && p29::std_is_zero(qy.c1);
    if (pz || qz) continue;
    acc = p29::f12_mul(acc, p29::miller_single(f29::from_std(px), f29::from_std(py), Fq2_29::load_std(qx), Fq2_29::load_std(qy)));
  }
  f[i] = acc;
}

// one pass of the product reduction over f[0 … n): f[i] ← f[i]·f[i + h] for i + h < n, h = ⌈n/2⌉.  A lane reads slots i and
// i + h ≥ h and writes slot i < n − h ≤ h: no slot is read by one lane and written by another.  Fq12 products are exact, so the
// value left in f[0] after the last pass does not depend on the shape of the tree.
__global__ __launch_bounds__(WG) void f12_product_pass_kernel(p29::F12* __restrict__ f, uint32_t n, uint32_t h)
{
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= n || h >= n - i) return; // i + h < n without overflow
  f[i] = p29::f12_mul(f[i], f[i + h]);
}

// out = f[0]^((p¹²−1)/r) (or 1 when there is no f[0]) in bn254_pairing's basis and form: one lane
__global__ void product_finish_kernel(const p29::F12* __restrict__ f, int have, fe* __restrict__ out)
{
  if (blockIdx.x || threadIdx.x) return;
  p29::f12_store_std(have ? p29::final_exp(f[0]) : p29::f12_one(), out);
}

// f[0] ← Π f[0 … n), n ≥ 1
hipError_t reduce_product(p29::F12* f, uint32_t n, hipStream_t st)
{
  while (n > 1) {
    const uint32_t h = (n + 1) / 2, work = n - h;
    hipLaunchKernelGGL(f12_product_pass_kernel, dim3((work + WG - 1) / WG), dim3(WG), 0, st, f, n, h);
    n = h;
  }
  return hipGetLastError();
}

bool os_random(uint8_t* out, size_t n)
{
  size_t got = 0;
  while (got < n) {
    const ssize_t r = getrandom(out + got, n - got, 0);
    if (r < 0) {
      if (errno == EINTR) continue;
      break;
    }
    got += (size_t)r;
  }
  if (got == n) return true;
  FILE* f = fopen("/dev/urandom", "rb");
  if (!f) return false;
  const size_t rd = fread(out, 1, n, f);
  fclose(f);
  return rd == n;
}

// The combined attempt over the live items.  0 with *accepted set, or the call's error code.
int combined_stage(const isnark::vb::Parsed& pz, int dev, const uint8_t seed[32], bool* accepted)
{
  using namespace isnark::vb;
  *accepted = false;
  const std::vector<int>& live = pz.live;
  const VbKey& key = pz.key;
  const size_t np = key.n_public, nl = live.size();

  // coefficients and signal sums on the pool: zₖ for live item k from its index in the caller's arrays, u₀ = Σ z, u_{j+1} = Σ z·sⱼ
  std::vector<uint32_t> z(4 * nl);
  const int tasks = (int)std::max<size_t>(1, std::min<size_t>(16, nl / 256));
  std::vector<std::vector<fe>> part(tasks, std::vector<fe>(np + 1, Fr::zero()));
  std::vector<isnark::HostTask> ht(tasks);
  for (int t = 0; t < tasks; t++) {
    const size_t lo = nl * t / tasks, hi = nl * (t + 1) / tasks;
    ht[t].fn = [&, t, lo, hi] {
      std::vector<fe>& u = part[t];
      for (size_t k = lo; k < hi; k++) {
        uint8_t c[16];
        isnark::combined_coefficient(seed, (uint64_t)live[k], c);
        fe zf = Fr::zero();
        for (int w = 0; w < 4; w++) zf.l[w] = z[4 * k + w] = (uint32_t)c[4 * w] | (uint32_t)c[4 * w + 1] << 8 | (uint32_t)c[4 * w + 2] << 16 | (uint32_t)c[4 * w + 3] << 24;
        u[0] = Fr::add(u[0], zf);
        const fe zm = Fr::to_mont(zf); // (z·R)·s·R⁻¹ = z·s
        const fe* s = pz.pub.data() + (size_t)live[k] * np;
        for (size_t j = 0; j < np; j++) u[j + 1] = Fr::add(u[j + 1], Fr::mul(zm, s[j]));
      }
    };
    if (t > 0) isnark::WorkerPool::get().run_or_inline(&ht[t]);
  }
  // the key's part on this thread meanwhile: γ₂ / δ₂ lines, IC shifted behind an identity entry (p29::combined_accept)
  const auto g2_zero = [](const fe2* q) { return p29::std_is_zero(q[0].c0) && p29::std_is_zero(q[0].c1) && p29::std_is_zero(q[1].c0) && p29::std_is_zero(q[1].c1); };
  std::vector<p29::Line> gl, dl;
  if (!g2_zero(key.gamma)) {
    gl.resize(p29::N_LINES);
    p29::precompute_lines(Fq2_29::load_std(key.gamma[0]), Fq2_29::load_std(key.gamma[1]), gl.data());
  }
  if (!g2_zero(key.delta)) {
    dl.resize(p29::N_LINES);
    p29::precompute_lines(Fq2_29::load_std(key.delta[0]), Fq2_29::load_std(key.delta[1]), dl.data());
  }
  std::vector<G1L::A> ic1(np + 2);
  std::vector<uint8_t> ic1z(np + 2);
  ic1[0] = {f29::one_m(), f29::one_m()};
  ic1z[0] = 1;
  for (size_t j = 0; j <= np; j++) {
    ic1z[j + 1] = p29::std_is_zero(key.ic[2 * j]) && p29::std_is_zero(key.ic[2 * j + 1]);
    ic1[j + 1] = {f29::from_std(key.ic[2 * j]), f29::from_std(key.ic[2 * j + 1])};
  }
  ht[0].fn();
  for (int t = 1; t < tasks; t++)
    if (ht[t].queued) isnark::WorkerPool::wait(&ht[t]);
  std::vector<fe> u(np + 1, Fr::zero());
  for (int t = 0; t < tasks; t++)
    for (size_t j = 0; j <= np; j++) u[j] = Fr::add(u[j], part[t][j]);

  // device part: the library's device and two pooled streams of its own (the MSM's workspace follows its stream's life): the
  // lanes on one, the MSM on the other — 4096 lanes are 64 waves on 1024 SIMDs, so the two can run side by side.  (Today they do
  // not: the downloads below go into pageable memory and hold this thread until the lanes are done — DESIGN §7a.)
  IcicleDevice want;
  memset(&want, 0, sizeof want);
  strcpy(want.type, "HIP");
  want.id = dev;
  const int prev = isnark::default_device_or_none();
  struct Restore {
    int d;
    ~Restore()
    {
      if (d < 0) return;
      IcicleDevice b;
      memset(&b, 0, sizeof b);
      strcpy(b.type, "HIP");
      b.id = d;
      (void)icicle_set_device(&b);
    }
  } restore{prev};
  if (icicle_set_device(&want) != ICICLE_SUCCESS) return fail((int)ICICLE_INVALID_DEVICE, "device: hipSetDevice: invalid device ordinal");
  icicleStreamHandle sh = nullptr;
  if (icicle_create_stream(&sh) != ICICLE_SUCCESS) return fail((int)ICICLE_UNKNOWN_ERROR, "device: stream creation failed");
  struct StreamGuard {
    icicleStreamHandle s;
    ~StreamGuard() { (void)icicle_destroy_stream(s); }
  } sg{sh};
  hipStream_t st = (hipStream_t)sh;
  icicleStreamHandle sh2 = nullptr;
  if (icicle_create_stream(&sh2) != ICICLE_SUCCESS) return fail((int)ICICLE_UNKNOWN_ERROR, "device: stream creation failed");
  StreamGuard sg2{sh2};
  const uint32_t cap = (uint32_t)std::min<size_t>(CHUNK, nl);
  DevBuf db;
  VbItem* d_items = db.alloc<VbItem>(cap);
  uint32_t* d_z = db.alloc<uint32_t>(4 * (size_t)cap);
  p29::F12* d_f = db.alloc<p29::F12>(cap);
  uint8_t* d_ok = db.alloc<uint8_t>(cap);
  if (!d_items || !d_z || !d_f || !d_ok) return device_fail(ICICLE_ALLOCATION_FAILED, "hipMalloc", hipErrorOutOfMemory);
  std::vector<VbItem> hitems(cap);
  std::vector<uint8_t> hok(cap);
  std::vector<bn254_scalar_t> msm_s(cap);
  std::vector<bn254_affine_t> msm_b(cap);
  p29::F12 prod = p29::f12_one(), part_prod, tail = p29::f12_one();
  bn254_projective_t sum_c;
  bool have_c = false;
  MSMConfig mc;
  memset(&mc, 0, sizeof mc);
  mc.stream = sh2;
  mc.precompute_factor = 1;
  mc.bitsize = 128;
  mc.batch_size = 1;
  hipError_t e;
  for (size_t base = 0; base < nl; base += cap) {
    const uint32_t m = (uint32_t)std::min<size_t>(cap, nl - base);
    for (uint32_t k = 0; k < m; k++) hitems[k] = pz.items[live[base + k]];
    if ((e = hipMemcpyAsync(d_items, hitems.data(), m * sizeof(VbItem), hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = hipMemcpyAsync(d_z, z.data() + 4 * base, (size_t)m * 16, hipMemcpyHostToDevice, st)) != hipSuccess)
      return device_fail(ICICLE_COPY_FAILED, "upload", e);
    hipLaunchKernelGGL(combined_lane_kernel, dim3((m + WG - 1) / WG), dim3(WG), 0, st, d_items, d_z, m, d_f, d_ok);
    if ((e = hipGetLastError()) != hipSuccess) return device_fail(ICICLE_UNKNOWN_ERROR, "combined_lane_kernel launch", e);
    if ((e = reduce_product(d_f, m, st)) != hipSuccess) return device_fail(ICICLE_UNKNOWN_ERROR, "f12_product_pass_kernel launch", e);
    if ((e = hipMemcpyAsync(hok.data(), d_ok, m, hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipMemcpyAsync(&part_prod, d_f, sizeof(p29::F12), hipMemcpyDeviceToHost, st)) != hipSuccess)
      return device_fail(ICICLE_COPY_FAILED, "download", e);
    // Σ zₖ·Cₖ of the chunk: the library's G1 MSM over 128-bit scalars.  An identity C takes part as 0·G₁.
    for (uint32_t k = 0; k < m; k++) {
      const VbItem& it = hitems[k];
      const bool c_zero = p29::std_is_zero(it.c[0]) && p29::std_is_zero(it.c[1]);
      memset(&msm_s[k], 0, sizeof msm_s[k]);
      if (!c_zero) memcpy(&msm_s[k], z.data() + 4 * (base + k), 16);
      memcpy(&msm_b[k].x, &it.c[0], 32);
      memcpy(&msm_b[k].y, &it.c[1], 32);
      if (c_zero) {
        msm_b[k].x.limbs[0] = 1;
        msm_b[k].y.limbs[0] = 2;
      }
    }
    bn254_projective_t chunk_c;
    if (eIcicleError me = bn254_msm(msm_s.data(), msm_b.data(), (int)m, &mc, &chunk_c)) {
      char msg[300];
      snprintf(msg, sizeof msg, "device: msm: %s", icicle_snark_last_error());
      return fail((int)me, msg);
    }
    if (have_c) bn254_ecadd(&sum_c, &chunk_c, &sum_c);
    else sum_c = chunk_c;
    have_c = true;
    if (base + m == nl) {
      // the Miller loop of the three fixed-G2 pairs needs the sums only, not the lanes' product
      bn254_affine_t sc_aff;
      bn254_to_affine(&sum_c, &sc_aff);
      fe sc[2];
      memcpy(&sc[0], &sc_aff.x, 32);
      memcpy(&sc[1], &sc_aff.y, 32);
      tail = p29::combined_tail_miller(key.alpha, key.beta, gl.empty() ? nullptr : gl.data(), dl.empty() ? nullptr : dl.data(), ic1.data(), ic1z.data(),
                                       (int)np, u.data(), sc);
    }
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return device_fail(ICICLE_SYNCHRONIZATION_FAILED, "combined_lane_kernel", e);
    for (uint32_t k = 0; k < m; k++)
      if (!hok[k]) return 0; // a pi_b outside the subgroup: the per-item stage names it
    prod = p29::f12_mul(prod, part_prod);
  }
  *accepted = p29::combined_finish(prod, tail);
  return 0;
}

} // namespace

ISNARK_API eIcicleError icicle_snark_pairing_product(const bn254_affine_t* p, const bn254_g2_affine_t* q, uint64_t n, icicleStreamHandle stream,
                                                     bn254_fq12_t* out)
{
  if (!out || (n && (!p || !q))) return ICICLE_INVALID_POINTER;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t lanes = (uint32_t)std::min<uint64_t>(n, PRODUCT_LANES);
  isnark::WsScoped<p29::F12> f;
  if (lanes) {
    if (f.alloc(lanes, st) != hipSuccess) return ICICLE_ALLOCATION_FAILED;
    hipLaunchKernelGGL(miller_strided_kernel, dim3((lanes + WG - 1) / WG), dim3(WG), 0, st, (const fe*)p, (const fe2*)q, n, lanes, f.p);
    (void)reduce_product(f.p, lanes, st);
  }
  hipLaunchKernelGGL(product_finish_kernel, dim3(1), dim3(WG), 0, st, f.p, lanes ? 1 : 0, (fe*)out);
  return isnark::check_launch("pairing_product");
}

ISNARK_API void groth16_verify_combined_coefficients(const uint8_t seed32[32], uint64_t first, uint64_t count, uint8_t* out16)
{
  if (!seed32 || !out16) return;
  for (uint64_t k = 0; k < count; k++) isnark::combined_coefficient(seed32, first + k, out16 + 16 * k);
}

ISNARK_API int groth16_verify_batch_combined(const char* const* proof_jsons, const char* const* public_jsons, int n, const char* vk_json,
                                             const char* device, const uint8_t* seed32, int32_t* verdicts, int32_t* path)
{
  using namespace isnark::vb;
  if (path) *path = 0;
  int dev = 0;
  bool done = false;
  const int rc0 = batch_prologue(proof_jsons, public_jsons, n, vk_json, device, verdicts, &dev, &done);
  if (done) {
    if (path && rc0 == 0) *path = 1; // n = 0: nothing was left to the per-item stage
    return rc0;
  }
  uint8_t seed[32];
  if (seed32) memcpy(seed, seed32, 32);
  else if (!os_random(seed, 32)) return fail(-3, "no randomness from the operating system (getrandom, /dev/urandom)");
  Parsed pz;
  if (int rc = parse_stage(proof_jsons, public_jsons, n, vk_json, verdicts, &pz, nullptr)) return rc;
  if (pz.live.empty()) {
    if (path) *path = 1;
    return 0;
  }
  const auto t0 = std::chrono::steady_clock::now();
  bool accepted = false;
  const int rc = combined_stage(pz, dev, seed, &accepted);
  double parse_ms = 0;
  groth16_verify_batch_last_timings(&parse_ms, nullptr);
  set_last_timings(parse_ms, ms_since(t0));
  if (rc) return rc;
  if (accepted) {
    for (int i : pz.live) verdicts[i] = 1;
    if (path) *path = 1;
    return 0;
  }
  DeviceKey dk;
  make_device_key(pz.key, &dk);
  return per_item_stage(pz, dk, dev, verdicts);
}
