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
//
// The attempt is combined_stage: named stages over one CombinedCtx.  The arithmetic of the sums and the per-key preparation are
// verify_host.h's (CombinedSums, PreparedKey — prepared once, and handed on to the fallback), the device, the two streams and the
// buffers are verify_batch.h's DeviceSession.
#include <chrono>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../../../include/groth16_prover.h"
#include "../common.h"
#include "../pairing29.h"
#include "../workers.h"
#include "device_call.h"
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
    const fe P[2] = {p[2 * k], p[2 * k + 1]};
    const fe2 Q[2] = {q[2 * k], q[2 * k + 1]};
    const bool pz = p29::g1_std_is_zero(P), qz = p29::g2_std_is_zero(Q);
    if (pz || qz) continue;
    acc = p29::f12_mul(acc, p29::miller_single(f29::from_std(P[0]), f29::from_std(P[1]), Fq2_29::load_std(Q[0]), Fq2_29::load_std(Q[1])));
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

// What the stages of one combined attempt share.  Lives on combined_stage's stack and outlives the pooled tasks of host_sums,
// which are waited for there.
struct CombinedCtx {
  const isnark::vb::Parsed& pz;
  isnark::vb::PreparedKey& pk;
  const uint8_t* const seed;
  const size_t np, nl; // public signals of the key, live items
  const uint32_t cap;  // live items per chunk
  // host_sums
  std::vector<uint32_t> z; // zₖ of live item k, four words
  std::vector<fe> u;       // u₀ = Σ z, u_{j+1} = Σ z·sⱼ
  // open_device: the lanes on stream 0, the MSM on stream 1 — 4096 lanes are 64 waves on 1024 SIMDs, so the two can run side by
  // side.  (Today they do not: the downloads of enqueue_lanes go into pageable memory and hold this thread until the lanes are
  // done — DESIGN §7a.)
  isnark::vb::DeviceSession ds;
  isnark::vb::VbItem* d_items = nullptr;
  uint32_t* d_z = nullptr;
  p29::F12* d_f = nullptr;
  uint8_t* d_ok = nullptr;
  std::vector<isnark::vb::VbItem> hitems;
  std::vector<uint8_t> hok;
  std::vector<bn254_scalar_t> msm_s;
  std::vector<bn254_affine_t> msm_b;
  MSMConfig mc;
  // what the chunks leave
  p29::F12 prod = p29::f12_one(), part_prod, tail = p29::f12_one();
  bn254_projective_t sum_c;
  bool have_c = false;

  CombinedCtx(const isnark::vb::Parsed& parsed, isnark::vb::PreparedKey& key, const uint8_t* seed32)
      : pz(parsed), pk(key), seed(seed32), np(parsed.key.n_public), nl(parsed.live.size()), cap((uint32_t)std::min<size_t>(CHUNK, parsed.live.size()))
  {
  }
};

// coefficients and signal sums on the pool (zₖ for live item k from its index in the caller's arrays), the key's part — γ₂ / δ₂
// lines, IC in lazy form — on this thread meanwhile
void host_sums(CombinedCtx& c)
{
  using isnark::vb::CombinedSums;
  c.z.resize(4 * c.nl);
  std::vector<CombinedSums> part(isnark::ranges_of(c.nl, 256), CombinedSums(c.np));
  isnark::run_ranges(
    c.nl, 256,
    [&](int t, size_t lo, size_t hi) {
      for (size_t k = lo; k < hi; k++) part[t].add_item(c.seed, (uint64_t)c.pz.live[k], c.pz.pub.data() + (size_t)c.pz.live[k] * c.np, &c.z[4 * k]);
    },
    [&] { c.pk.prepare(c.pz.key); });
  CombinedSums all(c.np);
  for (const CombinedSums& p : part) all.add(p);
  c.u = all.u;
}

int open_device(CombinedCtx& c, int dev)
{
  if (int rc = c.ds.open(dev, 2)) return rc;
  isnark::vb::DevBuf& db = c.ds.buf;
  c.d_items = db.alloc<isnark::vb::VbItem>(c.cap);
  c.d_z = db.alloc<uint32_t>(4 * (size_t)c.cap);
  c.d_f = db.alloc<p29::F12>(c.cap);
  c.d_ok = db.alloc<uint8_t>(c.cap);
  if (!c.d_items || !c.d_z || !c.d_f || !c.d_ok) return isnark::vb::device_fail(ICICLE_ALLOCATION_FAILED, "hipMalloc", hipErrorOutOfMemory);
  c.hitems.resize(c.cap);
  c.hok.resize(c.cap);
  c.msm_s.resize(c.cap);
  c.msm_b.resize(c.cap);
  c.mc = isnark::prover::msm_config(c.ds.streams[1], 128); // (scalars and bases on the host)
  return 0;
}

// the chunk's m live items from `base`: upload, lanes, product reduction, and the downloads of the subgroup flags and the product
int enqueue_lanes(CombinedCtx& c, size_t base, uint32_t m)
{
  using isnark::vb::device_fail;
  using isnark::vb::VbItem;
  const hipStream_t st = c.ds.stream(0);
  hipError_t e;
  for (uint32_t k = 0; k < m; k++) c.hitems[k] = c.pz.items[c.pz.live[base + k]];
  if ((e = hipMemcpyAsync(c.d_items, c.hitems.data(), m * sizeof(VbItem), hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = hipMemcpyAsync(c.d_z, c.z.data() + 4 * base, (size_t)m * 16, hipMemcpyHostToDevice, st)) != hipSuccess)
    return device_fail(ICICLE_COPY_FAILED, "upload", e);
  hipLaunchKernelGGL(combined_lane_kernel, dim3((m + WG - 1) / WG), dim3(WG), 0, st, c.d_items, c.d_z, m, c.d_f, c.d_ok);
  if ((e = hipGetLastError()) != hipSuccess) return device_fail(ICICLE_UNKNOWN_ERROR, "combined_lane_kernel launch", e);
  if ((e = reduce_product(c.d_f, m, st)) != hipSuccess) return device_fail(ICICLE_UNKNOWN_ERROR, "f12_product_pass_kernel launch", e);
  if ((e = hipMemcpyAsync(c.hok.data(), c.d_ok, m, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipMemcpyAsync(&c.part_prod, c.d_f, sizeof(p29::F12), hipMemcpyDeviceToHost, st)) != hipSuccess)
    return device_fail(ICICLE_COPY_FAILED, "download", e);
  return 0;
}

// Σ zₖ·Cₖ of the chunk, added to sum_c: the library's G1 MSM over 128-bit scalars.  An identity C takes part as 0·G₁.
int chunk_msm(CombinedCtx& c, size_t base, uint32_t m)
{
  for (uint32_t k = 0; k < m; k++) {
    const isnark::vb::VbItem& it = c.hitems[k];
    const bool c_zero = p29::g1_std_is_zero(it.c);
    memset(&c.msm_s[k], 0, sizeof c.msm_s[k]);
    if (!c_zero) memcpy(&c.msm_s[k], c.z.data() + 4 * (base + k), 16);
    memcpy(&c.msm_b[k].x, &it.c[0], 32);
    memcpy(&c.msm_b[k].y, &it.c[1], 32);
    if (c_zero) {
      c.msm_b[k].x.limbs[0] = 1;
      c.msm_b[k].y.limbs[0] = 2;
    }
  }
  bn254_projective_t chunk_c;
  if (eIcicleError me = bn254_msm(c.msm_s.data(), c.msm_b.data(), (int)m, &c.mc, &chunk_c)) {
    char msg[300];
    snprintf(msg, sizeof msg, "device: msm: %s", icicle_snark_last_error());
    return isnark::vb::fail((int)me, msg);
  }
  if (c.have_c) bn254_ecadd(&c.sum_c, &chunk_c, &c.sum_c);
  else c.sum_c = chunk_c;
  c.have_c = true;
  return 0;
}

// the Miller loop of the three fixed-G2 pairs: needs the sums only, not the lanes' product
void tail_miller(CombinedCtx& c)
{
  bn254_affine_t sc_aff;
  bn254_to_affine(&c.sum_c, &sc_aff);
  fe sc[2];
  memcpy(&sc[0], &sc_aff.x, 32);
  memcpy(&sc[1], &sc_aff.y, 32);
  const isnark::vb::VbKey& key = c.pz.key;
  c.tail = p29::combined_tail_miller(key.alpha, key.beta, c.pk.gamma_lines(), c.pk.delta_lines(), c.pk.ic1.data(), c.pk.ic1_zero.data(), (int)c.np,
                                     c.u.data(), sc);
}

// The combined attempt over the live items, pk left prepared for the fallback.  0 with *accepted set, or the call's error code.
int combined_stage(const isnark::vb::Parsed& pz, isnark::vb::PreparedKey& pk, int dev, const uint8_t seed[32], bool* accepted)
{
  *accepted = false;
  CombinedCtx c(pz, pk, seed);
  host_sums(c);
  if (int rc = open_device(c, dev)) return rc;
  for (size_t base = 0; base < c.nl; base += c.cap) {
    const uint32_t m = (uint32_t)std::min<size_t>(c.cap, c.nl - base);
    if (int rc = enqueue_lanes(c, base, m)) return rc;
    if (int rc = chunk_msm(c, base, m)) return rc;
    if (base + m == c.nl) tail_miller(c);
    const hipError_t e = hipStreamSynchronize(c.ds.stream(0));
    if (e != hipSuccess) return isnark::vb::device_fail(ICICLE_SYNCHRONIZATION_FAILED, "combined_lane_kernel", e);
    for (uint32_t k = 0; k < m; k++)
      if (!c.hok[k]) return 0; // a pi_b outside the subgroup: the per-item stage names it
    c.prod = p29::f12_mul(c.prod, c.part_prod);
  }
  *accepted = p29::combined_finish(c.prod, c.tail);
  return 0;
}

} // namespace

// ---- the three kernels above as the mixed-key verifier (verify_mixed.hip) enqueues them: declared in verify_batch.h ------------------
namespace isnark {
namespace vb {

hipError_t enqueue_combined_lanes(const VbItem* items, const uint32_t* z, uint32_t m, p29::F12* f, uint8_t* ok, hipStream_t st)
{
  hipLaunchKernelGGL(combined_lane_kernel, dim3((m + WG - 1) / WG), dim3(WG), 0, st, items, z, m, f, ok);
  return hipGetLastError();
}
hipError_t enqueue_miller_strided(const fe* p, const fe2* q, uint64_t n, uint32_t lanes, p29::F12* f, hipStream_t st)
{
  hipLaunchKernelGGL(miller_strided_kernel, dim3((lanes + WG - 1) / WG), dim3(WG), 0, st, p, q, n, lanes, f);
  return hipGetLastError();
}
hipError_t enqueue_product(p29::F12* f, uint32_t n, hipStream_t st) { return reduce_product(f, n, st); }

} // namespace vb
} // namespace isnark

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
  if (int rc = isnark::prover::seed_or_random(seed32, seed)) return fail(rc, isnark::prover::last_error_text()); // (the text through this entry's own channel)
  Parsed pz;
  if (int rc = parse_stage(proof_jsons, public_jsons, n, vk_json, verdicts, &pz, nullptr)) return rc;
  if (pz.live.empty()) {
    if (path) *path = 1;
    return 0;
  }
  const auto t0 = std::chrono::steady_clock::now();
  bool accepted = false;
  PreparedKey pk;
  const int rc = combined_stage(pz, pk, dev, seed, &accepted);
  double parse_ms = 0;
  groth16_verify_batch_last_timings(&parse_ms, nullptr);
  set_last_timings(parse_ms, ms_since(t0));
  if (rc) return rc;
  if (accepted) {
    for (int i : pz.live) verdicts[i] = 1;
    if (path) *path = 1;
    return 0;
  }
  return per_item_stage(pz, pk, dev, verdicts);
}
