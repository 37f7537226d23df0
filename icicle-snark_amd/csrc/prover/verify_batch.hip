// verify_batch.hip — Groth16 verification of many proofs against one verification key on one GPU, and the batched pairing
// primitive it is built from (pairing29.h: the host pairing's algorithm on the lazy radix-2^29 field).
//
//   icicle_snark_pairing_batch   out[i] = e(p[i], q[i]), one lane per pairing
//   groth16_verify_batch         per proof, one lane: [r]·pi_b = O, cpub = IC₀ + Σ pubⱼ·ICⱼ₊₁, one multi-Miller loop over
//                                (−A, B), (cpub, γ₂), (C, δ₂) with γ₂ / δ₂'s lines precomputed once per call on the host, the
//                                final exponentiation, and a comparison with conj(e(α₁, β₂)) (also computed once per call)
//
// The JSON texts are parsed on the host (pairing.cpp: vb::parse_vk / parse_item, the checks groth16_verify_json runs too) by up
// to 16 pooled workers; items that fail there keep their negative code and never reach the device.  The rest go to the device in
// chunks of at most CHUNK proofs, so device memory stays bounded whatever n is.  The per-key preparation is verify_host.h's
// PreparedKey; the device, the stream and the buffers of a call are verify_batch.h's DeviceSession.
#include <chrono>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../../include/groth16_prover.h"
#include "../common.h"
#include "../pairing29.h"
#include "../workers.h"
#include "verify_batch.h"

using namespace bn254;

namespace {

constexpr uint32_t CHUNK = 1u << 16;
constexpr int WG = 64;

__global__ __launch_bounds__(WG) void pairing_batch_kernel(const fe* __restrict__ p, const fe2* __restrict__ q, uint64_t n, fe* __restrict__ out)
{
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  const fe* pi = p + 2 * i;
  const fe2* qi = q + 2 * i;
  const fe P[2] = {pi[0], pi[1]};
  const fe2 Q[2] = {qi[0], qi[1]};
  const bool pz = p29::g1_std_is_zero(P), qz = p29::g2_std_is_zero(Q);
  const p29::F12 e = (pz || qz) ? p29::f12_one() : p29::pairing(f29::from_std(P[0]), f29::from_std(P[1]), Fq2_29::load_std(Q[0]), Fq2_29::load_std(Q[1]));
  p29::f12_store_std(e, out + 12 * i);
}

// items[i] / pub[j·m + i] (public signal j of item i) → verdict[i] ∈ {1, 0, −2}
__global__ __launch_bounds__(WG) void verify_batch_kernel(const p29::VerifyKey29* __restrict__ vk, const G1L::A* __restrict__ ic,
                                                          const uint8_t* __restrict__ ic_zero, const isnark::vb::VbItem* __restrict__ items,
                                                          const fe* __restrict__ pub, uint32_t m, int32_t* __restrict__ verdict)
{
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= m) return;
  const isnark::vb::VbItem it = items[i];
  verdict[i] = p29::verify_proof(*vk, ic, ic_zero, it.a, it.b, it.c, pub + i, m);
}

thread_local double g_last_parse_ms = 0, g_last_device_ms = 0;

} // namespace

ISNARK_API eIcicleError icicle_snark_pairing_batch(const bn254_affine_t* p, const bn254_g2_affine_t* q, uint64_t n, icicleStreamHandle stream,
                                                   bn254_fq12_t* out)
{
  if (n == 0) return ICICLE_SUCCESS;
  if (!p || !q || !out) return ICICLE_INVALID_POINTER;
  const uint64_t blocks = (n + WG - 1) / WG;
  hipLaunchKernelGGL(pairing_batch_kernel, dim3((uint32_t)blocks), dim3(WG), 0, (hipStream_t)stream, (const fe*)p, (const fe2*)q, n, (fe*)out);
  return isnark::check_launch("pairing_batch_kernel");
}

ISNARK_API void groth16_verify_batch_last_timings(double* parse_ms, double* device_ms)
{
  if (parse_ms) *parse_ms = g_last_parse_ms;
  if (device_ms) *device_ms = g_last_device_ms;
}

// ---- the stages of a batch call, shared with groth16_verify_batch_combined (verify_combined.hip) ------------------------------
namespace isnark {
namespace vb {

// "HIP", "CUDA" (device 0) or "HIP:k" / "CUDA:k"; −1 for anything else (a device list included)
int parse_one_device(const char* s)
{
  const char* colon = strchr(s, ':');
  const std::string type = colon ? std::string(s, colon) : std::string(s);
  if (type != "HIP" && type != "CUDA") return -1;
  if (!colon) return 0;
  const char* d = colon + 1;
  if (!*d || strlen(d) > 6 || strspn(d, "0123456789") != strlen(d)) return -1;
  return atoi(d);
}

void set_last_timings(double parse_ms, double device_ms)
{
  g_last_parse_ms = parse_ms;
  g_last_device_ms = device_ms;
}

int batch_prologue(const char* const* proof_jsons, const char* const* public_jsons, int n, const char* vk_json, const char* device,
                   const int32_t* verdicts, int* dev, bool* done)
{
  *done = true;
  g_last_parse_ms = g_last_device_ms = 0;
  if (n < 0) return fail(-3, "negative batch size");
  if (n == 0) return 0;
  if (!proof_jsons || !public_jsons || !vk_json || !device || !verdicts) return fail(-3, "null argument");
  *dev = parse_one_device(device);
  if (*dev < 0) return fail((int)ICICLE_INVALID_DEVICE, "device must be HIP, CUDA or HIP:k (one device)");
  *done = false;
  return 0;
}

int parse_stage(const char* const* proof_jsons, const char* const* public_jsons, int n, const char* vk_json, int32_t* verdicts, Parsed* out,
                const std::function<void(const VbKey&)>& meanwhile)
{
  const auto t0 = std::chrono::steady_clock::now();
  VbKey& key = out->key;
  if (int rc = parse_vk(vk_json, &key)) return rc;
  const size_t np = key.n_public;

  // items on the pool (≤ 16 contiguous ranges), the caller's per-key work on this thread meanwhile
  std::vector<VbItem>& items = out->items;
  std::vector<fe>& pub = out->pub;
  items.resize(n);
  pub.resize((size_t)n * np + 1);
  isnark::run_ranges(
    (size_t)n, 64,
    [&](int, size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; i++) verdicts[i] = parse_item(proof_jsons[i], public_jsons[i], np, &items[i], pub.data() + i * np, false);
    },
    [&] {
      if (meanwhile) meanwhile(key);
    });
  out->live.clear();
  out->live.reserve(n);
  for (int i = 0; i < n; i++)
    if (verdicts[i] == 0) out->live.push_back(i);
  g_last_parse_ms = ms_since(t0);
  return 0;
}

int per_item_stage(const Parsed& pz, PreparedKey& pk, int dev, int32_t* verdicts)
{
  const std::vector<int>& live = pz.live;
  const std::vector<VbItem>& items = pz.items;
  const std::vector<fe>& pub = pz.pub;
  const size_t np = pz.key.n_public;
  if (live.empty()) return 0;
  pk.need_target();
  DeviceSession ds;
  if (int rc = ds.open(dev, 1)) return rc;
  const hipStream_t st = ds.stream(0);
  hipError_t e;
  const uint32_t cap = (uint32_t)std::min<size_t>(CHUNK, live.size());
  DevBuf& db = ds.buf;
  p29::VerifyKey29* d_vk = db.alloc<p29::VerifyKey29>(1);
  G1L::A* d_ic = db.alloc<G1L::A>(np + 1);
  uint8_t* d_icz = db.alloc<uint8_t>(np + 1);
  VbItem* d_items = db.alloc<VbItem>(cap);
  fe* d_pub = db.alloc<fe>((size_t)cap * np + 1);
  int32_t* d_verdict = db.alloc<int32_t>(cap);
  if (!d_vk || !d_ic || !d_icz || !d_items || !d_pub || !d_verdict) return device_fail(ICICLE_ALLOCATION_FAILED, "hipMalloc", hipErrorOutOfMemory);
  hipEvent_t ev0, ev1;
  (void)hipEventCreate(&ev0);
  (void)hipEventCreate(&ev1);
  struct EvGuard {
    hipEvent_t a, b;
    ~EvGuard()
    {
      (void)hipEventDestroy(a);
      (void)hipEventDestroy(b);
    }
  } eg{ev0, ev1};
  (void)hipEventRecord(ev0, st);
  if ((e = hipMemcpyAsync(d_vk, pk.vk.data(), sizeof(p29::VerifyKey29), hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = hipMemcpyAsync(d_ic, pk.ic(), (np + 1) * sizeof(G1L::A), hipMemcpyHostToDevice, st)) != hipSuccess ||
      (e = hipMemcpyAsync(d_icz, pk.ic_zero(), np + 1, hipMemcpyHostToDevice, st)) != hipSuccess)
    return device_fail(ICICLE_COPY_FAILED, "upload", e);
  std::vector<VbItem> hitems(cap);
  std::vector<fe> hpub((size_t)cap * np + 1);
  std::vector<int32_t> hv(cap);
  for (size_t base = 0; base < live.size(); base += cap) {
    const uint32_t m = (uint32_t)std::min<size_t>(cap, live.size() - base);
    for (uint32_t k = 0; k < m; k++) {
      const int i = live[base + k];
      hitems[k] = items[i];
      for (size_t j = 0; j < np; j++) hpub[j * m + k] = pub[(size_t)i * np + j];
    }
    if ((e = hipMemcpyAsync(d_items, hitems.data(), m * sizeof(VbItem), hipMemcpyHostToDevice, st)) != hipSuccess ||
        (np && (e = hipMemcpyAsync(d_pub, hpub.data(), (size_t)m * np * sizeof(fe), hipMemcpyHostToDevice, st)) != hipSuccess))
      return device_fail(ICICLE_COPY_FAILED, "upload", e);
    hipLaunchKernelGGL(verify_batch_kernel, dim3((m + WG - 1) / WG), dim3(WG), 0, st, d_vk, d_ic, d_icz, d_items, d_pub, m, d_verdict);
    if ((e = hipGetLastError()) != hipSuccess) return device_fail(ICICLE_UNKNOWN_ERROR, "verify_batch_kernel launch", e);
    if ((e = hipMemcpyAsync(hv.data(), d_verdict, m * sizeof(int32_t), hipMemcpyDeviceToHost, st)) != hipSuccess)
      return device_fail(ICICLE_COPY_FAILED, "download", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return device_fail(ICICLE_SYNCHRONIZATION_FAILED, "verify_batch_kernel", e);
    for (uint32_t k = 0; k < m; k++) verdicts[live[base + k]] = hv[k];
  }
  (void)hipEventRecord(ev1, st);
  if ((e = hipEventSynchronize(ev1)) != hipSuccess) return device_fail(ICICLE_SYNCHRONIZATION_FAILED, "event", e);
  float dms = 0;
  (void)hipEventElapsedTime(&dms, ev0, ev1);
  g_last_device_ms += dms;
  return 0;
}

} // namespace vb
} // namespace isnark

ISNARK_API int groth16_verify_batch(const char* const* proof_jsons, const char* const* public_jsons, int n, const char* vk_json, const char* device,
                                    int32_t* verdicts)
{
  using namespace isnark::vb;
  int dev = 0;
  bool done = false;
  const int rc0 = batch_prologue(proof_jsons, public_jsons, n, vk_json, device, verdicts, &dev, &done);
  if (done) return rc0;
  Parsed pz;
  PreparedKey pk;
  const auto key_part = [&pk](const VbKey& key) {
    pk.prepare(key);
    pk.need_target();
  };
  if (int rc = parse_stage(proof_jsons, public_jsons, n, vk_json, verdicts, &pz, key_part)) return rc;
  return per_item_stage(pz, pk, dev, verdicts);
}
