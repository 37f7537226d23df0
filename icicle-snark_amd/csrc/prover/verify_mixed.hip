// verify_mixed.hip — a batch of Groth16 proofs of MANY keys, interleaved, decided by one randomised pairing equation.
//
//   groth16_vkset_new / _info / _free   a set of verification keys, parsed and checked once (vb::parse_vk) and kept on one device
//   groth16_verify_batch_mixed          Πᵢ e(−zᵢ·Aᵢ, Bᵢ) · Π_k [ e(S_C,k, δ₂,k) · e(S_pub,k, γ₂,k) · e(u₀,k·α₁,k, β₂,k) ] = 1
//                                       with u₀,k = Σ_{i∈k} zᵢ, u_{j+1,k} = Σ_{i∈k} zᵢ·sᵢⱼ, S_pub,k = Σⱼ uⱼ,k·ICⱼ,k, S_C,k = Σ_{i∈k} zᵢ·Cᵢ
//
// The coefficients are groth16_verify_batch_combined's (zᵢ from the seed and the item's index in the caller's arrays), so with
// one key this is that call's equation.  The lanes (subgroup test of pi_b, [zᵢ](−Aᵢ), one Miller loop) are verify_combined.hip's
// kernel over all live items in the caller's order, whatever their keys; the 3·K sums are ONE icicle_snark_msm_segmented launch
// on the second stream; the 3·K fixed-G2 pairs are verify_combined.hip's strided Miller kernel into slots behind the lanes'
// values; its product passes fold all slots, and one Fq12 comes down for the final exponentiation.
// When that equation fails, or a pi_b is flagged, the keys are decided one by one from the values already on the device:
// key_product_kernel multiplies each key's lane values and its three tail values, K Fq12 come down, and a key whose own equation
// holds and whose items all passed the subgroup test is accepted.  Only the other keys' items go through groth16_verify_batch's
// per-item stage.  Not here: bisection inside a failing key, several lanes per proof, more than one GPU.
#include <chrono>
#include <mutex>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../../include/groth16_prover.h"
#include "../common.h"
#include "../pairing29.h"
#include "../workers.h"
#include "device_call.h"
#include "sha256.h"
#include "verify_batch.h"

using namespace bn254;
using namespace isnark::vb;

// The keys as parsed, their per-item preparation (made when a key first falls back), and on the device the operands the mixed
// call's kernels read, in standard form with (0, 0) the identity — the encoding both kernels test, so no flag array goes with them:
//   d_g1   [ IC of every key, key after key | α₁ of every key ]        the tail of the segmented sum's point array
//   d_g2   [ δ₂ of every key | γ₂ of every key | β₂ of every key ]     miller_strided_kernel's q, in the order of the 3·K sums
struct Groth16VkSet {
  std::mutex mu; // one call at a time
  int dev = 0;
  std::vector<VbKey> keys;
  std::vector<size_t> n_public;
  std::vector<PreparedKey> prepared;
  std::vector<uint8_t> is_prepared;
  uint64_t g1_points = 0;
  fe* d_g1 = nullptr;
  fe2* d_g2 = nullptr;
};

namespace {

constexpr uint32_t CHUNK = 1u << 16; // live proofs per lane launch, as groth16_verify_batch
constexpr int KEY_WG = 64;

// one workgroup per key: out[k] = Π f[idx[j]] over idx_off[k] ≤ j < idx_off[k + 1] — the key's lane values and its three tail values
__global__ __launch_bounds__(KEY_WG) void key_product_kernel(const p29::F12* __restrict__ f, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ idx_off,
                                                             p29::F12* __restrict__ out)
{
  __shared__ p29::F12 sh[KEY_WG];
  const uint32_t k = blockIdx.x, t = threadIdx.x, hi = idx_off[k + 1];
  p29::F12 acc = p29::f12_one();
  for (uint32_t j = idx_off[k] + t; j < hi; j += KEY_WG) acc = p29::f12_mul(acc, f[idx[j]]);
  sh[t] = acc;
  __syncthreads();
  for (int h = KEY_WG / 2; h >= 1; h >>= 1) {
    if (t < (uint32_t)h) sh[t] = p29::f12_mul(sh[t], sh[t + h]);
    __syncthreads();
  }
  if (t == 0) out[k] = sh[0];
}

// What the stages of one mixed call share; lives on the entry point's stack and outlives the pooled tasks, which are waited for.
struct MixedCtx {
  Groth16VkSet& set;
  const char* const* proofs;
  const char* const* publics;
  const int32_t* key_of;
  const int n;
  const uint8_t* seed;
  int32_t* verdicts;
  const size_t K;
  // parse_items
  std::vector<VbItem> items;
  std::vector<size_t> pub_off; // item i's signals: pub[pub_off[i] …)
  std::vector<fe> pub;
  std::vector<int> live;
  // host_sums
  KeyGroups groups;
  MixedSegments seg;
  std::vector<uint32_t> z; // zₚ of live position p, four words
  std::vector<CombinedSums> u;
  // device
  DeviceSession ds;
  size_t nl = 0;
  uint32_t slots = 0; // nl lane values, then 3K tail values
  VbItem* d_items = nullptr;
  uint32_t* d_z = nullptr;
  p29::F12 *d_f = nullptr, *d_red = nullptr, *d_keyprod = nullptr;
  uint8_t* d_ok = nullptr;
  fe *d_pts = nullptr, *d_scal = nullptr, *d_sums = nullptr;
  uint32_t* d_idx = nullptr;
  std::vector<VbItem> hitems;
  std::vector<fe> h_pts, h_scal;
  std::vector<uint8_t> hok;
  std::vector<uint32_t> h_idx;
  std::vector<p29::F12> keyprod;
  p29::F12 prod;
  hipEvent_t sums_done = nullptr;

  MixedCtx(Groth16VkSet& s, const char* const* pj, const char* const* qj, const int32_t* ko, int count, const uint8_t* seed32, int32_t* out)
      : set(s), proofs(pj), publics(qj), key_of(ko), n(count), seed(seed32), verdicts(out), K(s.keys.size())
  {
  }
  ~MixedCtx()
  {
    if (sums_done) (void)hipEventDestroy(sums_done);
  }
};

// items on the pool, each with its own key's n_public; an item whose key index is out of range is refused here, on this thread
void parse_items(MixedCtx& c)
{
  c.items.resize(c.n);
  c.pub_off.resize((size_t)c.n + 1);
  size_t at = 0;
  for (int i = 0; i < c.n; i++) {
    c.pub_off[i] = at;
    const bool in_range = c.key_of[i] >= 0 && (size_t)c.key_of[i] < c.K;
    if (in_range) at += c.set.n_public[c.key_of[i]];
    else {
      char msg[120];
      snprintf(msg, sizeof msg, "item %d: key index %d is not in the set (%zu keys)", i, (int)c.key_of[i], c.K);
      c.verdicts[i] = fail(-2, msg);
    }
  }
  c.pub_off[c.n] = at;
  c.pub.resize(at + 1);
  isnark::run_ranges((size_t)c.n, 64, [&](int, size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      if (c.key_of[i] < 0 || (size_t)c.key_of[i] >= c.K) continue;
      c.verdicts[i] = parse_item(c.proofs[i], c.publics[i], c.set.n_public[c.key_of[i]], &c.items[i], c.pub.data() + c.pub_off[i], false);
    }
  });
  c.live.reserve(c.n);
  for (int i = 0; i < c.n; i++)
    if (c.verdicts[i] == 0) c.live.push_back(i);
  c.nl = c.live.size();
}

// coefficients and per-key signal sums on the pool: one MixedSums per range, added afterwards; then the segmented sum's layout
void host_sums(MixedCtx& c)
{
  c.groups = group_by_key(c.key_of, c.live, c.K);
  c.seg = mixed_segments(c.groups, c.set.n_public);
  c.z.resize(4 * c.nl);
  std::vector<MixedSums> part(isnark::ranges_of(c.nl, 256), MixedSums(c.set.n_public));
  isnark::run_ranges(c.nl, 256, [&](int t, size_t lo, size_t hi) {
    for (size_t p = lo; p < hi; p++) {
      const int i = c.live[p];
      part[t].add_item((size_t)c.key_of[i], c.seed, (uint64_t)i, c.pub.data() + c.pub_off[i], &c.z[4 * p]);
    }
  });
  for (size_t t = 1; t < part.size(); t++) part[0].add(part[t]);
  c.u = std::move(part[0].per_key);
}

int open_device(MixedCtx& c)
{
  if (int rc = c.ds.open(c.set.dev, 2)) return rc;
  DevBuf& db = c.ds.buf;
  const uint32_t cap = (uint32_t)std::min<size_t>(CHUNK, c.nl);
  c.slots = (uint32_t)(c.nl + 3 * c.K);
  c.d_items = db.alloc<VbItem>(cap);
  c.d_z = db.alloc<uint32_t>(4 * c.nl);
  c.d_f = db.alloc<p29::F12>(c.slots);
  c.d_red = db.alloc<p29::F12>(c.slots);
  c.d_ok = db.alloc<uint8_t>(c.nl);
  c.d_pts = db.alloc<fe>(2 * c.seg.total);
  c.d_scal = db.alloc<fe>(c.seg.total);
  c.d_sums = db.alloc<fe>(2 * 3 * c.K);
  if (!c.d_items || !c.d_z || !c.d_f || !c.d_red || !c.d_ok || !c.d_pts || !c.d_scal || !c.d_sums)
    return device_fail(ICICLE_ALLOCATION_FAILED, "hipMalloc", hipErrorOutOfMemory);
  const hipError_t e = hipEventCreateWithFlags(&c.sums_done, hipEventDisableTiming);
  if (e != hipSuccess) return device_fail(ICICLE_UNKNOWN_ERROR, "hipEventCreate", e);
  return 0;
}

// stream 0: every live item, in the caller's order, through combined_lane_kernel in chunks; the values stay in d_f[0 … nl)
int enqueue_lanes(MixedCtx& c)
{
  const hipStream_t st = c.ds.stream(0);
  hipError_t e;
  c.hitems.resize(c.nl);
  for (size_t p = 0; p < c.nl; p++) c.hitems[p] = c.items[c.live[p]];
  if ((e = hipMemcpyAsync(c.d_z, c.z.data(), c.nl * 16, hipMemcpyHostToDevice, st)) != hipSuccess) return device_fail(ICICLE_COPY_FAILED, "upload", e);
  for (size_t base = 0; base < c.nl; base += CHUNK) {
    const uint32_t m = (uint32_t)std::min<size_t>(CHUNK, c.nl - base);
    if ((e = hipMemcpyAsync(c.d_items, c.hitems.data() + base, m * sizeof(VbItem), hipMemcpyHostToDevice, st)) != hipSuccess)
      return device_fail(ICICLE_COPY_FAILED, "upload", e);
    if ((e = enqueue_combined_lanes(c.d_items, c.d_z + 4 * base, m, c.d_f + base, c.d_ok + base, st)) != hipSuccess)
      return device_fail(ICICLE_UNKNOWN_ERROR, "combined_lane_kernel launch", e);
  }
  return 0;
}

// stream 1: the operands of the 3·K sums (the items' C gathered key by key, the set's IC and α₁ behind them; zᵢ, uⱼ,k, u₀,k), the
// one segmented sum, and the Miller loops of (sum, δ₂ / γ₂ / β₂) into d_f[nl … nl + 3K)
int enqueue_sums_and_tail(MixedCtx& c)
{
  const hipStream_t st = c.ds.stream(1);
  const size_t K = c.K;
  hipError_t e;
  c.h_pts.resize(2 * c.nl + 1);
  c.h_scal.assign(c.seg.total, Fr::zero());
  for (size_t q = 0; q < c.nl; q++) {
    const uint32_t p = c.groups.pos[q];
    c.h_pts[2 * q] = c.hitems[p].c[0];
    c.h_pts[2 * q + 1] = c.hitems[p].c[1];
    for (int w = 0; w < 4; w++) c.h_scal[q].l[w] = c.z[4 * (size_t)p + w];
  }
  for (size_t k = 0; k < K; k++) {
    const uint64_t at = c.seg.offsets[K + k];
    for (size_t j = 0; j <= c.set.n_public[k]; j++) c.h_scal[at + j] = c.u[k].u[j];
    c.h_scal[c.seg.alpha_base + k] = c.u[k].u[0];
  }
  if ((c.nl && (e = hipMemcpyAsync(c.d_pts, c.h_pts.data(), 2 * c.nl * sizeof(fe), hipMemcpyHostToDevice, st)) != hipSuccess) ||
      (e = hipMemcpyAsync(c.d_pts + 2 * c.seg.ic_base, c.set.d_g1, 2 * c.set.g1_points * sizeof(fe), hipMemcpyDeviceToDevice, st)) != hipSuccess ||
      (e = hipMemcpyAsync(c.d_scal, c.h_scal.data(), c.seg.total * sizeof(fe), hipMemcpyHostToDevice, st)) != hipSuccess)
    return device_fail(ICICLE_COPY_FAILED, "upload", e);
  if (eIcicleError me = icicle_snark_msm_segmented((const bn254_affine_t*)c.d_pts, (const bn254_scalar_t*)c.d_scal, c.seg.offsets.data(), (uint32_t)(3 * K),
                                                   c.seg.bits.data(), 0, c.ds.streams[1], (bn254_affine_t*)c.d_sums)) {
    char msg[300];
    snprintf(msg, sizeof msg, "device: msm_segmented: %s", icicle_snark_last_error());
    return fail((int)me, msg);
  }
  if ((e = enqueue_miller_strided(c.d_sums, c.set.d_g2, 3 * K, (uint32_t)(3 * K), c.d_f + c.nl, st)) != hipSuccess)
    return device_fail(ICICLE_UNKNOWN_ERROR, "miller_strided_kernel launch", e);
  if ((e = hipEventRecord(c.sums_done, st)) != hipSuccess) return device_fail(ICICLE_UNKNOWN_ERROR, "hipEventRecord", e);
  return 0;
}

// stream 0, behind the tail: the product of all slots (on a copy: the per-key stage reads the values again), one Fq12 and the
// subgroup flags down, the final exponentiation on the host
int global_decision(MixedCtx& c, bool* accepted)
{
  const hipStream_t st = c.ds.stream(0);
  hipError_t e;
  c.hok.resize(c.nl);
  if ((e = hipStreamWaitEvent(st, c.sums_done, 0)) != hipSuccess) return device_fail(ICICLE_SYNCHRONIZATION_FAILED, "hipStreamWaitEvent", e);
  if ((e = hipMemcpyAsync(c.d_red, c.d_f, (size_t)c.slots * sizeof(p29::F12), hipMemcpyDeviceToDevice, st)) != hipSuccess)
    return device_fail(ICICLE_COPY_FAILED, "copy", e);
  if ((e = enqueue_product(c.d_red, c.slots, st)) != hipSuccess) return device_fail(ICICLE_UNKNOWN_ERROR, "f12_product_pass_kernel launch", e);
  if ((e = hipMemcpyAsync(c.hok.data(), c.d_ok, c.nl, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipMemcpyAsync(&c.prod, c.d_red, sizeof(p29::F12), hipMemcpyDeviceToHost, st)) != hipSuccess)
    return device_fail(ICICLE_COPY_FAILED, "download", e);
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return device_fail(ICICLE_SYNCHRONIZATION_FAILED, "combined_lane_kernel", e);
  if ((e = hipStreamSynchronize(c.ds.stream(1))) != hipSuccess) return device_fail(ICICLE_SYNCHRONIZATION_FAILED, "msm_segmented", e);
  bool flags = true;
  for (size_t p = 0; p < c.nl; p++) flags = flags && c.hok[p];
  *accepted = flags && p29::combined_finish(c.prod, p29::f12_one());
  return 0;
}

// key by key from the values on the device: holds[k] = key k has live items, its own equation holds and none of its pi_b is flagged
int per_key_decision(MixedCtx& c, std::vector<uint8_t>* holds)
{
  const hipStream_t st = c.ds.stream(0);
  const size_t K = c.K;
  hipError_t e;
  std::vector<uint32_t> idx_off(K + 1);
  c.h_idx.clear();
  for (size_t k = 0; k < K; k++) {
    idx_off[k] = (uint32_t)c.h_idx.size();
    for (uint32_t q = c.groups.off[k]; q < c.groups.off[k + 1]; q++) c.h_idx.push_back(c.groups.pos[q]);
    for (size_t part = 0; part < 3; part++) c.h_idx.push_back((uint32_t)(c.nl + part * K + k));
  }
  idx_off[K] = (uint32_t)c.h_idx.size();
  c.h_idx.insert(c.h_idx.end(), idx_off.begin(), idx_off.end()); // one upload: the list, then its offsets
  c.d_idx = c.ds.buf.alloc<uint32_t>(c.h_idx.size());
  c.d_keyprod = c.ds.buf.alloc<p29::F12>(K);
  if (!c.d_idx || !c.d_keyprod) return device_fail(ICICLE_ALLOCATION_FAILED, "hipMalloc", hipErrorOutOfMemory);
  c.keyprod.resize(K);
  if ((e = hipMemcpyAsync(c.d_idx, c.h_idx.data(), c.h_idx.size() * 4, hipMemcpyHostToDevice, st)) != hipSuccess)
    return device_fail(ICICLE_COPY_FAILED, "upload", e);
  hipLaunchKernelGGL(key_product_kernel, dim3((uint32_t)K), dim3(KEY_WG), 0, st, c.d_f, c.d_idx, c.d_idx + idx_off[K], c.d_keyprod);
  if ((e = hipGetLastError()) != hipSuccess) return device_fail(ICICLE_UNKNOWN_ERROR, "key_product_kernel launch", e);
  if ((e = hipMemcpyAsync(c.keyprod.data(), c.d_keyprod, K * sizeof(p29::F12), hipMemcpyDeviceToHost, st)) != hipSuccess)
    return device_fail(ICICLE_COPY_FAILED, "download", e);
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return device_fail(ICICLE_SYNCHRONIZATION_FAILED, "key_product_kernel", e);
  holds->assign(K, 0);
  isnark::run_ranges(K, 1, [&](int, size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; k++) {
      if (c.groups.count(k) == 0) continue;
      bool flags = true;
      for (uint32_t q = c.groups.off[k]; q < c.groups.off[k + 1]; q++) flags = flags && c.hok[c.groups.pos[q]];
      (*holds)[k] = flags && p29::combined_finish(c.keyprod[k], p29::f12_one());
    }
  });
  return 0;
}

// key k's live items through groth16_verify_batch's per-item stage, as a batch of their own
int fallback_key(MixedCtx& c, size_t k)
{
  Groth16VkSet& set = c.set;
  if (!set.is_prepared[k]) {
    set.prepared[k].prepare(set.keys[k]);
    set.is_prepared[k] = 1;
  }
  const size_t np = set.n_public[k], m = c.groups.count(k);
  Parsed pz;
  pz.key = set.keys[k];
  pz.items.resize(m);
  pz.pub.resize(m * np + 1);
  pz.live.resize(m);
  std::vector<int32_t> v(m, 0);
  for (size_t q = 0; q < m; q++) {
    const int i = c.live[c.groups.pos[c.groups.off[k] + q]];
    pz.items[q] = c.items[i];
    for (size_t j = 0; j < np; j++) pz.pub[q * np + j] = c.pub[c.pub_off[i] + j];
    pz.live[q] = (int)q;
  }
  if (int rc = per_item_stage(pz, set.prepared[k], set.dev, v.data())) return rc;
  for (size_t q = 0; q < m; q++) c.verdicts[c.live[c.groups.pos[c.groups.off[k] + q]]] = v[q];
  return 0;
}

int mixed_stages(MixedCtx& c, Groth16MixedReport* rep)
{
  host_sums(c);
  if (int rc = open_device(c)) return rc;
  if (int rc = enqueue_lanes(c)) return rc;
  if (int rc = enqueue_sums_and_tail(c)) return rc;
  bool accepted = false;
  if (int rc = global_decision(c, &accepted)) return rc;
  for (size_t k = 0; k < c.K; k++) rep->keys_live += c.groups.count(k) ? 1 : 0;
  if (accepted) {
    for (int i : c.live) c.verdicts[i] = 1;
    rep->path = 1;
    return 0;
  }
  std::vector<uint8_t> holds;
  if (int rc = per_key_decision(c, &holds)) return rc;
  for (size_t k = 0; k < c.K; k++) {
    if (c.groups.count(k) == 0) continue;
    if (holds[k]) {
      for (uint32_t q = c.groups.off[k]; q < c.groups.off[k + 1]; q++) c.verdicts[c.live[c.groups.pos[q]]] = 1;
      continue;
    }
    rep->keys_fallback++;
    if (int rc = fallback_key(c, k)) return rc;
  }
  return 0;
}

} // namespace

ISNARK_API int groth16_vkset_new(const char* const* vk_jsons, int n_keys, const char* device, Groth16VkSet** out)
{
  if (out) *out = nullptr;
  if (!vk_jsons || !device || !out || n_keys < 0) return fail(-3, "null argument");
  for (int k = 0; k < n_keys; k++)
    if (!vk_jsons[k]) return fail(-3, "null argument");
  const int dev = parse_one_device(device);
  if (dev < 0) return fail((int)ICICLE_INVALID_DEVICE, "device must be HIP, CUDA or HIP:k (one device)");
  Groth16VkSet* set = new (std::nothrow) Groth16VkSet;
  if (!set) return fail(-3, "out of memory");
  struct Guard {
    Groth16VkSet* s;
    ~Guard() { groth16_vkset_free(s); }
  } guard{set};
  const size_t K = (size_t)n_keys;
  set->dev = dev;
  set->keys.resize(K);
  set->prepared.resize(K);
  set->is_prepared.assign(K, 0);

  // every key through the one statement of the key checks, on the pool; a pooled thread's message is fetched on that thread
  std::vector<int> rc(K, 0);
  std::vector<std::string> text(K);
  isnark::run_ranges(K, 1, [&](int, size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; k++)
      if ((rc[k] = parse_vk(vk_jsons[k], &set->keys[k])) != 0) text[k] = groth16_verify_last_error();
  });
  for (size_t k = 0; k < K; k++)
    if (rc[k]) {
      const std::string msg = "key " + std::to_string(k) + ": " + text[k];
      return fail(rc[k], msg.c_str());
    }

  // only now the device: [IC … | α₁ …] and [δ₂ … | γ₂ … | β₂ …]
  std::vector<fe> g1;
  std::vector<fe2> g2(2 * 3 * K);
  for (size_t k = 0; k < K; k++) {
    const VbKey& key = set->keys[k];
    set->n_public.push_back(key.n_public);
    g1.insert(g1.end(), key.ic.begin(), key.ic.begin() + 2 * (key.n_public + 1));
    for (int h = 0; h < 2; h++) {
      g2[2 * k + h] = key.delta[h];
      g2[2 * (K + k) + h] = key.gamma[h];
      g2[2 * (2 * K + k) + h] = key.beta[h];
    }
  }
  for (size_t k = 0; k < K; k++) g1.insert(g1.end(), set->keys[k].alpha, set->keys[k].alpha + 2);
  set->g1_points = g1.size() / 2;
  DeviceSession ds;
  if (int e = ds.open(dev, 0)) return e;
  hipError_t e;
  if ((e = hipMalloc((void**)&set->d_g1, g1.size() * sizeof(fe) + 16)) != hipSuccess || (e = hipMalloc((void**)&set->d_g2, g2.size() * sizeof(fe2) + 16)) != hipSuccess)
    return device_fail(ICICLE_ALLOCATION_FAILED, "hipMalloc", e);
  if ((K && (e = hipMemcpy(set->d_g1, g1.data(), g1.size() * sizeof(fe), hipMemcpyHostToDevice)) != hipSuccess) ||
      (K && (e = hipMemcpy(set->d_g2, g2.data(), g2.size() * sizeof(fe2), hipMemcpyHostToDevice)) != hipSuccess))
    return device_fail(ICICLE_COPY_FAILED, "upload", e);
  guard.s = nullptr;
  *out = set;
  return 0;
}

ISNARK_API int groth16_vkset_info(const Groth16VkSet* set, int key, uint32_t* n_public)
{
  if (!set) return fail(-3, "null argument");
  if (key == -1) return (int)set->keys.size();
  if (key < 0 || (size_t)key >= set->keys.size() || !n_public) return fail(-3, "key index out of range");
  *n_public = (uint32_t)set->n_public[key];
  return 0;
}

ISNARK_API void groth16_vkset_free(Groth16VkSet* set)
{
  if (!set) return;
  {
    std::lock_guard<std::mutex> lk(set->mu); // a call still running on the set ends first
    if (set->d_g1) (void)hipFree(set->d_g1);
    if (set->d_g2) (void)hipFree(set->d_g2);
  }
  delete set;
}

ISNARK_API int groth16_verify_batch_mixed(Groth16VkSet* set, const char* const* proof_jsons, const char* const* public_jsons, const int32_t* key_of, int n,
                                          const uint8_t* seed32, int32_t* verdicts, Groth16MixedReport* report)
{
  Groth16MixedReport local;
  Groth16MixedReport* rep = report ? report : &local;
  memset(rep, 0, sizeof *rep);
  set_last_timings(0, 0);
  if (!set) return fail(-3, "null argument");
  if (n < 0) return fail(-3, "negative batch size");
  if (n == 0) {
    rep->path = 1; // nothing was left to the per-item stage
    return 0;
  }
  if (!proof_jsons || !public_jsons || !key_of || !verdicts) return fail(-3, "null argument");
  uint8_t seed[32];
  if (int rc = isnark::prover::seed_or_random(seed32, seed)) return fail(rc, isnark::prover::last_error_text());
  std::lock_guard<std::mutex> lk(set->mu);
  const auto t0 = std::chrono::steady_clock::now();
  MixedCtx c(*set, proof_jsons, public_jsons, key_of, n, seed, verdicts);
  parse_items(c);
  rep->parse_ms = ms_since(t0);
  if (c.live.empty()) {
    rep->path = 1;
    set_last_timings(rep->parse_ms, 0);
    return 0;
  }
  const auto t1 = std::chrono::steady_clock::now();
  const int rc = mixed_stages(c, rep);
  rep->device_ms = ms_since(t1);
  set_last_timings(rep->parse_ms, rep->device_ms);
  return rc;
}
