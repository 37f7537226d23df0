// msm_sort.hip — stage 1-3 of the MSM pipeline (see msm_impl.h): signed-digit recoding of the scalars and
// a counting sort of (point index | sign) by (window, bucket).
//
//  recode      (arithmetic and host plan: msm_recode.h, checked on the host by tests/msm_recode_check.cpp)
//              s ↦ digits d_w ∈ [−2^(c−1), 2^(c−1)) with Σ d_w 2^(cw) = s: scalars above (r − 1)/2 are
//              negated first (s ← r − s, sign flipped), then t = s + H with H = Σ_w 2^(cw+c−1) makes
//              d_w = ((t >> cw) & (2^c − 1)) − 2^(c−1) independent per window (W = ⌊254/c⌋ + 1 windows, the
//              top one cannot overflow; table mode narrows the top windows by one bit so that they tile the 254 bits
//              exactly, MsmGeom.wide).  Signed digits halve the bucket count of the reference's unsigned
//              digits (cuda_msm.cuh:166-203).
//  histogram   one global atomic per non-zero digit into counts[w·NB + |d| − 1]            (2 MiB of counters at c = 16: L2-resident)
//  scan        exclusive prefix sum, three small kernels (block sums / top / finish) + list of large buckets
//  scatter     second pass over the scalars; returning atomic on a cursor copy gives each entry its slot.
//              The order inside a bucket is arbitrary — addition is commutative, results are not affected.
// HBM traffic: 2 × 32 B per scalar read, 4 B per digit written (the key is implicit in the position): the
// reference moves 8-byte (key, value) pairs through three CUB radix sorts + RLE + scan (cuda_msm.cuh:401-485, :561-636).
// The shape of a sort — threshold, path, partitions, LDS sizes, workspace layouts — is msm_sort_shape (msm_sort_plan.h, walked on the
// host by tests/msm_sort_plan_check.cpp); msm_sort_run allocates what it says and enqueues one of enqueue_staged / _two_level / _global.
#include <atomic>
#include <mutex>
#include <string.h>

#include "msm_plan.h"
#include "msm_sort_plan.h"

using namespace bn254;

namespace isnark {

// one ring per device: the events are recorded on streams of the device whose thread issues the MSM, and an event only
// records on a stream of the device it was created on (a process that drives several GPUs has one prover thread per device)
constexpr int MSM_PROFILE_DEVICES = 16;
struct MsmProfileRing {
  MsmProfile slots[MSM_PROFILE_RING];
  uint64_t seq = 0;
};
static MsmProfileRing g_msm_rings[MSM_PROFILE_DEVICES];
static std::mutex g_msm_prof_mu;
static MsmProfileRing& msm_ring_of_active_device()
{
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= MSM_PROFILE_DEVICES) d = 0;
  return g_msm_rings[d];
}

MsmProfile* msm_profile_next()
{
  std::lock_guard<std::mutex> lk(g_msm_prof_mu);
  MsmProfileRing& r = msm_ring_of_active_device();
  MsmProfile* p = &r.slots[r.seq % MSM_PROFILE_RING];
  if (!p->ev[0])
    for (auto& e : p->ev) (void)hipEventCreate(&e);
  p->valid = false;
  p->has_sort_end = false;
  p->resolved = false;
  r.seq++;
  return p;
}

void msm_profile_own_init(MsmProfile* p)
{
  if (!p->ev[0])
    for (auto& e : p->ev) (void)hipEventCreate(&e);
  p->valid = false;
  p->has_sort_end = false;
  p->resolved = false;
}
void msm_profile_own_destroy(MsmProfile* p)
{
  for (auto& e : p->ev) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
}
static void msm_profile_resolve(const MsmProfile& p, float out_ms[5])
{
  for (int k = 0; k < 5; k++) out_ms[k] = 0;
  (void)hipEventElapsedTime(&out_ms[0], p.ev[0], p.ev[1]);
  (void)hipEventElapsedTime(&out_ms[1], p.ev[1], p.ev[2]);
  (void)hipEventElapsedTime(&out_ms[2], p.ev[2], p.ev[3]);
  (void)hipEventElapsedTime(&out_ms[3], p.ev[0], p.ev[3]);
  if (p.has_sort_end) (void)hipEventElapsedTime(&out_ms[4], p.ev[0], p.ev[4]);
  (void)hipGetLastError();
}
// the caller's streams are synchronised: the ring of the active device receives n resolved copies, in order (the last one is
// "back = 0" of icicle_snark_msm_profile); the ring's own events of those slots are left alone
void msm_profile_publish(const MsmProfile* src, int n)
{
  std::lock_guard<std::mutex> lk(g_msm_prof_mu);
  MsmProfileRing& r = msm_ring_of_active_device();
  for (int k = 0; k < n; k++) {
    MsmProfile* p = &r.slots[r.seq % MSM_PROFILE_RING];
    hipEvent_t keep[5];
    memcpy(keep, p->ev, sizeof keep);
    *p = src[k];
    memcpy(p->ev, keep, sizeof keep);
    p->resolved = true;
    for (float& m : p->ms) m = 0;
    if (src[k].valid && src[k].L) msm_profile_resolve(src[k], p->ms); // (L = 0: a slot that stands for "did not run", e.g. the head sort of an unsplit witness)
    r.seq++;
  }
}

namespace {

__device__ __forceinline__ fe ld_fe(const fe* p)
{
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4 a = q[0], b = q[1];
  fe r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  return r;
}

// scalar i of the vector → t = s' + H (9 limbs), neg = (s was replaced by r − s): the load here, the arithmetic in msm_recode.h
__device__ __forceinline__ void recode(const fe* scalars, uint32_t i, const MsmGeom& g, int mont, uint32_t t[9], uint32_t& neg)
{
  recode_fe(ld_fe(scalars + i), g, mont, t, neg);
}

// zero `n` u32 words (a kernel instead of hipMemsetAsync keeps every dependency on the compute queue)
__global__ __launch_bounds__(256) void msm_zero_kernel(uint32_t* __restrict__ p, uint32_t n)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = 0;
}

// Small digits of the two lowest windows are first counted in LDS: real witnesses are dominated by 0/1 and other
// small values, i.e. by a handful of buckets of windows 0/1; without this, a third of all global atomics of a
// witness-like scalar set hit ONE counter (measured 4.6 ms instead of 1 ms at L = 2^20).
constexpr uint32_t HIST_HOT = 512; // cached magnitudes per window, windows 0 and 1
__global__ __launch_bounds__(256) void msm_hist_kernel(const fe* __restrict__ scalars, uint32_t L, MsmGeom g, int mont, uint32_t* __restrict__ counts)
{
  __shared__ uint32_t hot[2 * HIST_HOT];
  for (uint32_t k = threadIdx.x; k < 2 * HIST_HOT; k += blockDim.x) hot[k] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < L) {
    uint32_t t[9], neg;
    recode(scalars, i, g, mont, t, neg);
    for (int w = 0; w < g.W; w++) {
      const uint32_t d = digit(t, w, g);
      if (d) {
        const uint32_t bk = (d & 0x7fffffffu) - 1;
        if ((g.tab || w < 2) && bk < HIST_HOT && bk < g.NB) atomicAdd(&hot[(g.tab ? 0 : w) * HIST_HOT + bk], 1u);
        else atomicAdd(&counts[bucket_id(g, w, bk)], 1u);
      }
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < 2 * HIST_HOT; k += blockDim.x) {
    const uint32_t v = hot[k];
    if (v) atomicAdd(&counts[bucket_id(g, (int)(k / HIST_HOT), k % HIST_HOT)], v);
  }
}

__global__ __launch_bounds__(256) void msm_scatter_kernel(const fe* __restrict__ scalars, uint32_t L, MsmGeom g, int mont, uint32_t* __restrict__ cursor, uint32_t* __restrict__ sorted)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  uint32_t t[9], neg;
  recode(scalars, i, g, mont, t, neg);
  for (int w = 0; w < g.W; w++) {
    const uint32_t d = digit(t, w, g);
    if (d) {
      const uint32_t pos = atomicAdd(&cursor[bucket_id(g, w, (d & 0x7fffffffu) - 1)], 1u);
      const uint32_t sign = (d >> 31) ^ neg;
      sorted[pos] = entry_idx(g, w, i) | (sign << 31);
    }
  }
}

// ---- exclusive scan of m counters: 2048 per workgroup (256 threads × 8) --------------------------
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* sh, uint32_t* total)
{
  const uint32_t tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (uint32_t d = 1; d < SCAN_T; d <<= 1) {
    uint32_t x = tid >= d ? sh[tid - d] : 0;
    __syncthreads();
    sh[tid] += x;
    __syncthreads();
  }
  if (total) *total = sh[SCAN_T - 1];
  return sh[tid] - v;
}

__global__ __launch_bounds__(SCAN_T) void msm_scan_sums_kernel(const uint32_t* __restrict__ counts, uint32_t m, uint32_t* __restrict__ bsum)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  __shared__ uint32_t sh[SCAN_T];
  const uint32_t base = blockIdx.x * SCAN_B + threadIdx.x * SCAN_E;
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_E; k++)
    if (base + k < m) s += counts[base + k];
  uint32_t total;
  block_exclusive_scan(s, sh, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
__global__ __launch_bounds__(SCAN_T) void msm_scan_top_kernel(uint32_t* bsum, uint32_t nblocks)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  __shared__ uint32_t sh[SCAN_T];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nblocks; base += SCAN_T) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nblocks ? bsum[i] : 0;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan(v, sh, &total);
    if (i < nblocks) bsum[i] = carry + ex;
    carry += total;
    __syncthreads();
  }
}
__global__ __launch_bounds__(SCAN_T) void msm_scan_finish_kernel(const uint32_t* __restrict__ counts, uint32_t m, const uint32_t* __restrict__ bsum, uint32_t* __restrict__ offsets,
                                                                  uint32_t* __restrict__ cursor, uint32_t thr, uint32_t* __restrict__ n_large, uint32_t* __restrict__ large_list,
                                                                  uint32_t* __restrict__ large_first, uint2* __restrict__ large_items, uint32_t item_cap)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  __shared__ uint32_t sh[SCAN_T];
  const uint32_t base = blockIdx.x * SCAN_B + threadIdx.x * SCAN_E;
  uint32_t v[SCAN_E], s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_E; k++) {
    v[k] = base + k < m ? counts[base + k] : 0;
    s += v[k];
  }
  uint32_t run = bsum[blockIdx.x] + block_exclusive_scan(s, sh, nullptr);
#pragma unroll
  for (int k = 0; k < SCAN_E; k++) {
    if (base + k < m) {
      offsets[base + k] = run;
      cursor[base + k] = run;
      if (v[k] > thr) {
        // a large bucket becomes ⌈count / MSM_LARGE_CHUNK⌉ work items, each summed by one workgroup
        const uint32_t li = atomicAdd(n_large, 1u);
        const uint32_t nch = (v[k] + MSM_LARGE_CHUNK - 1) / MSM_LARGE_CHUNK;
        const uint32_t first = atomicAdd(n_large + 2, nch);
        large_list[li] = base + k;
        large_first[li] = first;
        for (uint32_t q = 0; q < nch && first + q < item_cap; q++) large_items[first + q] = make_uint2(base + k, q);
      }
      run += v[k];
    }
  }
}

// generic finish of the 3-kernel exclusive scan: out[i] = bsum[block] + local exclusive prefix
__global__ __launch_bounds__(SCAN_T) void msm_scan_apply_kernel(const uint32_t* __restrict__ in, uint32_t m, const uint32_t* __restrict__ bsum, uint32_t* __restrict__ out)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  __shared__ uint32_t sh[SCAN_T];
  const uint32_t base = blockIdx.x * SCAN_B + threadIdx.x * SCAN_E;
  uint32_t v[SCAN_E], s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_E; k++) {
    v[k] = base + k < m ? in[base + k] : 0;
    s += v[k];
  }
  uint32_t run = bsum[blockIdx.x] + block_exclusive_scan(s, sh, nullptr);
#pragma unroll
  for (int k = 0; k < SCAN_E; k++) {
    if (base + k < m) out[base + k] = run;
    run += v[k];
  }
}

// ---- order buckets by decreasing size (counting sort on min(count, ORDER_BINS-1)) ----------------
// One thread accumulates one bucket; buckets of a wave should hold the same number of points or the
// wave runs for its largest bucket (random digits: Poisson sizes, a quarter of the lanes idle —
// SQ_THREAD_CYCLES_VALU / (64·SQ_ACTIVE_INST_VALU) = 0.77 before this ordering, 0.99 after).  The
// reference sorts bucket sizes with two more CUB radix sorts (cuda_msm.cuh:606-630); sizes are small
// integers, so a counting sort is enough: per-workgroup LDS histograms, one scan, LDS ranks — no global
// atomics (a first version with global atomics on ~100 hot counters cost 1.1 ms at 2^19 buckets).
__device__ __forceinline__ uint32_t order_key(uint32_t cnt) { return (uint32_t)ORDER_BINS - 1 - min(cnt, (uint32_t)ORDER_BINS - 1); } // ascending key = descending size
__global__ __launch_bounds__(ORDER_BINS) void msm_order_hist_kernel(const uint32_t* __restrict__ counts, uint32_t m, uint32_t nblk, uint32_t* __restrict__ blockhist)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  __shared__ uint32_t h[ORDER_BINS];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t b = blockIdx.x * ORDER_BINS + threadIdx.x;
  if (b < m) atomicAdd(&h[order_key(counts[b])], 1u);
  __syncthreads();
  blockhist[threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x]; // key-major
}
__global__ __launch_bounds__(ORDER_BINS) void msm_order_scatter_kernel(const uint32_t* __restrict__ counts, uint32_t m, uint32_t nblk, const uint32_t* __restrict__ scanned, uint32_t* __restrict__ order)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  __shared__ uint32_t h[ORDER_BINS];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t b = blockIdx.x * ORDER_BINS + threadIdx.x;
  if (b < m) {
    const uint32_t key = order_key(counts[b]);
    const uint32_t r = atomicAdd(&h[key], 1u);
    order[scanned[key * nblk + blockIdx.x] + r] = b;
  }
}

// ---- two-level scatter ----------------------------------------------------------------------------
// The one-level scatter writes 4 bytes at a random position of a 134 MB array per digit (PMC: WRITE_SIZE 2.0 GB for
// 134 MB of payload at L = 2^21 — every store is its own partial-line write).  Two levels keep every store inside
// a small, densely written region:
//  A  (msm_partition_kernel)   a workgroup takes 4096 scalars × all windows, counts its digits per PARTITION
//     (the top ≤8 bits of the bucket index; LDS atomics), reserves a run per partition with one global atomic,
//     and writes (index | low bucket bits | sign) into that run — ≈16 consecutive entries (64 B) per partition.
//  B  (msm_fine_count_kernel, msm_fine_place_kernel) 8 workgroups per partition (≈8 K entries, 32 KB, L2-resident)
//     count the ≤128 buckets of the partition in LDS, derive their offsets and place the entries at offset + rank.
constexpr int PA_THREADS = 256, PA_PER_THREAD = 16, PA_SCALARS = PA_THREADS * PA_PER_THREAD;

__global__ __launch_bounds__(PA_THREADS) void msm_partition_kernel(const fe* __restrict__ scalars, uint32_t L, MsmGeom g, int mont, int low_bits, uint32_t NP, uint32_t nparts,
                                                                    uint32_t* __restrict__ part_cursor, uint32_t* __restrict__ tmp)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  extern __shared__ uint32_t sh[];
  uint32_t* hist = sh;
  uint32_t* cur = sh + nparts;
  for (uint32_t p = threadIdx.x; p < nparts; p += PA_THREADS) hist[p] = 0;
  __syncthreads();
  const uint32_t first = blockIdx.x * PA_SCALARS;
  for (int u = 0; u < PA_PER_THREAD; u++) {
    const uint32_t i = first + u * PA_THREADS + threadIdx.x;
    if (i < L) {
      uint32_t t[9], neg;
      recode(scalars, i, g, mont, t, neg);
      for (int w = 0; w < g.W; w++) {
        const uint32_t d = digit(t, w, g);
        if (d) atomicAdd(&hist[bucket_id(g, w, (d & 0x7fffffffu) - 1) >> low_bits], 1u);
      }
    }
  }
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < nparts; p += PA_THREADS) {
    const uint32_t h = hist[p];
    cur[p] = h ? atomicAdd(&part_cursor[p], h) : 0;
  }
  __syncthreads();
  const uint32_t low_mask = (1u << low_bits) - 1;
  const int fs = 31 - low_bits; // entry = index bits [0, fs) | low bucket bits [fs, 31) | sign
  for (int u = 0; u < PA_PER_THREAD; u++) {
    const uint32_t i = first + u * PA_THREADS + threadIdx.x;
    if (i < L) {
      uint32_t t[9], neg;
      recode(scalars, i, g, mont, t, neg);
      for (int w = 0; w < g.W; w++) {
        const uint32_t d = digit(t, w, g);
        if (d) {
          const uint32_t bk = bucket_id(g, w, (d & 0x7fffffffu) - 1);
          const uint32_t pos = atomicAdd(&cur[bk >> low_bits], 1u);
          tmp[pos] = entry_idx(g, w, i) | ((bk & low_mask) << fs) | (((d >> 31) ^ neg) << 31);
        }
      }
    }
  }
}


// ---- counts and offsets from the partitions (no global histogram) ------------------------------------------------
// The per-digit global atomics of msm_hist_kernel (25.6 M at 1.6 M constraints, 1.1 ms, and the main source of
// interference with the kernels running beside the sort) are only needed by the one-level scatter.  The two-level
// path counts digits per PARTITION in LDS (coarse histogram: one global atomic per workgroup and partition), scans
// the ≤ 8192 partition totals in one workgroup, partitions, and then derives the per-bucket counts and offsets
// inside each partition (≤ 128 buckets, LDS).
__global__ __launch_bounds__(PA_THREADS) void msm_coarse_hist_kernel(const fe* __restrict__ scalars, uint32_t L, MsmGeom g, int mont, int low_bits, uint32_t nparts,
                                                                      uint32_t* __restrict__ part_count)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  extern __shared__ uint32_t sh[];
  for (uint32_t p = threadIdx.x; p < nparts; p += PA_THREADS) sh[p] = 0;
  __syncthreads();
  const uint32_t first = blockIdx.x * PA_SCALARS;
  for (int u = 0; u < PA_PER_THREAD; u++) {
    const uint32_t i = first + u * PA_THREADS + threadIdx.x;
    if (i < L) {
      uint32_t t[9], neg;
      recode(scalars, i, g, mont, t, neg);
      for (int w = 0; w < g.W; w++) {
        const uint32_t d = digit(t, w, g);
        if (d) atomicAdd(&sh[bucket_id(g, w, (d & 0x7fffffffu) - 1) >> low_bits], 1u);
      }
    }
  }
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < nparts; p += PA_THREADS) {
    const uint32_t h = sh[p];
    if (h) atomicAdd(&part_count[p], h);
  }
}
// exclusive scan of the partition totals, one workgroup (nparts ≤ 8192 = 256 threads × 32)
__global__ __launch_bounds__(SCAN_T) void msm_part_scan_kernel(const uint32_t* __restrict__ part_count, uint32_t nparts, uint32_t* __restrict__ part_start, uint32_t* __restrict__ part_cursor)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  __shared__ uint32_t sh[SCAN_T];
  const uint32_t per = (nparts + SCAN_T - 1) / SCAN_T, lo = threadIdx.x * per;
  uint32_t s = 0;
  for (uint32_t k = 0; k < per; k++)
    if (lo + k < nparts) s += part_count[lo + k];
  uint32_t total;
  uint32_t run = block_exclusive_scan(s, sh, &total);
  for (uint32_t k = 0; k < per; k++)
    if (lo + k < nparts) {
      part_start[lo + k] = run;
      part_cursor[lo + k] = run;
      run += part_count[lo + k];
    }
  if (threadIdx.x == 0) part_start[nparts] = total;
}
constexpr int PB_SPLIT = 8; // workgroups per partition (a witness-like scalar set puts a third of all entries into ONE partition)
__global__ __launch_bounds__(256) void msm_fine_count_kernel(const uint32_t* __restrict__ tmp, const uint32_t* __restrict__ part_start, int low_bits, uint32_t* __restrict__ counts)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  __shared__ uint32_t hist[128];
  const uint32_t part = blockIdx.x, b0 = part << low_bits, nbk = 1u << low_bits;
  const int fs = 31 - low_bits;
  const uint32_t fmask = nbk - 1;
  const uint32_t start = part_start[part], end = part_start[part + 1];
  const uint32_t stride = blockDim.x * gridDim.y, first = start + blockIdx.y * blockDim.x + threadIdx.x;
  if (first - threadIdx.x >= end) return;
  if (threadIdx.x < 128) hist[threadIdx.x] = 0;
  __syncthreads();
  for (uint32_t e = first; e < end; e += stride) atomicAdd(&hist[(tmp[e] >> fs) & fmask], 1u);
  __syncthreads();
  if (threadIdx.x < nbk) {
    const uint32_t h = hist[threadIdx.x];
    if (h) atomicAdd(&counts[b0 + threadIdx.x], h);
  }
}
// offsets of the partition's buckets (every workgroup recomputes them from the counts; split 0 publishes them and
// registers large buckets), then this workgroup's stripe of entries is placed.  cursor[] starts at zero.
__global__ __launch_bounds__(256) void msm_fine_place_kernel(const uint32_t* __restrict__ tmp, const uint32_t* __restrict__ part_start, const uint32_t* __restrict__ counts,
                                                             uint32_t* __restrict__ cursor, int low_bits, uint32_t thr, uint32_t* __restrict__ offsets, uint32_t* __restrict__ n_large,
                                                             uint32_t* __restrict__ large_list, uint32_t* __restrict__ large_first, uint2* __restrict__ large_items, uint32_t item_cap,
                                                             uint32_t* __restrict__ sorted)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  __shared__ uint32_t offs[128], hist[128], cur[128];
  const uint32_t part = blockIdx.x, b0 = part << low_bits, nbk = 1u << low_bits;
  const int fs = 31 - low_bits;
  const uint32_t fmask = nbk - 1;
  const uint32_t start = part_start[part], end = part_start[part + 1];
  const uint32_t mine = threadIdx.x < nbk ? counts[b0 + threadIdx.x] : 0;
  if (threadIdx.x < 128) {
    offs[threadIdx.x] = mine;
    hist[threadIdx.x] = 0;
  }
  __syncthreads();
  for (uint32_t d = 1; d < 128; d <<= 1) { // inclusive scan over ≤ 128 counters
    uint32_t x = 0;
    if (threadIdx.x < 128 && threadIdx.x >= d) x = offs[threadIdx.x - d];
    __syncthreads();
    if (threadIdx.x < 128) offs[threadIdx.x] += x;
    __syncthreads();
  }
  if (threadIdx.x < nbk) {
    const uint32_t o = start + offs[threadIdx.x] - mine;
    cur[threadIdx.x] = o;
    if (blockIdx.y == 0) {
      offsets[b0 + threadIdx.x] = o;
      if (mine > thr) {
        // a large bucket becomes ⌈count / MSM_LARGE_CHUNK⌉ work items, each summed by one workgroup
        const uint32_t li = atomicAdd(n_large, 1u);
        const uint32_t nch = (mine + MSM_LARGE_CHUNK - 1) / MSM_LARGE_CHUNK;
        const uint32_t firsti = atomicAdd(n_large + 2, nch);
        large_list[li] = b0 + threadIdx.x;
        large_first[li] = firsti;
        for (uint32_t q = 0; q < nch && firsti + q < item_cap; q++) large_items[firsti + q] = make_uint2(b0 + threadIdx.x, q);
      }
    }
  }
  __syncthreads();
  const uint32_t stride = blockDim.x * gridDim.y, first = start + blockIdx.y * blockDim.x + threadIdx.x;
  if (first - threadIdx.x >= end) return; // nothing for this workgroup (uniform across the workgroup)
  for (uint32_t e = first; e < end; e += stride) atomicAdd(&hist[(tmp[e] >> fs) & fmask], 1u);
  __syncthreads();
  if (threadIdx.x < nbk) {
    const uint32_t h = hist[threadIdx.x];
    cur[threadIdx.x] += h ? atomicAdd(&cursor[b0 + threadIdx.x], h) : 0;
  }
  __syncthreads();
  for (uint32_t e = first; e < end; e += stride) {
    const uint32_t v = tmp[e];
    const uint32_t pos = atomicAdd(&cur[(v >> fs) & fmask], 1u);
    sorted[pos] = v & ~(fmask << fs);
  }
}


// ---- LDS-staged two-pass sort (table mode, large sets) ------------------------------------------------------------------
// PMC of the two-level scatter above on MI355X (profiles/r02_pmc_*): the partition pass WRITES 640 MB for 83 MB of entries
// and the place pass 197 MB — a store instruction costs one 32-byte fabric write per sector it touches and the L2 does not
// merge the 4-byte stores of different instructions, so entries must leave a workgroup as runs of consecutive lanes.  Here
// both passes sort their tile in LDS first and copy it out run by run:
//  A  a tile of 1024 scalars counts its digits per PARTITION (top bits of the bucket; sort2_tile_hist), a column scan over the
//     tiles gives every (tile, partition) run its place (no atomics, deterministic), and the tile — ALL its windows, one recode —
//     is staged in LDS sorted by partition and written as ≤ P runs of ≈ 13 entries (sort2_tile_partition).  Entries carry the
//     scalar's index WITHIN THE TILE (10 bits), which leaves room for up to 17 low bucket bits in 32 bits;
//  B  partitions are cut into chunks of 12 K entries; a chunk is counting-sorted by its low bucket bits in LDS and written out as
//     runs of ≈ 23 entries per bucket.  A chunk is walked ROW BY ROW — the runs of the tiles that fed the partition, in tile
//     order, whose first entries are the partition's column of `off` — so the tile of an entry (needed to restore the global
//     scalar index) is known from the row being walked.  Per-bucket counts and offsets fall out of the chunk histograms.
// Round 5: every scalar is read and recoded TWICE per sort (histogram, placement) instead of three times (the tile used to be
// staged in two window groups), and no entry is located by binary search any more — rounds 2–4 searched the partition of every
// entry in pass A's copy-out (10 steps), its tile (11 steps) and its bucket (9 steps) in pass B: 138 / 205 VALU instructions per
// entry in the two big kernels (profiles/r04_pmc_kernels_1600k.txt).  The copy-outs are now run-cooperative: 16 lanes take one
// run (of a partition, a row, a bucket), so the run is known by construction and consecutive lanes still write consecutive
// words; runs longer than S2_LONG entries (the 0/1 wires of a real witness all land in one bucket) are left to the whole
// workgroup.  Launches per sort: 14 → 9 (zeroing folded into the histogram, the column scan's middle kernel into its first,
// the size order's histogram into the bucket scan, its three-kernel scan into one).
// HBM bytes: scalars 2 × 32·L, entries 4·L·W written and read twice, 4·L·W written — each once, in full lines.
// (tile, chunk and workgroup sizes: msm_sort_plan.h)

// largest i < n with a[i] <= x (a non-decreasing, a[0] <= x)
__device__ __forceinline__ uint32_t s2_upper(const uint32_t* a, uint32_t n, uint32_t x)
{
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}
// exclusive scan of n ≤ 64·per LDS counters by wave 0 (in → out, out[n] = total); the other waves wait at the caller's barrier
__device__ __forceinline__ void s2_wave_scan(const uint32_t* in, uint32_t* out, uint32_t n)
{
  if (threadIdx.x >= 64) return;
  const uint32_t per = (n + 63) / 64, lo = threadIdx.x * per;
  uint32_t s = 0;
  for (uint32_t k = 0; k < per; k++)
    if (lo + k < n) s += in[lo + k];
  uint32_t incl = s;
  for (int dlt = 1; dlt < 64; dlt <<= 1) {
    const uint32_t o = __shfl_up(incl, dlt, 64);
    if ((int)threadIdx.x >= dlt) incl += o;
  }
  uint32_t run = incl - s;
  for (uint32_t k = 0; k < per; k++)
    if (lo + k < n) {
      const uint32_t v = in[lo + k];
      out[lo + k] = run;
      run += v;
    }
  if (threadIdx.x == 63) out[n] = incl;
}
// Copy-out of `nruns` runs staged back to back in LDS (`start[k]` … `start[k + 1]` = run k in src; delta[k] = its place in dst minus
// start[k]): S2_GRP lanes per run, so that the run is known without a search and consecutive lanes write consecutive words;
// a run above S2_LONG entries is listed and copied by all threads afterwards.  `nlong` / `longs`: LDS scratch (counter zeroed by the
// caller before the barrier that precedes the call; ≤ S2_CHUNK / S2_LONG entries).
__device__ __forceinline__ void s2_copy_runs(const uint32_t* src, const uint32_t* start, const uint32_t* delta, uint32_t nruns, uint32_t* __restrict__ dst, uint32_t* nlong, uint32_t* longs)
{
  const uint32_t grp = threadIdx.x / S2_GRP, l = threadIdx.x % S2_GRP, ngrp = blockDim.x / S2_GRP;
  for (uint32_t k = grp; k < nruns; k += ngrp) {
    const uint32_t b0 = start[k], b1 = start[k + 1], d = delta[k];
    if (b1 - b0 > S2_LONG) {
      if (l == 0) longs[atomicAdd(nlong, 1u)] = k;
      continue;
    }
    for (uint32_t e = b0 + l; e < b1; e += S2_GRP) dst[e + d] = src[e];
  }
  __syncthreads();
  const uint32_t nl = *nlong;
  for (uint32_t j = 0; j < nl; j++) {
    const uint32_t k = longs[j], b0 = start[k], b1 = start[k + 1], d = delta[k];
    for (uint32_t e = b0 + threadIdx.x; e < b1; e += blockDim.x) dst[e + d] = src[e];
  }
}
constexpr uint32_t S2_MAXLONG = 1024 * 16 / S2_LONG + 2; // runs above S2_LONG that 16 K staged entries can hold

// pass A, step 1: digits of a tile counted per partition: cnt[tile·P + p].  Workgroup 0 also zeroes the plan's counters
// (n_large | tickets | the column scan's ticket): one launch less on a latency chain.
__global__ __launch_bounds__(256) void sort2_tile_hist_kernel(const fe* __restrict__ scalars, uint32_t L, MsmGeom g, int mont, int low_b, uint32_t P, uint32_t* __restrict__ cnt,
                                                              uint32_t* __restrict__ zero_p, uint32_t zero_n)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  extern __shared__ uint32_t sh[]; // [P]
  if (blockIdx.x == 0)
    for (uint32_t k = threadIdx.x; k < zero_n; k += 256) zero_p[k] = 0;
  for (uint32_t p = threadIdx.x; p < P; p += 256) sh[p] = 0;
  __syncthreads();
  const uint32_t first = blockIdx.x * S2_TILE;
  for (int u = 0; u < S2_TILE / 256; u++) {
    const uint32_t i = first + u * 256 + threadIdx.x;
    if (i < L) {
      uint32_t t[9], neg;
      recode(scalars, i, g, mont, t, neg);
      for (int w = 0; w < g.W; w++) {
        const uint32_t d = digit(t, w, g);
        if (d) atomicAdd(&sh[((d & 0x7fffffffu) - 1) >> low_b], 1u);
      }
    }
  }
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < P; p += 256) cnt[(size_t)blockIdx.x * P + p] = sh[p];
}
// column scan of cnt[R][P] over the rows, two short kernels: (1) sums per row group — and, in the workgroup that finishes last,
// the scan of the group sums, the partition starts and the chunk numbering — (2) running offsets written back.  Every load and
// store coalesced over p.
__global__ __launch_bounds__(256) void sort2_col_sum_kernel(const uint32_t* __restrict__ cnt, uint32_t R, uint32_t P, uint32_t* __restrict__ partial, uint32_t* __restrict__ ticket,
                                                            uint32_t* __restrict__ part_start, uint32_t* __restrict__ chunk_first)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  __shared__ uint32_t ps[4097], cf[4097]; // totals / chunk counts, scanned in place (last workgroup only)
  __shared__ uint32_t s_last;
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p < P) {
    const uint32_t rpg = (R + S2_RG - 1) / S2_RG, r0 = blockIdx.y * rpg, r1 = r0 + rpg < R ? r0 + rpg : R;
    uint32_t s = 0;
    for (uint32_t r = r0; r < r1; r++) s += cnt[(size_t)r * P + p];
    partial[(size_t)blockIdx.y * P + p] = s;
  }
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) s_last = atomicAdd(ticket, 1u) == gridDim.x * gridDim.y - 1 ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  for (uint32_t q = threadIdx.x; q < P; q += 256) {
    uint32_t t[S2_RG]; // all loads first: a load behind each store of the running sum would make this a chain of 32 round trips
#pragma unroll
    for (int gidx = 0; gidx < S2_RG; gidx++) t[gidx] = partial[(size_t)gidx * P + q];
    uint32_t run = 0;
#pragma unroll
    for (int gidx = 0; gidx < S2_RG; gidx++) {
      partial[(size_t)gidx * P + q] = run;
      run += t[gidx];
    }
    ps[q] = run;
    cf[q] = (run + S2_CHUNK - 1) / S2_CHUNK;
  }
  __syncthreads();
  s2_wave_scan(ps, ps, P);
  __syncthreads();
  s2_wave_scan(cf, cf, P);
  __syncthreads();
  for (uint32_t q = threadIdx.x; q <= P; q += 256) {
    part_start[q] = ps[q];
    chunk_first[q] = cf[q];
  }
}
// (out of place: the counts stay — the partition pass loads its row of them instead of recoding its scalars once more to count)
__global__ __launch_bounds__(256) void sort2_col_apply_kernel(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ off, uint32_t R, uint32_t P, const uint32_t* __restrict__ partial)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const uint32_t rpg = (R + S2_RG - 1) / S2_RG, r0 = blockIdx.y * rpg, r1 = r0 + rpg < R ? r0 + rpg : R;
  uint32_t run = partial[(size_t)blockIdx.y * P + p];
  for (uint32_t r = r0; r < r1; r++) {
    off[(size_t)r * P + p] = run;
    run += cnt[(size_t)r * P + p];
  }
}
// pass A, step 2: the tile's entries — every window, one recode — sorted by partition in LDS, then copied out run by run
template <int S2_THREADS>
__global__ __launch_bounds__(S2_THREADS) void sort2_tile_partition_kernel(const fe* __restrict__ scalars, uint32_t L, MsmGeom g, int mont, int low_b, uint32_t P,
                                                                           const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off, const uint32_t* __restrict__ part_start,
                                                                           uint32_t* __restrict__ tmp)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  extern __shared__ uint32_t sh[];
  __shared__ uint32_t nlong, longs[S2_MAXLONG];
  uint32_t* base = sh;          // [P + 1] exclusive prefix of the row's partition counts
  uint32_t* cur = sh + P + 1;   // [P] counts / rank counters, then the global position minus the local one
  uint32_t* buf = cur + P;      // [S2_TILE · W]
  const uint32_t row = blockIdx.x, first = row * S2_TILE;
  const uint32_t low_mask = (1u << low_b) - 1;
  // the row's digit counts per partition: what sort2_tile_hist_kernel counted for it
  for (uint32_t p = threadIdx.x; p < P; p += S2_THREADS) cur[p] = cnt[(size_t)row * P + p];
  if (threadIdx.x == 0) nlong = 0;
  __syncthreads();
  s2_wave_scan(cur, base, P);
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < P; p += S2_THREADS) cur[p] = 0;
  __syncthreads();
  for (int u = 0; u < S2_TILE / S2_THREADS; u++) {
    const uint32_t li = u * S2_THREADS + threadIdx.x, i = first + li;
    if (i < L) {
      uint32_t t[9], neg;
      recode(scalars, i, g, mont, t, neg);
      for (int w = 0; w < g.W; w++) {
        const uint32_t d = digit(t, w, g);
        if (d) {
          const uint32_t bk = (d & 0x7fffffffu) - 1, p = bk >> low_b;
          const uint32_t r = atomicAdd(&cur[p], 1u);
          buf[base[p] + r] = li | ((uint32_t)w << S2_W_SHIFT) | ((bk & low_mask) << S2_LOW_SHIFT) | (((d >> 31) ^ neg) << 31);
        }
      }
    }
  }
  __syncthreads();
  // cur[p] ← where the run of partition p starts in tmp, minus its start in buf
  for (uint32_t p = threadIdx.x; p < P; p += S2_THREADS) cur[p] = part_start[p] + off[(size_t)row * P + p] - base[p];
  __syncthreads();
  s2_copy_runs(buf, base, cur, P, tmp, &nlong, longs);
}
// the chunk a workgroup owns: partition, first entry, number of entries (false: beyond the last chunk)
__device__ __forceinline__ bool s2_chunk_of(uint32_t c, const uint32_t* __restrict__ part_start, const uint32_t* __restrict__ chunk_first, uint32_t P, uint32_t& p, uint32_t& start, uint32_t& n)
{
  __shared__ uint32_t s_p;
  if (c >= chunk_first[P]) return false;
  if (threadIdx.x == 0) s_p = s2_upper(chunk_first, P, c); // partitions without chunks share a value with their successor: the largest index wins, a non-empty one
  __syncthreads();
  p = s_p;
  const uint32_t k = c - chunk_first[p];
  start = part_start[p] + k * S2_CHUNK;
  const uint32_t end = part_start[p + 1];
  n = end - start < (uint32_t)S2_CHUNK ? end - start : (uint32_t)S2_CHUNK;
  return true;
}
// pass B, step 1: histogram of a chunk over the partition's 2^low_b buckets
template <int S2_THREADS>
__global__ __launch_bounds__(S2_THREADS) void sort2_chunk_hist_kernel(const uint32_t* __restrict__ tmp, const uint32_t* __restrict__ part_start, const uint32_t* __restrict__ chunk_first, uint32_t P, int low_b,
                                                                       uint32_t* __restrict__ chunk_hist)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  __shared__ uint32_t hist[1024];
  uint32_t p, start, n;
  if (!s2_chunk_of(blockIdx.x, part_start, chunk_first, P, p, start, n)) return;
  const uint32_t NL = 1u << low_b;
  for (uint32_t b = threadIdx.x; b < NL; b += S2_THREADS) hist[b] = 0;
  __syncthreads();
  for (uint32_t q = threadIdx.x; q < n; q += S2_THREADS) atomicAdd(&hist[(tmp[start + q] >> S2_LOW_SHIFT) & (NL - 1)], 1u);
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < NL; b += S2_THREADS) chunk_hist[(size_t)blockIdx.x * NL + b] = hist[b];
}
// pass B, step 2: one workgroup per partition, one thread per bucket: counts, offsets, the chunk's place inside each bucket,
// large buckets registered (as msm_fine_place_kernel does) — and the partition's histogram of bucket SIZES for the order by
// decreasing size (blockhist[key·P + p]: what msm_order_hist_kernel computes per 256 buckets in the other paths)
__global__ __launch_bounds__(1024) void sort2_bucket_scan_kernel(const uint32_t* __restrict__ chunk_hist, uint32_t* __restrict__ chunk_off, const uint32_t* __restrict__ part_start,
                                                                  const uint32_t* __restrict__ chunk_first, int low_b, uint32_t thr, uint32_t* __restrict__ counts, uint32_t* __restrict__ offsets,
                                                                  uint32_t* __restrict__ n_large, uint32_t* __restrict__ large_list, uint32_t* __restrict__ large_first, uint2* __restrict__ large_items,
                                                                  uint32_t item_cap, uint32_t* __restrict__ blockhist)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  __shared__ uint32_t sc[1024], oh[ORDER_BINS];
  const uint32_t NL = 1u << low_b, p = blockIdx.x, b = threadIdx.x, P = gridDim.x;
  for (uint32_t k = b; k < (uint32_t)ORDER_BINS; k += NL) oh[k] = 0;
  const uint32_t c0 = chunk_first[p], c1 = chunk_first[p + 1];
  uint32_t run = 0;
  for (uint32_t c = c0; c < c1; c++) {
    const uint32_t h = chunk_hist[(size_t)c * NL + b];
    chunk_off[(size_t)c * NL + b] = run;
    run += h;
  }
  sc[b] = run;
  __syncthreads();
  atomicAdd(&oh[order_key(run)], 1u);
  for (uint32_t d = 1; d < NL; d <<= 1) { // inclusive scan over the partition's buckets
    const uint32_t x = b >= d ? sc[b - d] : 0;
    __syncthreads();
    sc[b] += x;
    __syncthreads();
  }
  __syncthreads();
  for (uint32_t k = b; k < (uint32_t)ORDER_BINS; k += NL) blockhist[(size_t)k * P + p] = oh[k];
  const uint32_t bucket = (p << low_b) + b;
  counts[bucket] = run;
  offsets[bucket] = part_start[p] + sc[b] - run;
  if (run > thr) {
    const uint32_t li = atomicAdd(n_large, 1u);
    const uint32_t nch = (run + MSM_LARGE_CHUNK - 1) / MSM_LARGE_CHUNK;
    const uint32_t firsti = atomicAdd(n_large + 2, nch);
    large_list[li] = bucket;
    large_first[li] = firsti;
    for (uint32_t q = 0; q < nch && firsti + q < item_cap; q++) large_items[firsti + q] = make_uint2(bucket, q);
  }
}
// pass B, step 3: the chunk counting-sorted by bucket in LDS (entries rewritten with the global scalar index), copied out run
// by run.  The chunk is walked row by row: col[r] = first entry of row r's run inside the partition (the partition's column of
// `off`), 16 lanes per row — the tile of an entry is the row it is read from.
template <int S2_THREADS>
__global__ __launch_bounds__(S2_THREADS) void sort2_chunk_place_kernel(const uint32_t* __restrict__ tmp, const uint32_t* __restrict__ part_start, const uint32_t* __restrict__ chunk_first, uint32_t P, int low_b,
                                                                        const uint32_t* __restrict__ chunk_hist, const uint32_t* __restrict__ chunk_off, const uint32_t* __restrict__ offsets,
                                                                        const uint32_t* __restrict__ off, uint32_t R, MsmGeom g, uint32_t* __restrict__ sorted)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  extern __shared__ uint32_t sh[];
  __shared__ uint32_t nlong, longs[S2_MAXLONG], s_rows[2];
  const uint32_t NL = 1u << low_b;
  uint32_t* lbase = sh;             // [NL + 1]
  uint32_t* lcur = sh + NL + 1;     // [NL] counts / rank counters, then global position minus local one
  uint32_t* col = lcur + NL;        // [R + 1] first entry of every row's run inside the partition
  uint32_t* buf = col + R + 1;      // [S2_CHUNK]
  uint32_t p, start, n;
  if (!s2_chunk_of(blockIdx.x, part_start, chunk_first, P, p, start, n)) return;
  const uint32_t pstart = part_start[p], in_part = start - pstart; // position of the chunk inside its partition
  for (uint32_t r = threadIdx.x; r <= R; r += S2_THREADS) col[r] = r < R ? off[(size_t)r * P + p] : 0xffffffffu;
  for (uint32_t b = threadIdx.x; b < NL; b += S2_THREADS) lcur[b] = chunk_hist[(size_t)blockIdx.x * NL + b];
  if (threadIdx.x == 0) nlong = 0;
  __syncthreads();
  s2_wave_scan(lcur, lbase, NL);
  // rows the chunk touches (empty rows share their neighbour's value: the largest index wins, which is a row that holds the entry)
  if (threadIdx.x == 64) s_rows[0] = s2_upper(col, R, in_part);
  if (threadIdx.x == 128) s_rows[1] = s2_upper(col, R, in_part + n - 1);
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < NL; b += S2_THREADS) lcur[b] = 0;
  __syncthreads();
  {
    const uint32_t r_first = s_rows[0], r_last = s_rows[1], c_end = in_part + n;
    const uint32_t grp = threadIdx.x / S2_GRP, l = threadIdx.x % S2_GRP, ngrp = S2_THREADS / S2_GRP;
    auto place = [&](uint32_t r, uint32_t q) {
      const uint32_t v = tmp[pstart + q];
      const uint32_t b = (v >> S2_LOW_SHIFT) & (NL - 1);
      const uint32_t i = r * S2_TILE + (v & ((1u << S2_LI_BITS) - 1));
      const uint32_t w = (v >> S2_W_SHIFT) & 15u;
      const uint32_t rk = atomicAdd(&lcur[b], 1u);
      buf[lbase[b] + rk] = entry_idx(g, (int)w, i) | (v & 0x80000000u);
    };
    for (uint32_t r = r_first + grp; r <= r_last; r += ngrp) {
      const uint32_t lo = col[r] > in_part ? col[r] : in_part, hi = col[r + 1] < c_end ? col[r + 1] : c_end;
      if (hi > lo && hi - lo > S2_LONG) { // (a tile of 0/1 wires: hundreds of entries of one row in one partition)
        if (l == 0) longs[atomicAdd(&nlong, 1u)] = r;
        continue;
      }
      for (uint32_t q = lo + l; q < hi; q += S2_GRP) place(r, q);
    }
    __syncthreads();
    const uint32_t nl = nlong;
    for (uint32_t j = 0; j < nl; j++) {
      const uint32_t r = longs[j];
      const uint32_t lo = col[r] > in_part ? col[r] : in_part, hi = col[r + 1] < c_end ? col[r + 1] : c_end;
      for (uint32_t q = lo + threadIdx.x; q < hi; q += S2_THREADS) place(r, q);
    }
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < NL; b += S2_THREADS) lcur[b] = offsets[(p << low_b) + b] + chunk_off[(size_t)blockIdx.x * NL + b] - lbase[b];
  if (threadIdx.x == 0) nlong = 0;
  __syncthreads();
  s2_copy_runs(buf, lbase, lcur, NL, sorted, &nlong, longs);
}
// ---- order by decreasing size for the LDS-staged path: blockhist[key][P] (sort2_bucket_scan_kernel) → per key the exclusive
// prefix over the partitions (in place), and in the workgroup that finishes last the exclusive prefix of the key totals
__global__ __launch_bounds__(256) void sort2_order_scan_kernel(uint32_t* __restrict__ blockhist, uint32_t P, uint32_t* __restrict__ keytot, uint32_t* __restrict__ ticket)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  __shared__ uint32_t sh[SCAN_T];
  __shared__ uint32_t s_last;
  const uint32_t key = blockIdx.x, per = (P + 255) / 256, lo = threadIdx.x * per;
  uint32_t* row = blockhist + (size_t)key * P;
  uint32_t s = 0;
  for (uint32_t k = 0; k < per; k++)
    if (lo + k < P) s += row[lo + k];
  uint32_t total;
  uint32_t run = block_exclusive_scan(s, sh, &total);
  for (uint32_t k = 0; k < per; k++)
    if (lo + k < P) {
      const uint32_t v = row[lo + k];
      row[lo + k] = run;
      run += v;
    }
  if (threadIdx.x == 0) keytot[key] = total;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) s_last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  const uint32_t v = threadIdx.x < gridDim.x ? keytot[threadIdx.x] : 0; // ORDER_BINS = 256 keys = one per thread
  const uint32_t ex = block_exclusive_scan(v, sh, nullptr);
  if (threadIdx.x < gridDim.x) keytot[threadIdx.x] = ex;
}
__global__ __launch_bounds__(1024) void sort2_order_scatter_kernel(const uint32_t* __restrict__ counts, int low_b, const uint32_t* __restrict__ scanned, const uint32_t* __restrict__ keybase,
                                                                   uint32_t* __restrict__ order)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  __shared__ uint32_t h[ORDER_BINS];
  const uint32_t NL = 1u << low_b, p = blockIdx.x, P = gridDim.x;
  for (uint32_t k = threadIdx.x; k < (uint32_t)ORDER_BINS; k += NL) h[k] = 0;
  __syncthreads();
  const uint32_t b = (p << low_b) + threadIdx.x;
  const uint32_t key = order_key(counts[b]);
  const uint32_t r = atomicAdd(&h[key], 1u);
  order[keybase[key] + scanned[(size_t)key * P + p] + r] = b;
}

} // namespace

MsmGeom msm_geometry(uint32_t L, int c_cfg, int tab, int bits, int pf) { return msm_geometry_plan(L, c_cfg, tab, bits, pf); }

namespace {
// what the enqueue stages share: the shape, the caller's plan with its pointers carved, and the workspace regions no caller sees
struct SortCall {
  const SortShape& sh;
  SortPlan* pl;
  const fe* d_scalars;
  int mont_sc;
  hipStream_t s;
  uint32_t *cursor, *s2tickets, *bsum, *part_count, *part_start, *part_cursor, *blockhist, *obsum;
};

// LDS-staged path, nine launches: histogram (+ zeroing of n_large | tickets | this path's tickets), column scan (2), partition, chunk
// histogram, bucket scan (+ histogram of the bucket sizes), placement, size order (2).  `w`: its workspace (SortShape::s2), `tmp`: L·W entries
LdsCapOnce g_s2_cap; // both widths of the two kernels with dynamic LDS, at the first staged sort of a device
template <int THREADS>
eIcicleError enqueue_staged(const SortCall& c, uint32_t* w, uint32_t* tmp)
{
  int dev = 0;
  (void)hipGetDevice(&dev);
  ICICLE_TRY(g_s2_cap.raise(dev, (int)S2_LDS_MAX, sort2_tile_partition_kernel<S2_THREADS_WIDE>, sort2_chunk_place_kernel<S2_THREADS_WIDE>, sort2_tile_partition_kernel<S2_THREADS_CROWDED>,
                            sort2_chunk_place_kernel<S2_THREADS_CROWDED>));
  const SortShape& sh = c.sh;
  const MsmGeom& g = sh.g;
  SortPlan* pl = c.pl;
  hipStream_t s = c.s;
  const uint32_t L = pl->L, P = 1u << sh.pb, NL = 1u << sh.low, R = sh.ntiles;
  uint32_t *cnt = w + sh.s2.cnt, *off = w + sh.s2.off /* first entry of every (row, partition) run inside its partition */, *partial = w + sh.s2.partial;
  uint32_t *pstart = w + sh.s2.pstart, *cfirst = w + sh.s2.cfirst, *chist = w + sh.s2.chist, *coff = w + sh.s2.coff, *bh = w + sh.s2.bh, *keytot = w + sh.s2.keytot;
  const dim3 cgrid((P + 255) / 256, S2_RG);
  hipLaunchKernelGGL(sort2_tile_hist_kernel, dim3(R), dim3(256), (size_t)P * 4, s, c.d_scalars, L, g, c.mont_sc, sh.low, P, cnt, pl->n_large, 4u + TK + S2TK);
  hipLaunchKernelGGL(sort2_col_sum_kernel, cgrid, dim3(256), 0, s, cnt, R, P, partial, c.s2tickets, pstart, cfirst);
  hipLaunchKernelGGL(sort2_col_apply_kernel, cgrid, dim3(256), 0, s, cnt, off, R, P, partial);
  hipLaunchKernelGGL(sort2_tile_partition_kernel<THREADS>, dim3(R), dim3(THREADS), sh.lds_a, s, c.d_scalars, L, g, c.mont_sc, sh.low, P, cnt, off, pstart, tmp);
  hipLaunchKernelGGL(sort2_chunk_hist_kernel<THREADS>, dim3(sh.maxchunks), dim3(THREADS), 0, s, tmp, pstart, cfirst, P, sh.low, chist);
  hipLaunchKernelGGL(sort2_bucket_scan_kernel, dim3(P), dim3(NL), 0, s, chist, coff, pstart, cfirst, sh.low, sh.large_thr, pl->counts, pl->offsets, pl->n_large, pl->large_list, pl->large_first,
                     pl->large_items, pl->item_cap, bh);
  hipLaunchKernelGGL(sort2_chunk_place_kernel<THREADS>, dim3(sh.maxchunks), dim3(THREADS), sh.lds_b, s, tmp, pstart, cfirst, P, sh.low, chist, coff, pl->offsets, off, R, g, pl->sorted);
  hipLaunchKernelGGL(sort2_order_scan_kernel, dim3(ORDER_BINS), dim3(256), 0, s, bh, P, keytot, c.s2tickets + 1);
  hipLaunchKernelGGL(sort2_order_scatter_kernel, dim3(P), dim3(NL), 0, s, pl->counts, sh.low, bh, keytot, pl->order);
  return check_launch("msm_sort (LDS-staged)");
}

// both other paths start from zeroed counters
void enqueue_zero(const SortCall& c)
{
  const uint32_t nb = c.sh.nbuckets;
  unsigned zb = (3 * nb + 255) / 256;
  if (zb > 1024) zb = 1024;
  hipLaunchKernelGGL(msm_zero_kernel, dim3(zb), dim3(256), 0, c.s, c.pl->counts, 3 * nb); // counts | offsets | cursor
  hipLaunchKernelGGL(msm_zero_kernel, dim3(8), dim3(256), 0, c.s, c.pl->n_large, 4u + TK + S2TK + c.sh.nblocks + c.sh.nparts); // n_large | tickets | bsum | part_count
}
// two-level path: counts and offsets come out of the partitions, no per-digit global atomics
void enqueue_two_level(const SortCall& c, uint32_t* tmp)
{
  const SortShape& sh = c.sh;
  SortPlan* pl = c.pl;
  const uint32_t L = pl->L, nparts = sh.nparts;
  enqueue_zero(c);
  const unsigned pgrid = (L + PA_SCALARS - 1) / PA_SCALARS;
  if (L) hipLaunchKernelGGL(msm_coarse_hist_kernel, dim3(pgrid), dim3(PA_THREADS), (size_t)nparts * 4, c.s, c.d_scalars, L, sh.g, c.mont_sc, sh.low_bits, nparts, c.part_count);
  hipLaunchKernelGGL(msm_part_scan_kernel, dim3(1), dim3(SCAN_T), 0, c.s, c.part_count, nparts, c.part_start, c.part_cursor);
  if (L) {
    if ((size_t)nparts * 8 > 65536) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(msm_partition_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)nparts * 8));
    hipLaunchKernelGGL(msm_partition_kernel, dim3(pgrid), dim3(PA_THREADS), (size_t)nparts * 8, c.s, c.d_scalars, L, sh.g, c.mont_sc, sh.low_bits, sh.NP, nparts, c.part_cursor, tmp);
    hipLaunchKernelGGL(msm_fine_count_kernel, dim3(nparts, PB_SPLIT), dim3(256), 0, c.s, tmp, c.part_start, sh.low_bits, pl->counts);
  }
  hipLaunchKernelGGL(msm_fine_place_kernel, dim3(nparts, PB_SPLIT), dim3(256), 0, c.s, tmp, c.part_start, pl->counts, c.cursor, sh.low_bits, sh.large_thr, pl->offsets, pl->n_large, pl->large_list,
                     pl->large_first, pl->large_items, pl->item_cap, pl->sorted);
}
// global-histogram path: histogram, scan (+ list of large buckets), scatter
void enqueue_global(const SortCall& c)
{
  const SortShape& sh = c.sh;
  SortPlan* pl = c.pl;
  const uint32_t L = pl->L, nb = sh.nbuckets;
  enqueue_zero(c);
  const unsigned lgrid = (L + 255) / 256;
  if (L) hipLaunchKernelGGL(msm_hist_kernel, dim3(lgrid), dim3(256), 0, c.s, c.d_scalars, L, sh.g, c.mont_sc, pl->counts);
  hipLaunchKernelGGL(msm_scan_sums_kernel, dim3(sh.nblocks), dim3(SCAN_T), 0, c.s, pl->counts, nb, c.bsum);
  hipLaunchKernelGGL(msm_scan_top_kernel, dim3(1), dim3(SCAN_T), 0, c.s, c.bsum, sh.nblocks);
  hipLaunchKernelGGL(msm_scan_finish_kernel, dim3(sh.nblocks), dim3(SCAN_T), 0, c.s, pl->counts, nb, c.bsum, pl->offsets, c.cursor, sh.large_thr, pl->n_large, pl->large_list, pl->large_first, pl->large_items, pl->item_cap);
  if (L) hipLaunchKernelGGL(msm_scatter_kernel, dim3(lgrid), dim3(256), 0, c.s, c.d_scalars, L, sh.g, c.mont_sc, c.cursor, pl->sorted);
}
// bucket ids by decreasing size (the staged path orders them itself)
eIcicleError enqueue_size_order(const SortCall& c)
{
  const SortShape& sh = c.sh;
  hipLaunchKernelGGL(msm_order_hist_kernel, dim3(sh.oblk), dim3(ORDER_BINS), 0, c.s, c.pl->counts, sh.nbuckets, sh.oblk, c.blockhist);
  hipLaunchKernelGGL(msm_scan_sums_kernel, dim3(sh.oscan), dim3(SCAN_T), 0, c.s, c.blockhist, sh.om, c.obsum);
  hipLaunchKernelGGL(msm_scan_top_kernel, dim3(1), dim3(SCAN_T), 0, c.s, c.obsum, sh.oscan);
  hipLaunchKernelGGL(msm_scan_apply_kernel, dim3(sh.oscan), dim3(SCAN_T), 0, c.s, c.blockhist, sh.om, c.obsum, c.blockhist);
  hipLaunchKernelGGL(msm_order_scatter_kernel, dim3(sh.oblk), dim3(ORDER_BINS), 0, c.s, c.pl->counts, sh.nbuckets, sh.oblk, c.blockhist, c.pl->order);
  return check_launch("msm_sort");
}
} // namespace

eIcicleError msm_sort_run(const fe* d_scalars, uint32_t L, int c_cfg, int lbf, int mont_sc, hipStream_t s, SortPlan* pl, int tab, int bits, int pf, uint64_t entries_hint, bool crowded)
{
  const SortShape sh = msm_sort_shape(L, c_cfg, lbf, tab, bits, pf, entries_hint);
  pl->g = sh.g;
  pl->L = L;
  pl->stream = s;
  pl->nbuckets = sh.nbuckets;
  pl->large_thr = sh.large_thr;
  if (sh.err != ICICLE_SUCCESS) {
    set_last_error("%s", sh.msg);
    return sh.err;
  }
  pl->item_cap = sh.item_cap;
  // workspace, entries, and the scatter buffer of whichever path needs one
  HIP_TRY(ws_alloc((void**)&pl->ws, sh.ws.total * 4, s), ICICLE_ALLOCATION_FAILED);
  HIP_TRY(ws_alloc((void**)&pl->sorted, (size_t)(sh.nentries ? sh.nentries : 1) * 4, s), ICICLE_ALLOCATION_FAILED);
  WsScoped<uint32_t> tmp, s2ws, s2tmp;
  if (sh.two_level_ok) HIP_TRY(tmp.alloc((size_t)sh.nentries, s), ICICLE_ALLOCATION_FAILED);
  if (sh.path == SORT_STAGED) {
    HIP_TRY(s2ws.alloc(sh.s2.total, s), ICICLE_ALLOCATION_FAILED);
    if (!tmp.p) HIP_TRY(s2tmp.alloc((size_t)sh.nentries, s), ICICLE_ALLOCATION_FAILED);
  }
  uint32_t* const w = pl->ws;
  pl->counts = w + sh.ws.counts;
  pl->offsets = w + sh.ws.offsets;
  pl->large_list = w + sh.ws.large_list;
  pl->order = w + sh.ws.order;
  pl->large_first = w + sh.ws.large_first;
  pl->n_large = w + sh.ws.n_large;
  pl->tickets = w + sh.ws.tickets;
  pl->large_items = reinterpret_cast<uint2*>(w + sh.ws.large_items);
  const SortCall c = {sh, pl, d_scalars, mont_sc, s, w + sh.ws.cursor, w + sh.ws.s2tickets, w + sh.ws.bsum, w + sh.ws.part_count, w + sh.ws.part_start, w + sh.ws.part_cursor,
                      w + sh.ws.blockhist, w + sh.ws.obsum};
  if (sh.path == SORT_STAGED) {
    uint32_t* const t = tmp.p ? tmp.p : s2tmp.p;
    return crowded ? enqueue_staged<S2_THREADS_CROWDED>(c, s2ws.p, t) : enqueue_staged<S2_THREADS_WIDE>(c, s2ws.p, t);
  }
  if (sh.path == SORT_TWO_LEVEL) enqueue_two_level(c, tmp.p);
  else enqueue_global(c);
  return enqueue_size_order(c);
}

void msm_sort_release(SortPlan* pl)
{
  if (pl->ws) (void)ws_free(pl->ws, pl->stream);
  if (pl->sorted) (void)ws_free(pl->sorted, pl->stream);
  pl->ws = pl->sorted = nullptr;
}
SortPlan::~SortPlan() { msm_sort_release(this); }

// exclusive prefix sum of m 32-bit counters on stream s (the three kernels above: sums of 2048-counter blocks, their scan by one
// workgroup, the finish): out[i] = Σ_{j<i} in[j].  `bsum`: scratch of ⌈m / 2048⌉ words.  In place (out == in) is fine.  Used by the
// cache build's CSR (prover/csr.hip) as well — no third-party device code on any path of this library.
hipError_t exclusive_scan_u32(const uint32_t* in, uint32_t m, uint32_t* out, uint32_t* bsum, hipStream_t s)
{
  if (!m) return hipSuccess;
  const uint32_t nblocks = (m + SCAN_B - 1) / SCAN_B;
  hipLaunchKernelGGL(msm_scan_sums_kernel, dim3(nblocks), dim3(SCAN_T), 0, s, in, m, bsum);
  hipLaunchKernelGGL(msm_scan_top_kernel, dim3(1), dim3(SCAN_T), 0, s, bsum, nblocks);
  hipLaunchKernelGGL(msm_scan_apply_kernel, dim3(nblocks), dim3(SCAN_T), 0, s, in, m, bsum, out);
  return hipGetLastError();
}
size_t exclusive_scan_u32_scratch_words(uint32_t m) { return (m + SCAN_B - 1) / SCAN_B + 1; }

} // namespace isnark

// Profile of the `back`-th most recent MSM (0 = latest) issued by this process.  The caller must have
// synchronised the MSM's stream.  out_ms = {recode+sort, bucket accumulation kernel, large buckets +
// reduction (+ device tail), total, digit sort alone (0 when this MSM did not issue one: several base sets share one
// sort — the prover records it with the G2 MSM for the witness and with the H MSM)}; geom = {L, nbuckets, c, W, is_g2}.
ISNARK_API eIcicleError icicle_snark_msm_profile(int back, float out_ms[5], uint32_t geom[5])
{
  using namespace isnark;
  std::lock_guard<std::mutex> lk(g_msm_prof_mu);
  const MsmProfileRing& r = msm_ring_of_active_device();
  if (!out_ms || !geom || back < 0 || back >= MSM_PROFILE_RING || (uint64_t)back >= r.seq) return ICICLE_INVALID_ARGUMENT;
  const MsmProfile& p = r.slots[(r.seq - 1 - back) % MSM_PROFILE_RING];
  if (!p.valid) return ICICLE_INVALID_ARGUMENT;
  geom[0] = p.L; geom[1] = p.nbuckets; geom[2] = (uint32_t)p.c; geom[3] = (uint32_t)p.W; geom[4] = (uint32_t)p.is_g2;
  if (p.resolved) {
    memcpy(out_ms, p.ms, sizeof p.ms);
    return ICICLE_SUCCESS;
  }
  if (hipEventElapsedTime(&out_ms[0], p.ev[0], p.ev[1]) != hipSuccess) return ICICLE_UNKNOWN_ERROR;
  (void)hipEventElapsedTime(&out_ms[1], p.ev[1], p.ev[2]);
  (void)hipEventElapsedTime(&out_ms[2], p.ev[2], p.ev[3]);
  (void)hipEventElapsedTime(&out_ms[3], p.ev[0], p.ev[3]);
  out_ms[4] = 0;
  if (p.has_sort_end) (void)hipEventElapsedTime(&out_ms[4], p.ev[0], p.ev[4]);
  geom[0] = p.L; geom[1] = p.nbuckets; geom[2] = (uint32_t)p.c; geom[3] = (uint32_t)p.W; geom[4] = (uint32_t)p.is_g2;
  return ICICLE_SUCCESS;
}

// first launch of a translation unit's code object loads it onto the device (milliseconds): prewarm_modules (runtime.cpp) does that ahead
// of the first prove of a process
namespace isnark {
__global__ void module_warm_sort_kernel() {}
void module_warm_sort(hipStream_t s) { hipLaunchKernelGGL(module_warm_sort_kernel, dim3(1), dim3(1), 0, s); }
} // namespace isnark
