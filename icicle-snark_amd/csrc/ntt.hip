// ntt.hip — NTT / iNTT over the BN254 scalar field for gfx950.
//
// Replaces icicle/backend/cuda/include/ntt/ntt.cuh (Domain :441-562, dispatch :661-758) and
// icicle/backend/cuda/src/ntt/mixed_radix_ntt.cu behind bn254_ntt / bn254_ntt_init_domain /
// bn254_ntt_release_domain / bn254_get_root_of_unity.
//
// Design (MI355X-first, not the reference's 64-thread register-tiled radix-16/32/64 plan):
//  * a transform of size n = R1·R2[·R3] is 1–3 passes of a Cooley–Tukey decimation; each pass is a
//    batch of size-R sub-transforms done entirely in LDS.  A workgroup owns a tile of R rows × C
//    columns (R·C = 2048 elements = 64 KiB of the CU's 160 KiB LDS, two workgroups per CU), the
//    C columns being C consecutive elements in memory, so global traffic is runs of C·32 B.
//  * inside the tile: DIF rounds of radix 8 over the rows (eight operands per thread in registers,
//    three radix-2 stages per LDS round trip and per __syncthreads); the tile is kept as two uint4
//    planes (limbs 0-3 / 4-7) so that consecutive lanes read consecutive 16-B LDS slots (no bank
//    conflicts for ds_read_b128 / ds_write_b128).
//  * the inter-pass twiddle ω_n^(k·t), the final 1/n of the inverse transform and the
//    natural-order permutation are fused into the pass that produces the data — there is no
//    separate digit-reverse or normalise pass (the reference runs both:
//    mixed_radix_ntt.cu:61-126).
//  * data stay in STANDARD form; twiddles are stored in Montgomery form, so one Montgomery
//    multiply yields the standard-form product directly.
//  * per element each pass reads 32 B and writes 32 B: 64·P bytes of HBM traffic per element
//    (P = number of passes), the twiddle table (N·32 B) is L2/Infinity-Cache resident.
//  * transforms of 2^11 elements and more whose passes can all work on full tiles run the same plan on a LAZY
//    RADIX-2^29 field (fr29.h, ntt_pass29_kernel below): nine-word tiles, no reduction after additions, value
//    bounds planned on the host — ≈ 20 % faster; the 8×32-bit kernels keep the small and ragged sizes.
// The host plan — pass split, tile geometry, bounds, LDS, grids — is ntt_plan (ntt_plan.h, walked on the host by
// tests/ntt_plan_check.cpp); ntt_impl below stages the operands, asks for the plan and enqueues it (enqueue_passes).
#include <atomic>
#include <mutex>
#include <string.h>
#include <vector>

#include "common.h"
#include "ff.h"
#include "fr29.h"
#include "ntt_fuse.h"
#include "ntt_plan.h"

using namespace bn254;
using namespace isnark;
using namespace isnark::ntt;

namespace {

constexpr int OMEGAS_COUNT = 28;

// fp_config::rou — primitive 2^28-th root of unity, standard form
// (icicle/include/icicle/fields/snark_fields/bn254_scalar.h:68-69)
const uint32_t ROU28[8] = {0x725b19f0, 0x9bd61b6e, 0x41112ed4, 0x402d111e, 0x8ef62abc, 0x00e0a7eb, 0xa58a7e85, 0x2a3c09f0};

struct Domain {
  fe* tw = nullptr; // tw[i] = root^i, Montgomery form, i in [0, N)
  fe* tw29 = nullptr; // the same roots as root^i·2^261 (packed canonical): twiddles of the radix-2^29 passes (fr29.h)
  int log_n = -1;
  fe root_std;
  int device = -1;
};
// one domain per device (the reference's CUDA backend keeps `domains_for_devices`, ntt.cuh:441-450); every entry point
// below works on the domain of the calling thread's active device
constexpr int MAX_DEVICES = 32;
std::mutex g_dom_mu;
Domain g_doms[MAX_DEVICES];
Domain& cur_dom() // caller holds g_dom_mu
{
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= MAX_DEVICES) d = 0;
  return g_doms[d];
}
#define g_dom cur_dom()

fe host_omega(int logn) // Fr::omega — modular_arithmetic.h:61-73 ; standard form in/out
{
  fe w;
  memcpy(w.l, ROU28, 32);
  w = Fr::to_mont(w);
  for (int i = 0; i < OMEGAS_COUNT - logn; i++) w = Fr::sqr(w);
  return Fr::from_mont(w);
}

__global__ void gen_twiddles_kernel(fe* tw, const fe* pw /* root^(2^j), Montgomery */, int log_n)
{
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (1u << log_n)) return;
  fe acc = Fr::one_mont();
  for (int j = 0; j < log_n; j++)
    if ((i >> j) & 1) acc = Fr::mul(acc, pw[j]);
  tw[i] = acc;
}

__device__ __forceinline__ uint32_t tw_index(uint32_t e, uint32_t n_mask, int inverse)
{
  // ω^-e = ω^(N-e)
  return inverse ? ((n_mask + 1 - e) & n_mask) : e;
}

__device__ __forceinline__ fe lds_get(const uint4* lo, const uint4* hi, int idx)
{
  uint4 a = lo[idx], b = hi[idx];
  fe r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  return r;
}
__device__ __forceinline__ void lds_put(uint4* lo, uint4* hi, int idx, const fe& v)
{
  lo[idx] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  hi[idx] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
__device__ __forceinline__ fe g_get(const fe* p)
{
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4 a = q[0], b = q[1];
  fe r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  return r;
}
__device__ __forceinline__ void g_put(fe* p, const fe& v)
{
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

// radix-2^Q decimation-in-frequency butterfly on 2^Q elements held in registers.  Element k sits at row
// base + k·(M >> Q) of a size-M sub-transform whose first row is a multiple of M; j = base mod (M >> Q).
// Twiddles ω_R^e come from the LDS table (e < R/2): ω_Ms^x = ω_R^(x·R/Ms).  Written out stage by stage so
// that every register index is a compile-time constant (a looped form was left rolled by the compiler and
// spilled the operands to scratch).
#define NTT_BF(a, b, e)                                                                                        \
  {                                                                                                            \
    const fe s_ = Fr::add(x[a], x[b]);                                                                         \
    const fe d_ = Fr::sub(x[a], x[b]);                                                                         \
    x[a] = s_;                                                                                                 \
    x[b] = Fr::mul(d_, lds_get(twlo, twhi, (e)));                                                              \
  }
template <int Q>
__device__ __forceinline__ void dif_butterfly(fe (&x)[1 << Q], int j, int log_m, int log_r, const uint4* twlo, const uint4* twhi);

template <>
__device__ __forceinline__ void dif_butterfly<3>(fe (&x)[8], int j, int log_m, int log_r, const uint4* twlo, const uint4* twhi)
{
  const int g = 1 << (log_m - 3);
  const int s0 = log_r - log_m, s1 = s0 + 1, s2 = s0 + 2;
  NTT_BF(0, 4, j << s0) NTT_BF(1, 5, (j + g) << s0) NTT_BF(2, 6, (j + 2 * g) << s0) NTT_BF(3, 7, (j + 3 * g) << s0)
  NTT_BF(0, 2, j << s1) NTT_BF(1, 3, (j + g) << s1) NTT_BF(4, 6, j << s1) NTT_BF(5, 7, (j + g) << s1)
  NTT_BF(0, 1, j << s2) NTT_BF(2, 3, j << s2) NTT_BF(4, 5, j << s2) NTT_BF(6, 7, j << s2)
}
template <>
__device__ __forceinline__ void dif_butterfly<2>(fe (&x)[4], int j, int log_m, int log_r, const uint4* twlo, const uint4* twhi)
{
  const int g = 1 << (log_m - 2);
  const int s0 = log_r - log_m, s1 = s0 + 1;
  NTT_BF(0, 2, j << s0) NTT_BF(1, 3, (j + g) << s0)
  NTT_BF(0, 1, j << s1) NTT_BF(2, 3, j << s1)
}
template <>
__device__ __forceinline__ void dif_butterfly<1>(fe (&x)[2], int j, int log_m, int log_r, const uint4* twlo, const uint4* twhi)
{
  NTT_BF(0, 1, j << (log_r - log_m))
}
// Last round of a sub-transform (log_m == Q: j = 0, g = 1): 7 of the 12 twiddles of a radix-8 group are ω^0 = 1 (3 of 4 for
// radix 4) — those products are skipped; the data are in standard form, so "times Montgomery one" is the identity.
#define NTT_BF1(a, b)                                                                                          \
  {                                                                                                            \
    const fe s_ = Fr::add(x[a], x[b]);                                                                         \
    x[b] = Fr::sub(x[a], x[b]);                                                                                \
    x[a] = s_;                                                                                                 \
  }
template <int Q>
__device__ __forceinline__ void dif_butterfly_last(fe (&x)[1 << Q], int log_r, const uint4* twlo, const uint4* twhi);
template <>
__device__ __forceinline__ void dif_butterfly_last<3>(fe (&x)[8], int log_r, const uint4* twlo, const uint4* twhi)
{
  const int s0 = log_r - 3, s1 = s0 + 1;
  NTT_BF1(0, 4) NTT_BF(1, 5, 1 << s0) NTT_BF(2, 6, 2 << s0) NTT_BF(3, 7, 3 << s0)
  NTT_BF1(0, 2) NTT_BF(1, 3, 1 << s1) NTT_BF1(4, 6) NTT_BF(5, 7, 1 << s1)
  NTT_BF1(0, 1) NTT_BF1(2, 3) NTT_BF1(4, 5) NTT_BF1(6, 7)
}
template <>
__device__ __forceinline__ void dif_butterfly_last<2>(fe (&x)[4], int log_r, const uint4* twlo, const uint4* twhi)
{
  const int s0 = log_r - 2;
  NTT_BF1(0, 2) NTT_BF(1, 3, 1 << s0)
  NTT_BF1(0, 1) NTT_BF1(2, 3)
}
template <>
__device__ __forceinline__ void dif_butterfly_last<1>(fe (&x)[2], int log_r, const uint4* twlo, const uint4* twhi)
{
  NTT_BF1(0, 1)
}
#undef NTT_BF1
#undef NTT_BF

// one round of radix-2^Q butterflies over the whole tile: 8 >> Q groups per thread
template <int Q, bool LAST = false>
__device__ __forceinline__ void dif_round(uint4* lo, uint4* hi, const uint4* twlo, const uint4* twhi, int log_m, int log_r, int log_c, int tid)
{
  const int C = 1 << log_c;
  const int log_g = log_m - Q; // groups per sub-transform = M >> Q
#pragma unroll
  for (int u = 0; u < (8 >> Q); u++) {
    const int gi = tid * (8 >> Q) + u;
    const int c = gi & (C - 1);
    const int rest = gi >> log_c;
    const int j = rest & ((1 << log_g) - 1);
    const int blk = rest >> log_g;
    const int base_row = (blk << log_m) + j;
    fe x[1 << Q];
#pragma unroll
    for (int k = 0; k < (1 << Q); k++) x[k] = lds_get(lo, hi, ((base_row + (k << log_g)) << log_c) + c);
    if (LAST) dif_butterfly_last<Q>(x, log_r, twlo, twhi); // log_m == Q
    else dif_butterfly<Q>(x, j, log_m, log_r, twlo, twhi);
#pragma unroll
    for (int k = 0; k < (1 << Q); k++) lds_put(lo, hi, ((base_row + (k << log_g)) << log_c) + c, x[k]);
  }
}

// One pass: grid = (tiles, batch); the tile always holds 2048 elements = 8 per thread (smaller transforms
// are padded by idle threads).  LDS: two uint4 planes of R·C entries + R/2 stage twiddles.
// The size-R sub-transforms run as ⌈log R / 3⌉ rounds of radix-8 (then one radix-4 / radix-2 round) with the
// eight operands of a butterfly in registers — one LDS round trip and one barrier per THREE radix-2 stages; the last
// round of a sub-transform skips its unit twiddles (7 of 12 products).
// FUSE (prover, last pass of the forward transform, grid.y = 1, full tiles): the workgroup transforms its tile of the
// three rows [B | A | C'] one after the other, keeps B's then A·B's eight outputs per thread in registers and writes
// A·B − C' — the pointwise epilogue of construct_r1cs (src/proof_helper.rs:154-167) — to row 0 of `out`: one n-element
// store instead of 3n, and no separate read-modify-write sweep.
// one row's tile: load → rounds → store.  MODE 0: plain store (inter-pass twiddle / scale); MODE 1, 2, 3: rows B, A, C' of the
// fused epilogue (see the kernel).  Instantiated once per mode so that nothing is live across the rows.
template <int MODE>
__device__ __forceinline__ void ntt_tile_row(const fe* __restrict__ src, fe* __restrict__ dst, const fe* __restrict__ tw, const PassParams& p, const fe& ninv_mont, uint4* lo, uint4* hi,
                                             const uint4* twlo, const uint4* twhi, uint32_t b_lo, uint64_t out_off, int tid)
{
  const int R = 1 << p.log_r, C = 1 << p.log_c, RC = R * C;
  // load tile: LDS index = r·C + c.  All of a thread's loads are issued before the first LDS store.
  if (RC == NT * 8) {
    fe v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int e = tid + u * NT;
      int r, c;
      if (p.load_rows_fastest) { r = e & (R - 1); c = e >> p.log_r; }
      else { c = e & (C - 1); r = e >> p.log_c; }
      v[u] = g_get(src + (uint64_t)r * p.in_row + (uint64_t)c * p.in_col);
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int e = tid + u * NT;
      int r, c;
      if (p.load_rows_fastest) { r = e & (R - 1); c = e >> p.log_r; }
      else { c = e & (C - 1); r = e >> p.log_c; }
      lds_put(lo, hi, (r << p.log_c) + c, v[u]);
    }
  } else {
    for (int e = tid; e < RC; e += NT) {
      int r, c;
      if (p.load_rows_fastest) { r = e & (R - 1); c = e >> p.log_r; }
      else { c = e & (C - 1); r = e >> p.log_c; }
      lds_put(lo, hi, (r << p.log_c) + c, g_get(src + (uint64_t)r * p.in_row + (uint64_t)c * p.in_col));
    }
  }
  __syncthreads();

  if (RC == NT * 8) {
    // natural order in → bit-reversed order out, three radix-2 stages per round
    int log_m = p.log_r;
    while (log_m > 3) {
      dif_round<3>(lo, hi, twlo, twhi, log_m, p.log_r, p.log_c, tid);
      __syncthreads();
      log_m -= 3;
    }
    if (log_m == 3) dif_round<3, true>(lo, hi, twlo, twhi, log_m, p.log_r, p.log_c, tid);
    else if (log_m == 2) dif_round<2, true>(lo, hi, twlo, twhi, log_m, p.log_r, p.log_c, tid);
    else if (log_m == 1) dif_round<1, true>(lo, hi, twlo, twhi, log_m, p.log_r, p.log_c, tid);
    __syncthreads();
  } else {
    // small transforms (tile smaller than 2048 elements): plain radix-2 stages
    const int nbf = RC >> 1;
    for (int s = p.log_r - 1; s >= 0; s--) {
      const int h = 1 << s;
      for (int q = tid; q < nbf; q += NT) {
        const int c = q & (C - 1);
        const int bf = q >> p.log_c;
        const int j = bf & (h - 1);
        const int i = ((bf >> s) << (s + 1)) + j;
        const int ia = (i << p.log_c) + c, ib = ((i + h) << p.log_c) + c;
        fe a = lds_get(lo, hi, ia), bb = lds_get(lo, hi, ib);
        fe sum = Fr::add(a, bb);
        fe dif = Fr::sub(a, bb);
        const int e = j << (p.log_r - 1 - s);
        if (e != 0) dif = Fr::mul(dif, lds_get(twlo, twhi, e));
        lds_put(lo, hi, ia, sum);
        lds_put(lo, hi, ib, dif);
      }
      __syncthreads();
    }
  }

  if (MODE != 0) {
    // full tile, last pass (no inter-pass twiddle, no scaling).  The running value (B̂, then Â·B̂) lives in the output
    // buffer itself: every thread re-reads exactly the addresses it wrote for the previous row (its own stores, program
    // order; the 64 KiB a workgroup touches stay in L2), so nothing is held in registers across a row's transform —
    // eight kept elements per thread (64 VGPRs) pushed the rounds into scratch.
    // four elements at a time (like the plain store): four L2 reads in flight without pushing the kernel past its registers
#pragma unroll 1
    for (int u0 = 0; u0 < 8; u0 += 4) {
      fe y[4];
      fe* q[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int e = tid + (u0 + u) * NT;
        const int c = e & (C - 1);
        const uint32_t kk = __brev((uint32_t)(e >> p.log_c)) >> (32 - p.log_r);
        q[u] = dst + (uint64_t)kk * p.out_row + (uint64_t)c * p.out_col;
        if (MODE != 1) y[u] = g_get(q[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const fe x = lds_get(lo, hi, tid + (u0 + u) * NT);
        if (MODE == 1) g_put(q[u], x);
        else if (MODE == 2) g_put(q[u], Fr::mul(Fr::mul(x, y[u]), Fr::r2())); // standard-form product
        else g_put(q[u], Fr::sub(y[u], x));
      }
    }
    return;
  }
  // store: LDS row s holds k = bitrev(s); inter-pass twiddle and 1/n (or the caller's per-element scale) fused here
  for (int e0 = tid; e0 < RC; e0 += NT * 4) {
    fe w[4];
    uint32_t kk[4], ex[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int e = e0 + u * NT;
      ex[u] = 0;
      if (e < RC) {
        const int c = e & (C - 1);
        kk[u] = __brev((uint32_t)(e >> p.log_c)) >> (32 - p.log_r);
        if (p.tw_mul) ex[u] = kk[u] * ((b_lo << p.log_c) + c) * p.tw_mul;
        if (ex[u]) w[u] = g_get(tw + tw_index(ex[u], p.n_mask, p.inverse));
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int e = e0 + u * NT;
      if (e < RC) {
        const int c = e & (C - 1);
        fe x = lds_get(lo, hi, e);
        if (ex[u]) x = Fr::mul(x, w[u]);
        if (p.scale_tab) x = Fr::mul(x, g_get(p.scale_tab + (out_off + (uint64_t)kk[u] * p.out_row + (uint64_t)c * p.out_col) * p.scale_stride));
        else if (p.scale) x = Fr::mul(x, ninv_mont);
        g_put(dst + (uint64_t)kk[u] * p.out_row + (uint64_t)c * p.out_col, x);
      }
    }
  }
}

template <bool FUSE>
__global__ __launch_bounds__(NT, 2) void ntt_pass_kernel(const fe* __restrict__ in, fe* __restrict__ out, const fe* __restrict__ tw, PassParams p, fe ninv_mont)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int R = 1 << p.log_r, C = 1 << p.log_c, RC = R * C;
  uint4* lo = reinterpret_cast<uint4*>(smem);
  uint4* hi = lo + RC;
  uint4* twlo = hi + RC; // R/2 entries
  uint4* twhi = twlo + (R >> 1);

  const uint32_t b = blockIdx.x;
  const uint32_t b_hi = b >> p.tiles_per_group_log, b_lo = b & ((1u << p.tiles_per_group_log) - 1);
  const uint64_t in_off = b_hi * p.in_hi + b_lo * p.in_lo, out_off = b_hi * p.out_hi + b_lo * p.out_lo;
  const int tid = threadIdx.x;

  // stage twiddles ω_R^e, e < R/2
  for (int e = tid; e < (R >> 1); e += NT) {
    fe w = g_get(tw + tw_index((uint32_t)e * p.stage_stride, p.n_mask, p.inverse));
    lds_put(twlo, twhi, e, w);
  }
  if (!FUSE) {
    ntt_tile_row<0>(in + (uint64_t)blockIdx.y * p.batch_stride + in_off, out + (uint64_t)blockIdx.y * p.batch_stride + out_off, tw, p, ninv_mont, lo, hi, twlo, twhi, b_lo, out_off, tid);
  } else {
    ntt_tile_row<1>(in + in_off, out + out_off, tw, p, ninv_mont, lo, hi, twlo, twhi, b_lo, out_off, tid);
    __syncthreads(); // the row's outputs have been read out of the tile
    ntt_tile_row<2>(in + p.batch_stride + in_off, out + out_off, tw, p, ninv_mont, lo, hi, twlo, twhi, b_lo, out_off, tid);
    __syncthreads();
    ntt_tile_row<3>(in + 2 * p.batch_stride + in_off, out + out_off, tw, p, ninv_mont, lo, hi, twlo, twhi, b_lo, out_off, tid);
  }
}

// ---- the same pass on the lazy radix-2^29 field (fr29.h) --------------------------------------------------------------------------
// Full 2048-element tiles only, at most 8 bits per pass.  Differences from ntt_pass_kernel:
//  * the tile holds NINE words per element — two uint4 planes + one word plane (72 KiB) — and the stage twiddles stay packed
//    (32 B, Montgomery-261, unpacked at use), so two workgroups still share a CU's LDS;
//  * a butterfly is  s = norm(a + b),  d = (a + K·r − b)·w :  nine-instruction add / sub, a 27-instruction carry pass, and a
//    product of 153 multiply-adds (the 8×32-bit form: ≈ 40 + 40 + 300).  Values are NOT reduced after additions: the bound of
//    level l's inputs (in multiples of r) is tracked on the host (Plan29), which hands the kernel the borrow-proof constant
//    K_l·r of every level and says whether the tile needs one `shrink` before its last round;
//  * everything that leaves a pass has gone through a product (inter-pass twiddle, 1/n, per-element scale) and is < 4·r, which
//    fits the packed 32-byte form; the LAST pass of a transform stores canonical values.
struct Lds29 {
  uint4 *lo, *hi;
  uint32_t* top;
};
__device__ __forceinline__ fe9 lds_get9(const Lds29& t, int idx)
{
  const uint4 a = t.lo[idx], b = t.hi[idx];
  fe9 r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  r.l[8] = t.top[idx];
  return r;
}
__device__ __forceinline__ void lds_put9(const Lds29& t, int idx, const fe9& v)
{
  t.lo[idx] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  t.hi[idx] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
  t.top[idx] = v.l[8];
}
// a + K·r − b with a wave-uniform K (the constant is computed in scalar registers); b's limbs ≤ J·(2^29 − 1), b < K − 1
__device__ __forceinline__ fe9 sub_k(const fe9& a, const fe9& b, const fr29::Limbs9& kc)
{
  fe9 o;
#pragma unroll
  for (int i = 0; i < 9; i++) o.l[i] = a.l[i] + (kc.v[i] - b.l[i]);
  return o;
}
// One level of a round.  NORM: the sums leave normalised (a level's sums may stay un-normalised — limbs < 2^30 — when the next
// level of the same round subtracts them against a J = 2 constant).  Differences with a unit twiddle (_1) are always normalised.
#define NTT_BF9(a, b, e, NORM)                                                                                 \
  {                                                                                                            \
    const fe9 s_ = NORM ? fr29::norm(fr29::add(x[a], x[b])) : fr29::add(x[a], x[b]);                           \
    const fe9 d_ = sub_k(x[a], x[b], kc);                                                                      \
    x[a] = s_;                                                                                                 \
    x[b] = fr29::mul(d_, lds_get9(tw, (e)));                                                                   \
  }
#define NTT_BF9_1(a, b, NORM)                                                                                  \
  {                                                                                                            \
    const fe9 s_ = NORM ? fr29::norm(fr29::add(x[a], x[b])) : fr29::add(x[a], x[b]);                           \
    x[b] = fr29::norm(sub_k(x[a], x[b], kc));                                                                  \
    x[a] = s_;                                                                                                 \
  }
// K of level l (inputs below B: K = B + 1)
__device__ __forceinline__ uint32_t k_mid(const Plan29& pl, int l) { return (pl.b0 << l) + 1u; }
__device__ __forceinline__ uint32_t k_last(const Plan29& pl, int t) { return (pl.bs + 1u) << t; }

__device__ __forceinline__ void dif_butterfly9_mid(fe9 (&x)[8], int j, int log_m, int log_r, const Lds29& tw, const Plan29& pl)
{
  const int g = 1 << (log_m - 3);
  const int s0 = log_r - log_m, s1 = s0 + 1, s2 = s0 + 2;
  {
    const fr29::Limbs9 kc = fr29::kr_borrow_proof(k_mid(pl, s0), 1);
    NTT_BF9(0, 4, j << s0, false) NTT_BF9(1, 5, (j + g) << s0, false) NTT_BF9(2, 6, (j + 2 * g) << s0, false) NTT_BF9(3, 7, (j + 3 * g) << s0, false)
  }
  {
    const fr29::Limbs9 kc = fr29::kr_borrow_proof(k_mid(pl, s1), 2);
    NTT_BF9(0, 2, j << s1, true) NTT_BF9(1, 3, (j + g) << s1, true) NTT_BF9(4, 6, j << s1, true) NTT_BF9(5, 7, (j + g) << s1, true)
  }
  {
    const fr29::Limbs9 kc = fr29::kr_borrow_proof(k_mid(pl, s2), 1);
    NTT_BF9(0, 1, j << s2, true) NTT_BF9(2, 3, j << s2, true) NTT_BF9(4, 5, j << s2, true) NTT_BF9(6, 7, j << s2, true)
  }
}
template <int Q>
__device__ __forceinline__ void dif_butterfly9_last(fe9 (&x)[1 << Q], int log_r, const Lds29& tw, const Plan29& pl);
template <>
__device__ __forceinline__ void dif_butterfly9_last<3>(fe9 (&x)[8], int log_r, const Lds29& tw, const Plan29& pl)
{
  const int s0 = log_r - 3, s1 = s0 + 1;
  {
    const fr29::Limbs9 kc = fr29::kr_borrow_proof(k_last(pl, 0), 1);
    NTT_BF9_1(0, 4, false) NTT_BF9(1, 5, 1 << s0, false) NTT_BF9(2, 6, 2 << s0, false) NTT_BF9(3, 7, 3 << s0, false)
  }
  {
    const fr29::Limbs9 kc = fr29::kr_borrow_proof(k_last(pl, 1), 2);
    NTT_BF9_1(0, 2, true) NTT_BF9(1, 3, 1 << s1, true) NTT_BF9_1(4, 6, true) NTT_BF9(5, 7, 1 << s1, true)
  }
  {
    const fr29::Limbs9 kc = fr29::kr_borrow_proof(k_last(pl, 2), 1);
    NTT_BF9_1(0, 1, true) NTT_BF9_1(2, 3, true) NTT_BF9_1(4, 5, true) NTT_BF9_1(6, 7, true)
  }
}
template <>
__device__ __forceinline__ void dif_butterfly9_last<2>(fe9 (&x)[4], int log_r, const Lds29& tw, const Plan29& pl)
{
  const int s0 = log_r - 2;
  {
    const fr29::Limbs9 kc = fr29::kr_borrow_proof(k_last(pl, 0), 1);
    NTT_BF9_1(0, 2, false) NTT_BF9(1, 3, 1 << s0, false)
  }
  {
    const fr29::Limbs9 kc = fr29::kr_borrow_proof(k_last(pl, 1), 2);
    NTT_BF9_1(0, 1, true) NTT_BF9_1(2, 3, true)
  }
}
template <>
__device__ __forceinline__ void dif_butterfly9_last<1>(fe9 (&x)[2], int log_r, const Lds29& tw, const Plan29& pl)
{
  const fr29::Limbs9 kc = fr29::kr_borrow_proof(k_last(pl, 0), 1);
  NTT_BF9_1(0, 1, true)
}
#undef NTT_BF9_1
#undef NTT_BF9

template <int Q, bool LAST>
__device__ __forceinline__ void dif_round9(const Lds29& t, const Lds29& tw, int log_m, int log_r, int log_c, int tid, const Plan29& pl)
{
  const int C = 1 << log_c;
  const int log_g = log_m - Q;
#pragma unroll
  for (int u = 0; u < (8 >> Q); u++) {
    const int gi = tid * (8 >> Q) + u;
    const int c = gi & (C - 1);
    const int rest = gi >> log_c;
    const int j = rest & ((1 << log_g) - 1);
    const int blk = rest >> log_g;
    const int base_row = (blk << log_m) + j;
    fe9 x[1 << Q];
#pragma unroll
    for (int k = 0; k < (1 << Q); k++) x[k] = lds_get9(t, ((base_row + (k << log_g)) << log_c) + c);
    if constexpr (LAST) {
      if (pl.shrink_last) {
#pragma unroll
        for (int k = 0; k < (1 << Q); k++) x[k] = fr29::shrink(x[k]);
      }
      dif_butterfly9_last<Q>(x, log_r, tw, pl);
    } else dif_butterfly9_mid(x, j, log_m, log_r, tw, pl);
#pragma unroll
    for (int k = 0; k < (1 << Q); k++) lds_put9(t, ((base_row + (k << log_g)) << log_c) + c, x[k]);
  }
}

// x·2^5 of an N value below 4 (→ N, below 128): the factor a Montgomery-256 operand leaves behind in a 2^261 product
__device__ __forceinline__ fe9 shl5(const fe9& a)
{
  fe9 o;
  o.l[0] = (a.l[0] & 0xffffffu) << 5;
#pragma unroll
  for (int i = 1; i < 8; i++) o.l[i] = ((a.l[i] & 0xffffffu) << 5) | (a.l[i - 1] >> 24);
  o.l[8] = (a.l[8] << 5) | (a.l[7] >> 24);
  return o;
}

// MODE as in ntt_tile_row
template <int MODE>
__device__ __forceinline__ void ntt_tile_row9(const fe* __restrict__ src, fe* __restrict__ dst, const fe* __restrict__ tw29, const PassParams& p, const Plan29& pl, const fe& ninv261, const Lds29& t,
                                              const Lds29& tw, uint32_t b_lo, uint64_t out_off, int tid)
{
  const int R = 1 << p.log_r, C = 1 << p.log_c;
  {
    fe v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int e = tid + u * NT;
      int r, c;
      if (p.load_rows_fastest) { r = e & (R - 1); c = e >> p.log_r; }
      else { c = e & (C - 1); r = e >> p.log_c; }
      v[u] = g_get(src + (uint64_t)r * p.in_row + (uint64_t)c * p.in_col);
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int e = tid + u * NT;
      int r, c;
      if (p.load_rows_fastest) { r = e & (R - 1); c = e >> p.log_r; }
      else { c = e & (C - 1); r = e >> p.log_c; }
      lds_put9(t, (r << p.log_c) + c, fr29::unpack(v[u]));
    }
  }
  __syncthreads();
  {
    int log_m = p.log_r;
    while (log_m > 3) {
      dif_round9<3, false>(t, tw, log_m, p.log_r, p.log_c, tid, pl);
      __syncthreads();
      log_m -= 3;
    }
    if (log_m == 3) dif_round9<3, true>(t, tw, log_m, p.log_r, p.log_c, tid, pl);
    else if (log_m == 2) dif_round9<2, true>(t, tw, log_m, p.log_r, p.log_c, tid, pl);
    else dif_round9<1, true>(t, tw, log_m, p.log_r, p.log_c, tid, pl);
    __syncthreads();
  }
  if (MODE != 0) {
    // fused epilogue (see ntt_tile_row): B̂ canonical → dst;  Â·B̂ (standard form, < 2·r) → dst;  Â·B̂ − Ĉ' canonical → dst
#pragma unroll 1
    for (int u0 = 0; u0 < 8; u0 += 4) {
      fe y[4];
      fe* q[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int e = tid + (u0 + u) * NT;
        const int c = e & (C - 1);
        const uint32_t kk = __brev((uint32_t)(e >> p.log_c)) >> (32 - p.log_r);
        q[u] = dst + (uint64_t)kk * p.out_row + (uint64_t)c * p.out_col;
        if (MODE != 1) y[u] = g_get(q[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const fe9 x = lds_get9(t, tid + (u0 + u) * NT);
        if (MODE == 1) g_put(q[u], fr29::pack(fr29::canon(x)));
        else if (MODE == 2) g_put(q[u], fr29::pack(fr29::mul(fr29::mul(x, fr29::unpack(y[u])), fr29::r2())));
        else g_put(q[u], fr29::pack(fr29::canon(fr29::norm(fr29::sub<600>(fr29::unpack(y[u]), x)))));
      }
    }
    return;
  }
  for (int e0 = tid; e0 < NT * 8; e0 += NT * 4) {
    fe w[4];
    uint32_t kk[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int e = e0 + u * NT;
      const int c = e & (C - 1);
      kk[u] = __brev((uint32_t)(e >> p.log_c)) >> (32 - p.log_r);
      if (p.tw_mul) w[u] = g_get(tw29 + tw_index(kk[u] * ((b_lo << p.log_c) + c) * p.tw_mul, p.n_mask, p.inverse)); // (index 0: the Montgomery one)
      else if (p.scale_tab) w[u] = g_get(p.scale_tab + (out_off + (uint64_t)kk[u] * p.out_row + (uint64_t)c * p.out_col) * p.scale_stride);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int e = e0 + u * NT;
      const int c = e & (C - 1);
      fe9 x = lds_get9(t, e);
      if (p.tw_mul) x = fr29::mul(x, fr29::unpack(w[u]));                               // < 4 (fits 32 bytes); not the last pass
      else if (p.scale_tab) x = fr29::canon(shl5(fr29::mul(x, fr29::unpack(w[u]))));     // the caller's table is Montgomery-256: ·2^5 afterwards
      else if (p.scale) x = fr29::canon4(fr29::mul(x, fr29::unpack(ninv261)));
      else x = fr29::canon(x);
      g_put(dst + (uint64_t)kk[u] * p.out_row + (uint64_t)c * p.out_col, fr29::pack(x));
    }
  }
}

template <bool FUSE>
__global__ __launch_bounds__(NT, 2) void ntt_pass29_kernel(const fe* __restrict__ in, fe* __restrict__ out, const fe* __restrict__ tw29, PassParams p, Plan29 pl, fe ninv261)
{
  ISNARK_CRITICAL_CHAIN_KERNEL();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int R = 1 << p.log_r, RC = NT * 8;
  // tile: two uint4 planes + one word plane of 2048 entries; stage twiddles ω_R^e (e < R/2, Montgomery-261) in the same form
  Lds29 t, tw;
  t.lo = reinterpret_cast<uint4*>(smem);
  t.hi = t.lo + RC;
  tw.lo = t.hi + RC;
  tw.hi = tw.lo + (R >> 1);
  t.top = reinterpret_cast<uint32_t*>(tw.hi + (R >> 1));
  tw.top = t.top + RC;

  uint32_t b = blockIdx.x, row = blockIdx.y;
  if (!FUSE && p.xcd_batch) {
    const uint32_t w = b >> 3;
    row = w % p.xcd_batch;
    b = (w / p.xcd_batch) * 8 + (b & 7);
  }
  const uint32_t b_hi = b >> p.tiles_per_group_log, b_lo = b & ((1u << p.tiles_per_group_log) - 1);
  const uint64_t in_off = b_hi * p.in_hi + b_lo * p.in_lo, out_off = b_hi * p.out_hi + b_lo * p.out_lo;
  const int tid = threadIdx.x;
  for (int e = tid; e < (R >> 1); e += NT) lds_put9(tw, e, fr29::unpack(g_get(tw29 + tw_index((uint32_t)e * p.stage_stride, p.n_mask, p.inverse))));
  if (!FUSE) {
    ntt_tile_row9<0>(in + (uint64_t)row * p.batch_stride + in_off, out + (uint64_t)row * p.batch_stride + out_off, tw29, p, pl, ninv261, t, tw, b_lo, out_off, tid);
  } else {
    ntt_tile_row9<1>(in + in_off, out + out_off, tw29, p, pl, ninv261, t, tw, b_lo, out_off, tid);
    __syncthreads();
    ntt_tile_row9<2>(in + p.batch_stride + in_off, out + out_off, tw29, p, pl, ninv261, t, tw, b_lo, out_off, tid);
    __syncthreads();
    ntt_tile_row9<3>(in + 2 * p.batch_stride + in_off, out + out_off, tw29, p, pl, ninv261, t, tw, b_lo, out_off, tid);
  }
}

// tw29[i] = tw[i]·2^5 (Montgomery-256 → Montgomery-261), packed canonical
__global__ __launch_bounds__(256) void twiddles_to_261_kernel(const fe* __restrict__ tw, fe* __restrict__ tw29, uint64_t n)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) g_put(tw29 + i, fr29::pack(fr29::canon4(fr29::mul(fr29::unpack(g_get(tw + i)), fr29::c256_to_261()))));
}

// natural row-major (b·n + i)  ↔  caller layout (bit-reversed index and/or columns_batch).  scatter = 0: out[b·n + i] =
// in[caller(b, i)] ; scatter = 1: out[caller(b, i)] = in[b·n + i]
__global__ __launch_bounds__(256) void relayout_kernel(const fe* __restrict__ in, fe* __restrict__ out, uint64_t n, int batch, int logn, int rev, int cols, int scatter)
{
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * (uint64_t)batch) return;
  const uint64_t b = t / n, i = t % n;
  const uint64_t j = rev ? (logn ? (uint64_t)(__brevll(i) >> (64 - logn)) : 0) : i;
  const uint64_t c = cols ? b + j * (uint64_t)batch : b * n + j;
  if (scatter) g_put(out + c, g_get(in + t));
  else g_put(out + t, g_get(in + c));
}

// coset pre/post multiplication x[j] *= g^(±j) (NTTConfig.coset_gen ≠ 1)
__global__ void coset_mul_kernel(fe* data, uint64_t n, int batch, const fe* gpow2 /* g^(±2^j), Montgomery */, int logn)
{
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe acc = Fr::one_mont();
  for (int j = 0; j < logn; j++)
    if ((i >> j) & 1) acc = Fr::mul(acc, gpow2[j]);
  for (int b = 0; b < batch; b++) {
    fe v = g_get(data + (uint64_t)b * n + i);
    g_put(data + (uint64_t)b * n + i, Fr::mul(v, acc));
  }
}

} // namespace

namespace isnark {
// twiddle table ω_N^i (Montgomery form) of the current domain; nullptr when none (used by the prover
// host for the coset keys)
const fe* ntt_domain_table(int* log_n)
{
  std::lock_guard<std::mutex> lk(g_dom_mu);
  if (log_n) *log_n = g_dom.log_n;
  return g_dom.tw;
}
} // namespace isnark

// ------------------------------------------------------------------------------------------------ API
ISNARK_API eIcicleError bn254_get_root_of_unity(uint64_t max_size, bn254_scalar_t* rou)
{
  // icicle/src/ntt.cpp:52-61
  if (!rou) return ICICLE_INVALID_POINTER;
  const int logn = ilog2(max_size);
  if (logn > OMEGAS_COUNT) {
    set_last_error("no root-of-unity of order 2^%d in the BN254 scalar field", logn);
    return ICICLE_INVALID_ARGUMENT;
  }
  fe w;
  if (logn == 0) w = Fr::one_std();
  else w = host_omega(logn);
  memcpy(rou->limbs, w.l, 32);
  return ICICLE_SUCCESS;
}

ISNARK_API eIcicleError bn254_ntt_init_domain(const bn254_scalar_t* primitive_root, const NTTInitDomainConfig* cfg)
{
  if (!primitive_root || !cfg) return ICICLE_INVALID_POINTER;
  ICICLE_TRY(require_device());
  std::lock_guard<std::mutex> lk(g_dom_mu);
  // the reference silently keeps an existing domain (cuda ntt.cuh:452, cpu_ntt_domain.h:69)
  if (g_dom.tw) return ICICLE_SUCCESS;
  fe root;
  memcpy(root.l, primitive_root->limbs, 32);
  fe rm = Fr::to_mont(root);
  // order of the root: smallest k with root^(2^k) = 1
  std::vector<fe> pw;
  fe cur = rm;
  int k = 0;
  while (!Fr::eq(cur, Fr::one_mont())) {
    pw.push_back(cur);
    cur = Fr::sqr(cur);
    if (++k > OMEGAS_COUNT) {
      set_last_error("ntt_init_domain: not a 2^k-th root of unity (k <= %d)", OMEGAS_COUNT);
      return ICICLE_INVALID_ARGUMENT;
    }
  }
  hipStream_t s = (hipStream_t)cfg->stream;
  const uint64_t N = 1ull << k;
  fe* tw = nullptr;
  fe* dpw = nullptr;
  HIP_TRY(hipMalloc(&tw, N * sizeof(fe)), ICICLE_ALLOCATION_FAILED);
  if (k > 0) {
    HIP_TRY(hipMalloc(&dpw, k * sizeof(fe)), ICICLE_ALLOCATION_FAILED);
    HIP_TRY(hipMemcpy(dpw, pw.data(), k * sizeof(fe), hipMemcpyHostToDevice), ICICLE_COPY_FAILED);
  }
  hipLaunchKernelGGL(gen_twiddles_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, tw, dpw, k);
  ICICLE_TRY(check_launch("gen_twiddles"));
  HIP_TRY(hipStreamSynchronize(s), ICICLE_SYNCHRONIZATION_FAILED); // pw (host vector) and dpw lifetimes
  if (dpw) (void)hipFree(dpw);
  // the same roots in Montgomery-261 form for the radix-2^29 passes (fr29.h); without the memory for it those stay off
  fe* tw29 = nullptr;
  if (hipMalloc(&tw29, N * sizeof(fe)) == hipSuccess) {
    hipLaunchKernelGGL(twiddles_to_261_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, tw, tw29, N);
    ICICLE_TRY(check_launch("twiddles_to_261"));
    HIP_TRY(hipStreamSynchronize(s), ICICLE_SYNCHRONIZATION_FAILED);
  } else {
    (void)hipGetLastError();
    tw29 = nullptr;
  }
  g_dom.tw = tw;
  g_dom.tw29 = tw29;
  g_dom.log_n = k;
  g_dom.root_std = root;
  (void)hipGetDevice(&g_dom.device);
  return ICICLE_SUCCESS;
}

ISNARK_API eIcicleError bn254_ntt_release_domain(void)
{
  std::lock_guard<std::mutex> lk(g_dom_mu);
  if (g_dom.tw) {
    (void)hipDeviceSynchronize();
    (void)hipFree(g_dom.tw);
    if (g_dom.tw29) (void)hipFree(g_dom.tw29);
  }
  Domain& d = g_dom;
  d = Domain();
  return ICICLE_SUCCESS;
}

ISNARK_API eIcicleError bn254_get_root_of_unity_from_domain(uint64_t logn, bn254_scalar_t* rou)
{
  if (!rou) return ICICLE_INVALID_POINTER;
  std::lock_guard<std::mutex> lk(g_dom_mu);
  if (!g_dom.tw || (int)logn > g_dom.log_n) {
    set_last_error("get_root_of_unity_from_domain: domain not initialised or too small");
    return ICICLE_INVALID_ARGUMENT;
  }
  fe w = Fr::to_mont(g_dom.root_std);
  for (int i = 0; i < g_dom.log_n - (int)logn; i++) w = Fr::sqr(w);
  w = Fr::from_mont(w);
  memcpy(rou->limbs, w.l, 32);
  return ICICLE_SUCCESS;
}

namespace {
// the caller's layout: the transform itself runs natural → natural; bit-reversed inputs / outputs and the columns_batch layout
// (element i of batch b at b + i·batch) are handled by one re-layout pass on either side (relayout_kernel)
struct Relayout {
  bool rev_in, rev_out, cols;
  WsScoped<fe> pre, post;
};
// stage 2: `d_in` / `d_out` become what the passes read and write
eIcicleError stage_layout(Relayout& r, const fe*& d_in, fe*& d_out, uint64_t n, int batch, int logn, hipStream_t s)
{
  const uint64_t total = n * batch;
  if (r.rev_in || r.cols) {
    HIP_TRY(r.pre.alloc(total, s), ICICLE_ALLOCATION_FAILED);
    hipLaunchKernelGGL(relayout_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_in, r.pre.p, n, batch, logn, r.rev_in ? 1 : 0, r.cols ? 1 : 0, 0);
    ICICLE_TRY(check_launch("ntt_relayout_in"));
    d_in = r.pre.p;
  }
  if (r.rev_out || r.cols) {
    HIP_TRY(r.post.alloc(total, s), ICICLE_ALLOCATION_FAILED);
    d_out = r.post.p;
  }
  return ICICLE_SUCCESS;
}
// stage 3: coset generator (NTTConfig.coset_gen): forward evaluates on g·H (x_j *= g^j first), inverse interpolates from g·H
// (multiply by g^-j afterwards) — ntt.h:52-64, mixed_radix_ntt.cu:911-1017.  *d_gpow = g^(±2^j), Montgomery; nullptr: g = 1
eIcicleError coset_powers(const NTTConfig* cfg, bool inverse, int logn, fe** d_gpow)
{
  fe g;
  memcpy(g.l, cfg->coset_gen.limbs, 32);
  *d_gpow = nullptr;
  if (Fr::eq(g, Fr::one_std())) return ICICLE_SUCCESS;
  fe gm = Fr::to_mont(g);
  if (inverse) gm = Fr::inv(gm);
  std::vector<fe> gp(logn > 0 ? logn : 1);
  fe cur = gm;
  for (int j = 0; j < logn; j++) { gp[j] = cur; cur = Fr::sqr(cur); }
  HIP_TRY(hipMalloc((void**)d_gpow, gp.size() * sizeof(fe)), ICICLE_ALLOCATION_FAILED);
  HIP_TRY(hipMemcpy(*d_gpow, gp.data(), gp.size() * sizeof(fe), hipMemcpyHostToDevice), ICICLE_COPY_FAILED);
  return ICICLE_SUCCESS;
}
eIcicleError coset_mul(fe* data, uint64_t n, int batch, const fe* d_gpow, int logn, hipStream_t s)
{
  hipLaunchKernelGGL(coset_mul_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, data, n, batch, d_gpow, logn);
  return check_launch("coset_mul");
}

// stage 5: the plan's passes, one launch each, over buf[BUF_IN | BUF_SCRATCH | BUF_OUT]
eIcicleError enqueue_passes(const Plan& plan, const Domain& dom, fe* const buf[3], uint64_t n, const isnark::NttFuse* fuse, hipStream_t s)
{
  static LdsCapOnce cap, cap29; // (the 8×32-bit kernels' cap is raised by every first transform of a device, as it always was)
  const int devi = dom.device >= 0 && dom.device < MAX_DEVICES ? dom.device : 0;
  ICICLE_TRY(cap.raise(devi, 160 * 1024, ntt_pass_kernel<false>, ntt_pass_kernel<true>));
  if (plan.use29) ICICLE_TRY(cap29.raise(devi, 160 * 1024, ntt_pass29_kernel<false>, ntt_pass29_kernel<true>));
  fe ninv = Fr::zero();
  ninv.l[0] = 1;
  if (plan.pass[0].p.inverse) {
    fe nn = Fr::zero();
    nn.l[0] = (uint32_t)n;
    ninv = Fr::inv(Fr::to_mont(nn)); // n^-1 in Montgomery form
  }
  fe c32 = Fr::zero();
  c32.l[0] = 32;
  const fe ninv261 = Fr::mul(ninv, Fr::to_mont(c32)); // n⁻¹·2^256 → n⁻¹·2^261
  for (int pi = 0; pi < plan.np; pi++) {
    const Pass& ps = plan.pass[pi];
    PassParams p = ps.p;
    if (ps.scale_tab) {
      p.scale_tab = fuse->scale_tab;
      p.scale_stride = fuse->scale_stride;
    }
    const fe* src = buf[ps.src];
    fe* dst = ps.fused ? fuse->fused_out : buf[ps.dst];
    const dim3 grid(ps.grid_x, ps.grid_y);
    if (plan.use29 && ps.fused) hipLaunchKernelGGL(ntt_pass29_kernel<true>, grid, dim3(NT), ps.lds, s, src, dst, dom.tw29, p, ps.pl29, ninv261);
    else if (plan.use29) hipLaunchKernelGGL(ntt_pass29_kernel<false>, grid, dim3(NT), ps.lds, s, src, dst, dom.tw29, p, ps.pl29, ninv261);
    else if (ps.fused) hipLaunchKernelGGL(ntt_pass_kernel<true>, grid, dim3(NT), ps.lds, s, src, dst, dom.tw, p, ninv);
    else hipLaunchKernelGGL(ntt_pass_kernel<false>, grid, dim3(NT), ps.lds, s, src, dst, dom.tw, p, ninv);
    ICICLE_TRY(check_launch("ntt_pass"));
  }
  return ICICLE_SUCCESS;
}

eIcicleError ntt_impl(const bn254_scalar_t* input, int size, NTTDir dir, const NTTConfig* cfg, bn254_scalar_t* output, const isnark::NttFuse* fuse)
{
  // 1. arguments and domain
  if (!cfg || !input || !output) return ICICLE_INVALID_POINTER;
  if (size <= 0 || (size & (size - 1))) {
    set_last_error("ntt: size %d is not a power of two", size);
    return ICICLE_INVALID_ARGUMENT;
  }
  if ((int)cfg->ordering < (int)kNN || (int)cfg->ordering > (int)kMN) {
    set_last_error("ntt: unknown ordering %d", (int)cfg->ordering);
    return ICICLE_INVALID_ARGUMENT;
  }
  ICICLE_TRY(require_device());
  const int logn = ilog2((uint64_t)size);
  Domain dom;
  {
    std::lock_guard<std::mutex> lk(g_dom_mu);
    dom = g_dom;
  }
  if (!dom.tw || logn > dom.log_n) {
    // the reference throws here (ntt.cuh:669-674); a C ABI returns the code instead
    set_last_error("ntt: size 2^%d exceeds the initialised domain (2^%d)", logn, dom.log_n);
    return ICICLE_INVALID_ARGUMENT;
  }
  const int batch = cfg->batch_size > 0 ? cfg->batch_size : 1;
  const uint64_t n = (uint64_t)size, total = n * batch;
  hipStream_t s = (hipStream_t)cfg->stream;
  const bool inverse = dir == kInverse;

  // 2. operands on the device, in the passes' layout.  Orderings (icicle/include/icicle/ntt.h:32-43): kNM / kMN ("mixed" digit order,
  // defined by the CUDA backend's radix plan) are taken as kNR / kRN, exactly as the reference's radix-2 CPU backend does (ntt.h:32).
  Staged sin, sout;
  ICICLE_TRY(sin.in(input, total * sizeof(fe), cfg->are_inputs_on_device, s));
  ICICLE_TRY(sout.out(output, total * sizeof(fe), cfg->are_outputs_on_device, s));
  Relayout lay;
  lay.rev_in = cfg->ordering == kRN || cfg->ordering == kRR || cfg->ordering == kMN;
  lay.rev_out = cfg->ordering == kNR || cfg->ordering == kRR || cfg->ordering == kNM;
  lay.cols = cfg->columns_batch && batch > 1;
  const fe* d_in = sin.ptr<fe>();
  fe* const d_final = sout.ptr<fe>();
  fe* d_out = d_final;
  ICICLE_TRY(stage_layout(lay, d_in, d_out, n, batch, logn, s));

  // 3. coset powers
  fe* d_gpow = nullptr;
  ICICLE_TRY(coset_powers(cfg, inverse, logn, &d_gpow));

  // 4. plan
  static const bool allow29 = env_int("ICICLE_SNARK_NTT29", 1) != 0;
  const FuseKind kind = fuse && fuse->fused_out ? FUSE_ABC : fuse && fuse->scale_tab ? FUSE_SCALE_TAB : FUSE_NONE;
  const Plan plan = ntt_plan(logn, dom.log_n, batch, inverse, allow29, dom.tw29 != nullptr, kind, lay.rev_out, lay.cols);
  if (plan.err != ICICLE_SUCCESS) {
    set_last_error("%s", plan.msg);
    return plan.err;
  }

  // 5. passes (the forward coset multiplies x_j by g^j into scratch first, and the transform reads that)
  WsScoped<fe> scratch;
  const bool pre_coset = d_gpow && !inverse;
  if (plan.need_scratch || pre_coset) HIP_TRY(scratch.alloc(total, s), ICICLE_ALLOCATION_FAILED);
  if (pre_coset) {
    HIP_TRY(hipMemcpyAsync(scratch.p, d_in, total * sizeof(fe), hipMemcpyDeviceToDevice, s), ICICLE_COPY_FAILED);
    ICICLE_TRY(coset_mul(scratch.p, n, batch, d_gpow, logn, s));
    d_in = scratch.p;
  }
  fe* const buf[3] = {const_cast<fe*>(d_in), scratch.p, d_out};
  ICICLE_TRY(enqueue_passes(plan, dom, buf, n, fuse, s));

  // 6. inverse coset, the caller's layout, releases
  if (d_gpow && inverse) ICICLE_TRY(coset_mul(d_out, n, batch, d_gpow, logn, s));
  if (lay.rev_out || lay.cols) {
    hipLaunchKernelGGL(relayout_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_out, d_final, n, batch, logn, lay.rev_out ? 1 : 0, lay.cols ? 1 : 0, 1);
    ICICLE_TRY(check_launch("ntt_relayout_out"));
  }
  lay.pre.release();
  lay.post.release();
  scratch.release();
  if (d_gpow) {
    HIP_TRY(hipStreamSynchronize(s), ICICLE_SYNCHRONIZATION_FAILED);
    HIP_TRY(hipFree(d_gpow), ICICLE_DEALLOCATION_FAILED);
  }
  ICICLE_TRY(sout.finish());
  return end_call(s, cfg->is_async);
}
} // namespace

ISNARK_API eIcicleError bn254_ntt(const bn254_scalar_t* input, int size, NTTDir dir, const NTTConfig* cfg, bn254_scalar_t* output)
{
  return ntt_impl(input, size, dir, cfg, output, nullptr);
}

namespace isnark {
// the prover's transforms (device in/out, natural order, asynchronous on `s`), with the fusions of NttFuse
eIcicleError ntt_fused(fe* d_inout, uint32_t n, int batch, bool inverse, hipStream_t s, const NttFuse& fuse)
{
  NTTConfig nc;
  memset(&nc, 0, sizeof nc);
  nc.stream = s;
  nc.coset_gen.limbs[0] = 1;
  nc.batch_size = batch;
  nc.ordering = kNN;
  nc.are_inputs_on_device = nc.are_outputs_on_device = true;
  nc.is_async = true;
  return ntt_impl((const bn254_scalar_t*)d_inout, (int)n, inverse ? kInverse : kForward, &nc, (bn254_scalar_t*)d_inout, &fuse);
}
// full 2048-element tiles in every pass (what the fused epilogue needs)
bool ntt_fusable(uint32_t n) { return n >= (1u << 12); }
// tab[i] = n⁻¹ · ω_{2n}^i  (Montgomery form), i < n: the per-element scale that folds 1/n and the coset keys g^i
// (g = ω_2n, src/cache.rs:183-184,264-289) into the last pass of the inverse transform
__global__ __launch_bounds__(256) void ntt_scaled_keys_kernel(const fe* __restrict__ tw, uint32_t tw_stride, uint32_t n, fe ninv_mont, fe* __restrict__ tab)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) g_put(tab + i, Fr::mul(g_get(tw + (size_t)i * tw_stride), ninv_mont));
}
eIcicleError ntt_build_scaled_keys(uint32_t n, fe* d_tab, hipStream_t s)
{
  int lg = 0;
  const fe* tw = ntt_domain_table(&lg);
  if (!tw || (1ull << lg) < 2ull * n) {
    set_last_error("ntt_build_scaled_keys: the domain must hold 2n = %llu roots", 2ull * n);
    return ICICLE_INVALID_ARGUMENT;
  }
  fe nn = Fr::zero();
  nn.l[0] = n;
  const fe ninv = Fr::inv(Fr::to_mont(nn));
  hipLaunchKernelGGL(ntt_scaled_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, s, tw, (uint32_t)((1ull << lg) / (2ull * n)), n, ninv, d_tab);
  return check_launch("ntt_scaled_keys");
}
} // namespace isnark

// first launch of a translation unit's code object loads it onto the device (milliseconds): prewarm_modules (runtime.cpp) does that ahead
// of the first prove of a process
namespace isnark {
__global__ void module_warm_ntt_kernel() {}
void module_warm_ntt(hipStream_t s) { hipLaunchKernelGGL(module_warm_ntt_kernel, dim3(1), dim3(1), 0, s); }
} // namespace isnark
