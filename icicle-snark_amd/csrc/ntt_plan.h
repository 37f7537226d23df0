// ntt_plan.h — the host plan of a transform, apart from the kernels and the code that launches them (ntt.hip), so that a host
// build can walk it over every size: tests/ntt_plan_check.cpp.
//
//  PassParams / Plan29   what a pass kernel is handed by value: the tile's geometry and the radix-2^29 value bounds
//  plan29 / bounds29     the pass split and the bounds of the radix-2^29 kernels
//  ntt_plan              everything ntt.hip enqueues for one transform, as data: 1–3 passes with their parameters (pointers
//                        left null), kernel form, dynamic LDS, grid and buffers — or the error the call returns
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/icicle_snark_hip.h"
#include "ff.h"

namespace isnark {
namespace ntt {

using bn254::fe;

constexpr int LOG_TILE = 11; // 2048 elements per workgroup
constexpr int NT = 256;      // threads per workgroup
constexpr int MAX_LOG_R = 9; // rows per tile ≤ 512 so that columns ≥ 4 (128-B runs)

struct PassParams {
  int log_r, log_c;
  uint32_t tiles_per_group_log; // b -> b_hi = b >> log, b_lo = b & mask
  uint64_t in_hi, in_lo, in_row, in_col;
  uint64_t out_hi, out_lo, out_row, out_col;
  uint32_t tw_mul;       // inter-pass twiddle exponent = k · (b_lo·C + c) · tw_mul ; 0 = none
  uint32_t stage_stride; // ω_R^e = tw[e · stage_stride]
  uint32_t n_mask;       // N − 1
  int inverse;
  int scale; // multiply by n^-1 (last pass of an inverse transform)
  uint64_t batch_stride;
  int load_rows_fastest; // global loads: consecutive threads walk rows (in_row == 1) instead of columns
  // prover fusions (last pass only; full 2048-element tiles):
  const fe* scale_tab;   // non-null: out[i] *= scale_tab[i·scale_stride] (i = natural output index) INSTEAD of the n⁻¹ constant —
  uint32_t scale_stride; // the prover passes n⁻¹·g^i, which folds the coset keys of src/proof_helper.rs:121-141 into the inverse transform
  int fuse_abc;          // batch of 3 rows [B | A | C'] handled by ONE workgroup per tile: writes A·B − C' (src/proof_helper.rs:154-167) to row 0 of `out`
  // radix-2^29 passes: 1-D grid of tiles·batch workgroups with the rows of ONE tile on consecutive workgroups of the SAME XCD
  // (workgroup b runs on XCD b mod 8): they gather the same inter-pass twiddles, and each XCD has its own L2
  uint32_t xcd_batch;    // 0: grid (tiles, batch) as before; else the batch count of the 1-D grid (tiles is a multiple of 8)
};
struct Plan29 {
  uint32_t b0;       // bound of the tile's values at the load (multiples of r): level l of a round that is not the last sees b0·2^l
  uint32_t bs;       // bound at the start of the last round (after the shrink, if any): its level t sees (bs + 1)·2^t − 1
  int shrink_last;   // apply fr29::shrink to the operands of the last round
};
static_assert(sizeof(PassParams) == 144 && sizeof(Plan29) == 12, "both are kernel arguments passed by value");

inline int ilog2(uint64_t x)
{
  int l = 0;
  while ((1ull << l) < x) l++;
  return l;
}

// pass plan of the radix-2^29 kernel: 2 or 3 passes of 4 … 8 bits whose tiles are all full (2048 elements), fewest LDS rounds
inline bool plan29(int logn, int& np, int (&lr)[3])
{
  int best = 1 << 30;
  auto full = [&](const int* l, int n) {
    uint64_t rem = 1ull << logn;
    for (int pi = 0; pi < n; pi++) {
      const uint64_t C = 1ull << (LOG_TILE - l[pi]);
      if (pi < n - 1) {
        const uint64_t tail = rem >> l[pi];
        if (C > tail) return false;
        rem = tail;
      } else if (C > (1ull << l[0])) return false;
    }
    return true;
  };
  for (int a = 8; a >= 4; a--)
    for (int b = 8; b >= 4; b--) {
      {
        const int l2[2] = {a, b};
        const int cost = (a + 2) / 3 + (b + 2) / 3;
        if (a + b == logn && cost < best && full(l2, 2)) { best = cost; np = 2; lr[0] = a; lr[1] = b; lr[2] = 0; }
      }
      for (int c = 8; c >= 4; c--) {
        const int l3[3] = {a, b, c};
        const int cost = (a + 2) / 3 + (b + 2) / 3 + (c + 2) / 3 + 1; // a third pass costs more than a round
        if (a + b + c == logn && cost < best && full(l3, 3)) { best = cost; np = 3; lr[0] = a; lr[1] = b; lr[2] = c; }
      }
    }
  return best < (1 << 30);
}
// value bounds of one pass (multiples of r): b_in at the load, ×2 per level (sums), 2B + 1 per level of the last round (its unit
// twiddles leave differences unmultiplied); one shrink (B → B/4 + 1) in front of the last round when the end would pass `limit`
inline bool bounds29(int log_r, uint32_t b_in, uint32_t limit, Plan29& pl)
{
  memset(&pl, 0, sizeof pl);
  const int q_last = log_r % 3 ? log_r % 3 : 3;
  pl.b0 = b_in;
  uint32_t B = b_in << (log_r - q_last); // at the start of the last round
  uint32_t e = B;
  for (int k = 0; k < q_last; k++) e = 2 * e + 1;
  if (e > limit) {
    pl.shrink_last = 1;
    B = B / 4 + 2;
  }
  pl.bs = B;
  for (int k = 0; k < q_last; k++) {
    if (2 * B + 1 >= 1350) return false; // (K·r)_8 + a_8 must fit 32 bits
    B = 2 * B + 1;
  }
  return B <= limit && (uint64_t)b_in << (log_r - q_last) < 650;
}

enum FuseKind { FUSE_NONE = 0, FUSE_SCALE_TAB, FUSE_ABC }; // NttFuse (ntt_fuse.h): per-element scale table (inverse) | A·B − C' epilogue
enum Buf { BUF_IN = 0, BUF_SCRATCH, BUF_OUT };              // the (relaid / coset-multiplied) input, the scratch block, the output

struct Pass {
  PassParams p;         // scale_tab / scale_stride stay empty: the enqueue fills them when `scale_tab` is set
  Plan29 pl29;          // radix-2^29 passes only
  bool fused, scale_tab; // fused: the FUSE instantiation, storing to NttFuse::fused_out instead of `dst`
  uint32_t lds;         // dynamic LDS bytes
  uint32_t grid_x, grid_y;
  Buf src, dst;
};
struct Plan {
  eIcicleError err; // ≠ ICICLE_SUCCESS: `msg` is the call's error text and nothing is to be enqueued
  char msg[96];
  bool use29;       // the radix-2^29 kernels (ntt_pass29_kernel) run every pass
  bool need_scratch;
  int np;
  Pass pass[3];
};

// The plan of a 2^logn transform in a domain of 2^domain_log roots.  8×32-bit kernels: one pass up to 9 bits, two up to 18, else
// 9 bits first and the rest in halves; the radix-2^29 split (plan29) where it exists, is allowed and has its twiddles.
inline Plan ntt_plan(int logn, int domain_log, int batch, bool inverse, bool allow29, bool have_tw29, FuseKind fuse, bool rev_out, bool cols)
{
  Plan pl;
  memset(&pl, 0, sizeof pl);
  int np, lr[3] = {0, 0, 0};
  if (logn <= MAX_LOG_R) { np = 1; lr[0] = logn; }
  else if (logn <= 2 * MAX_LOG_R) { np = 2; lr[0] = (logn + 1) / 2; lr[1] = logn / 2; }
  else { np = 3; lr[0] = MAX_LOG_R; lr[1] = (logn - MAX_LOG_R + 1) / 2; lr[2] = (logn - MAX_LOG_R) / 2; } // 9 bits = three radix-8 rounds
  // transforms whose passes can all work on full tiles of at most 8 bits run on the lazy radix-2^29 field (ntt_pass29_kernel)
  int np29 = 0, lr29[3] = {0, 0, 0};
  pl.use29 = allow29 && have_tw29 && plan29(logn, np29, lr29);
  if (pl.use29) {
    np = np29;
    for (int k = 0; k < 3; k++) lr[k] = lr29[k];
  }
  pl.np = np;
  pl.need_scratch = np > 1;
  const uint64_t n = 1ull << logn;
  const uint32_t N = 1u << domain_log;
  const uint32_t dom_stride = N >> logn; // ω_n = ω_N^dom_stride

  uint64_t rem = n; // n_p : size of the sub-transform still to do at pass p
  for (int pi = 0; pi < np; pi++) {
    Pass& ps = pl.pass[pi];
    PassParams& p = ps.p;
    const bool last = pi == np - 1;
    p.log_r = lr[pi];
    const uint64_t R = 1ull << p.log_r;
    const uint64_t tail = rem / R; // n_{p+1}
    int log_c = LOG_TILE - p.log_r;
    p.inverse = inverse;
    p.scale = last && inverse;
    p.n_mask = N - 1;
    p.stage_stride = N >> p.log_r;
    p.batch_stride = n;
    ps.src = pi == 0 ? BUF_IN : BUF_SCRATCH;
    ps.dst = last ? BUF_OUT : BUF_SCRATCH;
    uint64_t tiles;
    if (!last) {
      // in-place positions: pos = head·rem + j·tail + t ; tile = C consecutive t
      if ((uint64_t)(1 << log_c) > tail) log_c = ilog2(tail);
      p.log_c = log_c;
      const uint64_t C = 1ull << log_c;
      const uint64_t tpg = tail / C; // tiles per head
      p.tiles_per_group_log = ilog2(tpg);
      p.in_hi = rem; p.in_lo = C; p.in_row = tail; p.in_col = 1;
      p.out_hi = rem; p.out_lo = C; p.out_row = tail; p.out_col = 1;
      p.tw_mul = (uint32_t)((uint64_t)dom_stride * (n / rem)); // ω_rem^(k·t) = ω_N^(dom_stride·(n/rem)·k·t)
      p.load_rows_fastest = 0;
      tiles = (n / rem) * tpg;
    } else {
      // last pass: rows contiguous (tail == 1); columns walk the leading output digit k1
      const uint64_t R1 = np == 1 ? 1 : (1ull << lr[0]);
      if ((uint64_t)(1 << log_c) > R1) log_c = ilog2(R1);
      p.log_c = log_c;
      const uint64_t C = 1ull << log_c;
      const uint64_t mid = n / (R1 * R);   // product of the middle radices (R2 for 3 passes, else 1)
      const uint64_t tpg = R1 / C;         // tiles per middle index
      p.tiles_per_group_log = ilog2(tpg);
      p.in_lo = C * (n / R1); p.in_hi = R; p.in_row = 1; p.in_col = n / R1;
      p.out_lo = C; p.out_hi = R1; p.out_row = R1 * mid; p.out_col = 1;
      p.tw_mul = 0;
      p.load_rows_fastest = 1;
      tiles = tpg * mid;
    }
    ps.lds = (uint32_t)(((size_t)2 << (p.log_r + p.log_c)) * 16 + (size_t)(R >> 1) * 32 + 32);
    const bool full_tile = ((size_t)1 << (p.log_r + p.log_c)) == (size_t)NT * 8;
    ps.scale_tab = last && fuse == FUSE_SCALE_TAB && inverse;
    if (pl.use29) {
      // bounds: the first pass reads canonical values, later ones what a pass stored (< 4); a pass ends in a product (→ < 4) except
      // the last pass of a forward transform, plain or with the fused epilogue (→ canon / sub<600>)
      const bool ends_in_product = !last || inverse;
      if (!full_tile || !bounds29(p.log_r, pi == 0 ? 1u : 4u, ends_in_product ? 506u : 598u, ps.pl29)) {
        snprintf(pl.msg, sizeof pl.msg, "ntt: internal error — no radix-2^29 bound plan for a %d-bit pass", p.log_r);
        pl.err = ICICLE_UNKNOWN_ERROR;
        return pl;
      }
      ps.lds = (uint32_t)((size_t)NT * 8 * 36 + (size_t)(R >> 1) * 36);
    }
    ps.grid_x = (uint32_t)tiles;
    ps.grid_y = (uint32_t)batch;
    if (last && fuse == FUSE_ABC) {
      // A·B − C' epilogue: one workgroup per tile walks the three rows
      if (!full_tile || batch != 3 || inverse || rev_out || cols) {
        snprintf(pl.msg, sizeof pl.msg, "ntt: fused epilogue needs a forward batch-of-3 transform with full tiles");
        pl.err = ICICLE_INVALID_ARGUMENT;
        return pl;
      }
      ps.fused = true;
      p.fuse_abc = 1;
      ps.grid_y = 1;
    } else if (pl.use29 && batch > 1 && tiles % 8 == 0 && (uint64_t)tiles * (uint64_t)batch < (1ull << 31)) {
      // (measured at 3 × 2^21: 0.75 / 0.85 → 0.74 / 0.83 ms per transform alone, −0.1 to −0.2 ms per prove at 1.6 M constraints)
      p.xcd_batch = (uint32_t)batch;
      ps.grid_x = (uint32_t)(tiles * batch);
      ps.grid_y = 1;
    }
    rem = tail;
  }
  return pl;
}

} // namespace ntt
} // namespace isnark
