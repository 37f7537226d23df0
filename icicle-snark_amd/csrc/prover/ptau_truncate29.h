// ptau_truncate29.h — one lane of groth16_ptau_truncate's fix-up (ptau_truncate.hip), host and device: B − [s]·Q for
// a point B that differs from lane to lane, a full-width scalar s that the lane computes for itself, and ONE point Q that every
// lane shares.  The kernel runs a lane per element of section 12's block p + 1 through pt_lane; the host builds the table of Q with
// pt_fill_bases and pt_fill_rows, and the F29_CHECK host build (tests/ptau_truncate29_check.cpp) compiles the same text.
//
//   the scalar                  s_j = ω′^j·(2n′)⁻¹, n′ = 2^p, ω′ the root of order 2n′: ptau_contribute29.h's split, unchanged —
//                               pc_lane_scalar(hi[j ≫ k], lo[j mod 2^k]) with lo[i] = ω′^i and hi[m] = (2n′)⁻¹·ω′^(m·2^k),
//                               k = pc_table_bits(p).  The tables are public.
//   pt_next_digit(s, carry)     the next signed digit of width PT_C = 5 from the LOW end: v = (s mod 32) + carry, s ← s ≫ 5,
//                               v > 16 gives v − 32 and a carry.  Digits lie in [−15, 16]; Σ d_w·32^w = s.  s < 2^254 (r is below
//                               it): window 50 holds bits 250 … 253 and the carry, at most 16, so no carry leaves the top.  The
//                               scalar is a shift register of eight words: no array is indexed by a per-lane value.
//   pt_walk(s, fetch)           [s]·Q = Σ_w d_w·32^w·Q: one x_madd per non-zero digit of the row |d_w|·32^w·Q, y negated for a
//                               negative digit — at most PT_WINDOWS = 51 mixed additions, 31/32 of them on average, and NO
//                               doubling: pp_scale's walk is 256 doublings and 85 additions on average.  fetch(i) returns table
//                               entry i; the kernel reads LDS by it, the host an array.
//   pt_lane(B, hi, lo, fetch)   B − T, T = [s]·Q, as pp_side makes P − T: −(T − B), one x_madd of −B into T and x_neg.
//   pt_fill_bases, pt_fill_rows bases[w] = 32^w·Q by doublings, then row by row — ranges of rows side by side on the worker pool —
//                               table[16·w + d − 1] = d·32^w·Q, d = 1 … 16, w < 51: 816 affine points in the bucket kernels'
//                               encoding (packed canonical Montgomery-261: load_affine(·, INTERNAL, negate) is an unpack and a
//                               subtraction, no multiplication), 52 224 bytes — three workgroups' tables fit a CU's 160 KB of LDS.
//                               Width 6 would save 8 additions a lane for 88 064 bytes: one workgroup a CU.  Host point arithmetic.
//
// EXACTNESS.  Q is in the order-r group and not the identity (the caller skips an identity Q), so every row d·32^w·Q with d·32^w < r
// is a point, never the identity.  The additions of the walk come in any order: a partial sum that is the identity makes x_madd copy
// the row; one that equals ± the row takes x_madd's same-x branch, which doubles exactly (x_dbl_affine_exact) or cancels to the
// all-zero identity.  pt_lane: B the identity: no x_madd, −T; T = B: the same branch cancels, x_neg keeps the identity; T = −B: the
// same branch doubles, −(2T) = 2B = B − T.  An identity stays all-zero limbs throughout.
//
// BOUNDS.  ec29.h's XYZZ layer under its own invariant (X: N, < 7p; Y, ZZ, ZZZ: N, < 2p); x_madd takes and returns it.  A row comes
// from load_affine(·, INTERNAL, negate): canonical words unpacked (N, < p), y negated as 2p − y (limbs < 2^30, < 2p) — the operand the
// bucket accumulation feeds x_madd.  −B comes from load_affine(·, MONT256, true) on words the caller has sent through classify_g1.
// x_neg is ptau_prepare29.h's.  The scalar is ff.h's Fr: below r after from_mont.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ptau_contribute29.h"

namespace bn254 {
namespace pt29 {

constexpr int PT_C = 5;                                  // digit width
constexpr int PT_WINDOWS = 51;                           // 51·5 = 255 bits: s < 2^254 and the carry
constexpr int PT_ROW = 1 << (PT_C - 1);                  // |d| = 1 … 16
constexpr int PT_TABLE_POINTS = PT_WINDOWS * PT_ROW;     // 816
constexpr int PT_LDS_BYTES = PT_TABLE_POINTS * 64;       // 52 224

// the low digit of s and s ← s ≫ PT_C; carry in and out
PP_HD int pt_next_digit(uint32_t s[8], uint32_t& carry)
{
  const uint32_t v = (s[0] & ((1u << PT_C) - 1)) + carry;
  for (int i = 0; i < 7; i++) s[i] = s[i] >> PT_C | s[i + 1] << (32 - PT_C);
  s[7] >>= PT_C;
  carry = v > (uint32_t)PT_ROW ? 1u : 0u;
  return (int)v - (int)(carry << PT_C);
}

// [s]·Q from Q's table; s < 2^254
template <class Fetch>
PP_HD G1L::X pt_walk(const fe& s, const Fetch& fetch)
{
  uint32_t reg[8], carry = 0;
  for (int i = 0; i < 8; i++) reg[i] = s.l[i];
  G1L::X acc = G1L::x_zero();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int w = 0; w < PT_WINDOWS; w++) {
    const int d = pt_next_digit(reg, carry);
    if (d == 0) continue;
    const G1::A row = fetch((uint32_t)(w * PT_ROW + (d < 0 ? -d : d) - 1));
    G1L::x_madd(acc, G1L::load_affine(row, G1L::INTERNAL, d < 0));
  }
  return acc;
}

// B − [s]·Q, s from the lane's two table entries; B the file's form, the identity all zero
template <class Fetch>
PP_HD G1L::X pt_lane(const G1::A& b, const fe& hi_mont, const fe& lo_mont, const Fetch& fetch)
{
  const G1L::X t = pt_walk(pc29::pc_lane_scalar(hi_mont, lo_mont), fetch);
  return pp29::pp_side<Fq29>(t, b, true);
}

// the host's fetch: entry i of an array
struct PtArrayFetch {
  const G1::A* table;
  G1::A operator()(uint32_t i) const { return table[i]; }
};

inline G1::A pt_file_form(const G1L::X& x) { return G1::p_to_affine(G1::x_to_projective(G1L::x_store(x))); }

// bases[w] = 2^(PT_C·w)·Q, w < PT_WINDOWS, in the file's form; Q the file's form, on the curve, NOT the identity
inline void pt_fill_bases(const G1::A& q_file, G1::A* bases)
{
  G1L::X acc = G1L::x_zero();
  G1L::x_madd(acc, G1L::load_affine(q_file, G1L::MONT256, false)); // (the identity += Q: a copy)
  for (int w = 0; w < PT_WINDOWS; w++) {
    bases[w] = pt_file_form(acc);
    for (int i = 0; i < PT_C; i++) acc = G1L::x_dbl(acc);
  }
}
// rows first ≤ w < last of the table: table[PT_ROW·w + d − 1] = d·bases[w] in the internal encoding — a range, so that ranges can be
// filled side by side
inline void pt_fill_rows(const G1::A* bases, int first, int last, G1::A* table)
{
  for (int w = first; w < last; w++) {
    const G1L::A b = G1L::load_affine(bases[w], G1L::MONT256, false);
    G1L::X acc = G1L::x_zero();
    for (int d = 1; d <= PT_ROW; d++) {
      G1L::x_madd(acc, b); // (d = 1 copies, d = 2 doubles through the exact branch)
      table[w * PT_ROW + d - 1] = G1L::store_affine_internal(G1L::load_affine(pt_file_form(acc), G1L::MONT256, false));
    }
  }
}
// the whole table, in two ranges of rows
inline void pt_fill_table(const G1::A& q_file, G1::A* table)
{
  G1::A bases[PT_WINDOWS];
  pt_fill_bases(q_file, bases);
  pt_fill_rows(bases, 0, PT_WINDOWS / 2, table);
  pt_fill_rows(bases, PT_WINDOWS / 2, PT_WINDOWS, table);
}

// the host's whole lane in the file's form
inline G1::A pt_lane_affine(const G1::A& b, const fe& hi_mont, const fe& lo_mont, const G1::A* table)
{
  const PtArrayFetch fetch = {table};
  return pt_file_form(pt_lane(b, hi_mont, lo_mont, fetch));
}

} // namespace pt29
} // namespace bn254
