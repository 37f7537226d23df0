// zkey_new29.h — one column of groth16_zkey_new (zkey_new.hip), host and device: a wire's sum Σ_t v_t·P_t over the
// terms of its column of A, B or C, P_t the ptau's Lagrange point of the term's row.  The kernels run one lane per (wire, output)
// — or per slice of a heavy column — through zn_walk; the F29_CHECK host build (tests/zkey_new29_check.cpp) compiles the same text.
//
//   zn_signed_short(v)   v < r in standard form → |v| = min(v, r − v) as eight words, its bit length, and the sign.  r is odd, so
//                        the two are never equal: v ≤ (r − 1)/2 stays, v ≥ (r + 1)/2 becomes −(r − v).  v = 0: bits = 0.
//   zn_add_term(acc,P,v) acc += v·P.  bits = 0 or P the identity: nothing.  |v| = 1: one x_madd of ±P.  Otherwise a left-to-right
//                        double-and-add over exactly `bits` bits with mixed additions of ±P (zn_mul_bits: pairing29.h's g1_mul_bits
//                        for either group), then x_add into acc.
//   zn_walk(lists,…)     positions [lo, hi) of the concatenation of NL column lists, each with its own base range: comb_s reads
//                        A's column against [β·L]₁, B's against [α·L]₁ and C's against [L]₁ into one accumulator.
//
// BOUNDS.  Everything is ec29.h's XYZZ layer under its own invariant (X: N, < 7p for G1, < 2p for G2; Y, ZZ, ZZZ: N, < 2p): x_madd,
// x_dbl and x_add take and return it.  An affine operand comes from load_affine(·, MONT256, negate): canonical words from memory,
// negated there (p − y), then from_mont256 — N, < 1.01p per coordinate.  Every ptau point that is read has passed classify_g1 /
// classify_g2 (coordinates below q) before a lane of these kernels sees it.  A coefficient is Fr::from_mont of the handle's
// Montgomery value: canonical, below r.  x_add and x_madd handle P + P, P − P and the identity on either side exactly (their
// rare branches), so a column whose partial sum passes through the identity goes on from there.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../ec29.h"

#if defined(__HIPCC__)
#define ZN_HD __host__ __device__ inline
#else
#define ZN_HD inline
#endif

namespace bn254 {
namespace zn29 {

constexpr uint32_t ZN_BINDING = 0xffffffffu; // term index of a public-binding row: coefficient 1, no stored value

struct ZnEntry {
  uint32_t row, term; // the constraint (the ptau point's index in its block), the term's index in the handle's cols / vals
};

struct ZnShort {
  uint32_t w[8];
  int bits;
  bool neg;
};

ZN_HD ZnShort zn_signed_short(const fe& v)
{
  fe n; // r − v (v < r: no borrow out)
  uint64_t br = 0;
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)FrP::MOD[i] - v.l[i] - br;
    n.l[i] = (uint32_t)t;
    br = (t >> 32) & 1;
  }
  bool lt = false; // n < v: the most significant differing word decides
  for (int i = 0; i < 8; i++)
    if (n.l[i] != v.l[i]) lt = n.l[i] < v.l[i];
  ZnShort s;
  s.neg = lt;
  s.bits = 0;
  for (int i = 0; i < 8; i++) {
    s.w[i] = lt ? n.l[i] : v.l[i];
    if (s.w[i]) s.bits = 32 * i + 32 - __builtin_clz(s.w[i]);
  }
  return s;
}

// [z]·P, z of exactly `bits` ≥ 1 bits (little-endian words), P affine and not the identity: g1_mul_bits' walk, one load of a
// scalar word per 32 steps (the words are indexed at run time: they live in scratch)
template <class CL>
ZN_HD typename CL::X zn_mul_bits(const typename CL::A& p, const uint32_t* z, int bits)
{
  typename CL::X acc = CL::x_zero();
  const int top = (bits - 1) >> 5;
  for (int w = top; w >= 0; w--) {
    const uint32_t zw = z[w];
    for (int b = w == top ? ((bits - 1) & 31) : 31; b >= 0; b--) {
      acc = CL::x_dbl(acc);
      if ((zw >> b) & 1u) CL::x_madd(acc, p);
    }
  }
  return acc;
}

// acc += v·P: P as the .ptau holds it (affine, packed Montgomery-256, (0, 0) the identity), v standard form below r
template <class CL>
ZN_HD void zn_add_term(typename CL::X& acc, const typename CL::Old::A& base, const fe& v)
{
  const ZnShort s = zn_signed_short(v);
  if (s.bits == 0 || CL::Old::aff_is_zero(base)) return;
  const typename CL::A p = CL::load_affine(base, CL::MONT256, s.neg);
  if (s.bits == 1) {
    CL::x_madd(acc, p);
    return;
  }
  acc = CL::x_add(acc, zn_mul_bits<CL>(p, s.w, s.bits));
}

template <class CL>
struct ZnList {
  const ZnEntry* e;
  uint32_t len;
  const typename CL::Old::A* bases; // indexed by ZnEntry::row
};

// Σ over the positions [lo, hi) of lists[0] | lists[1] | … (hi ≤ the total length); vals: the handle's Montgomery coefficients
template <class CL, int NL>
ZN_HD typename CL::X zn_walk(const ZnList<CL> (&ls)[NL], const fe* vals, uint32_t lo, uint32_t hi)
{
  static_assert(NL == 1 || NL == 3, "one list, or comb's three");
  typename CL::X acc = CL::x_zero();
  const uint32_t end0 = ls[0].len, end1 = NL == 3 ? end0 + ls[1].len : end0;
  for (uint32_t q = lo; q < hi; q++) {
    const ZnEntry* e = ls[0].e + q;
    const typename CL::Old::A* bases = ls[0].bases;
    if (NL == 3 && q >= end0) {
      const bool third = q >= end1;
      e = third ? ls[NL - 1].e + (q - end1) : ls[NL / 2].e + (q - end0);
      bases = third ? ls[NL - 1].bases : ls[NL / 2].bases;
    }
    const ZnEntry t = *e;
    const fe v = t.term == ZN_BINDING ? Fr::one_std() : Fr::from_mont(vals[t.term]);
    zn_add_term<CL>(acc, bases[t.row], v);
  }
  return acc;
}

} // namespace zn29
} // namespace bn254
