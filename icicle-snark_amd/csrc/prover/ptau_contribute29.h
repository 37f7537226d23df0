// ptau_contribute29.h — one lane of groth16_ptau_contribute (ptau_contribute.hip), host and device: s·P for a
// full-width scalar s that differs from lane to lane and is computed in the lane, s = c·τ′^i for element i of a section.  The
// kernel runs one lane per point through pc_lane; the host builds the two tables with pc_fill_powers, and the F29_CHECK host build
// (tests/ptau_contribute29_check.cpp) compiles the same text.
//
//   pc_table_bits(power)        k = (power + 2)/2: the index i < 2^(power+1) splits into i ≫ k < 2^(power+1−k) and i mod 2^k.
//   pc_fill_powers(…)           out[i] = start·base^i for i in [first, last), Montgomery form in and out: lo[j] = τ′^j with
//                               start = 1, base = τ′; hi_c[m] = c·τ′^(m·2^k) with start = c, base = τ′^(2^k).
//   pc_lane_scalar(hi, lo)      from_mont(hi·lo): (c·τ′^(m·2^k)·R)·(τ′^j·R)·R⁻¹ = c·τ′^(m·2^k + j)·R, then one more R⁻¹ — the
//                               standard form of c·τ′^i, canonical (Fr::mul reduces below r).
//   pc_lane(P, hi, lo)          [s]·P: zc_recode(s), then pp29::pp_scale's walk — the masks as shift registers, no array indexed
//                               by a per-lane value.  P the identity (all zero) stays the identity.
//   pc_lane_affine(P, hi, lo)   the host's whole lane, back in the file's form.
//
// EXACTNESS.  τ′, c ∈ [1, r) and r is prime, so s = c·τ′^i is never 0 and zc_recode gives a form of length ≥ 1.  s = 1 (i = 0 of
// sections 2 and 3, or τ′ = 1) is the form "1": 255 doublings of the identity, which x_dbl returns untouched, and one x_madd that
// copies P — no special case.  Every point is in the order-r group (G1: every point of the curve; G2: classify_g2's subgroup
// test), so pp_scale's statement holds as ptau_prepare29.h makes it: a prefix of the form times P is the identity only for prefix
// ≡ 0 (r), ±P only for prefix ≡ ±1, and x_madd's same-x branch doubles exactly or cancels.
//
// BOUNDS.  The scalar is ff.h's Fr throughout: Montgomery words below r in the tables (Fr::mul's output), below r after
// from_mont; zc_recode takes k < r < 2^254, so 3k < 2^256.  The point arithmetic is pp_scale's under ec29.h's XYZZ invariant (X: N,
// < 7p for G1, < 2p for G2; Y, ZZ, ZZZ: N, < 2p), entered through load_affine(·, MONT256, ·) on words the caller has sent through
// classify_g1 / classify_g2: nothing of ptau_prepare29.h's BOUNDS paragraph changes, and nothing is added to it.
//
// The walk's additions follow s, which is secret: lanes diverge where their digits differ, and a kernel's duration depends on the
// digits of all its lanes.  Stated, not hidden.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ptau_prepare29.h"

namespace bn254 {
namespace pc29 {

using zc29::ZcDigits;

PP_HD uint32_t pc_table_bits(uint32_t power) { return (power + 2) / 2; }

// base^e, Montgomery form
inline fe pc_pow(fe base_mont, uint64_t e)
{
  fe acc = Fr::to_mont(Fr::one_std());
  for (; e; e >>= 1) {
    if (e & 1) acc = Fr::mul(acc, base_mont);
    base_mont = Fr::sqr(base_mont);
  }
  return acc;
}
// out[i] = start·base^i, first ≤ i < last: a range of a table, so that ranges can be filled side by side
inline void pc_fill_powers(const fe& base_mont, const fe& start_mont, size_t first, size_t last, fe* out)
{
  fe x = Fr::mul(start_mont, pc_pow(base_mont, first));
  for (size_t i = first; i < last; i++) {
    out[i] = x;
    x = Fr::mul(x, base_mont);
  }
}

// c·τ′^i in standard form from the two table entries of i
PP_HD fe pc_lane_scalar(const fe& hi_mont, const fe& lo_mont) { return Fr::from_mont(Fr::mul(hi_mont, lo_mont)); }

// [c·τ′^i]·P; P the file's form, the identity all zero
template <class F>
PP_HD typename CurveL<F>::X pc_lane(const typename CurveL<F>::Old::A& p, const fe& hi_mont, const fe& lo_mont)
{
  typedef CurveL<F> CL;
  if (CL::Old::aff_is_zero(p)) return CL::x_zero();
  const ZcDigits d = zc29::zc_recode(pc_lane_scalar(hi_mont, lo_mont));
  return pp29::pp_scale<F>(p, d);
}

// the host's whole lane in the file's form: C ec.h's curve, F its lazy field
template <class C, class F>
inline typename C::A pc_lane_affine(const typename C::A& p, const fe& hi_mont, const fe& lo_mont)
{
  return C::p_to_affine(C::x_to_projective(CurveL<F>::x_store(pc_lane<F>(p, hi_mont, lo_mont))));
}

} // namespace pc29
} // namespace bn254
