// ptau_prepare29.h — the point arithmetic of groth16_ptau_prepare (ptau_prepare.hip), host and device: one
// butterfly of an inverse NTT whose elements are curve points.  The kernels run one lane per butterfly through pp_butterfly and
// one lane per input through zc29::zc_scale (the 1/2^p every lane shares); the F29_CHECK host build
// (tests/ptau_prepare29_check.cpp) compiles the same text.
//
//   pp_scale(Q, w)              [w]·Q for Q affine as the .ptau holds it (packed Montgomery-256), NOT the identity, and a scalar w
//                               that differs from lane to lane: zc_recode's non-adjacent form kept as two 256-bit shift registers,
//                               256 steps in every lane — x_dbl each (the accumulator is the identity until the top digit: x_dbl
//                               returns it untouched), x_madd of ±Q where the top bit of `nonzero` says so.  The doublings are
//                               uniform over a wave, the additions diverge.  No array is indexed by a per-lane value: the masks
//                               stay in registers.
//   pp_twiddled(Q, w)           T = w·Q (w null: T = Q, level 0); Q the identity gives the identity.
//   pp_side(T, P, minus)        P + T, or P − T as −(T − P): an x_madd of ±P into T.  The kernel makes the two outputs one after
//                               the other, each stored before the next is begun: one x_madd's registers, not two.
//   pp_butterfly(P, Q, w, …)    both outputs.  P and Q affine, either may be the identity (all zero).
//   x_neg(X)                    −(X, Y, ZZ, ZZZ) = (X, −Y, ZZ, ZZZ).
//
// EXACTNESS.  Every point is in the order-r group (G1: every point of the curve; G2: the inputs pass classify_g2's subgroup test,
// and sums and multiples stay inside), w ∈ [1, r).  A prefix of w's form times Q is the identity only for prefix ≡ 0 (r): x_madd
// then copies; it equals ±Q only for prefix ≡ ±1: x_madd's same-x branch doubles exactly or cancels.  T = ±P: the same branch in
// the two sums — one of them doubles (x_dbl_affine_exact), the other is the identity.  Q the identity: T is, the sums are ±P
// (x_madd's copy); P the identity: no x_madd, the sums are ±T.  Both: two identities.  An identity stays all-zero limbs throughout.
//
// BOUNDS.  ec29.h's XYZZ layer under its own invariant (X: N, < 7p for G1, < 2p for G2; Y, ZZ, ZZZ: N, < 2p); x_madd and x_dbl take
// and return it.  ±P and ±Q come from load_affine(·, MONT256, negate): canonical words from memory (the caller has run classify_g1 /
// classify_g2 on them, or they are this library's own affine output), negated there (p − y), then from_mont256: N, < 1.01p.  pp_scale
// keeps Q's x once and both y.  x_neg: Y N, < 2p → sub3(0, Y) = 3p − Y: limbs < 2^29 + 2^30, value in (p, 3p] → lt2p (takes < 8p) → N, < 2p.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "zkey_contribute29.h"

#define PP_HD FF_HD

namespace bn254 {
namespace pp29 {

using zc29::ZcDigits;

template <class F>
PP_HD typename CurveL<F>::X x_neg(typename CurveL<F>::X p)
{
  if (CurveL<F>::x_is_zero(p)) return p;
  p.y = F::lt2p(F::sub3(F::zero(), p.y));
  return p;
}

// [w]·Q, Q not the identity, w by its digits, per lane
template <class F>
PP_HD typename CurveL<F>::X pp_scale(const typename CurveL<F>::Old::A& base, const ZcDigits& d)
{
  typedef CurveL<F> CL;
  const typename CL::A pos = CL::load_affine(base, CL::MONT256, false);
  const typename CL::T neg_y = CL::load_affine(base, CL::MONT256, true).y;
  uint32_t nz[8], ng[8];
  for (int i = 0; i < 8; i++) nz[i] = d.nonzero[i], ng[i] = d.negative[i];
  typename CL::X acc = CL::x_zero();
  for (int step = 0; step < 256; step++) {
    acc = CL::x_dbl(acc);
    if (nz[7] >> 31) {
      typename CL::A b = pos;
      if (ng[7] >> 31) b.y = neg_y;
      CL::x_madd(acc, b);
    }
    for (int i = 7; i > 0; i--) nz[i] = nz[i] << 1 | nz[i - 1] >> 31, ng[i] = ng[i] << 1 | ng[i - 1] >> 31;
    nz[0] <<= 1, ng[0] <<= 1;
  }
  return acc;
}

// T = w·Q (w null: w = 1, no multiplication); Q the file's form, the identity all zero
template <class F>
PP_HD typename CurveL<F>::X pp_twiddled(const typename CurveL<F>::Old::A& q, const ZcDigits* w)
{
  typedef CurveL<F> CL;
  typename CL::X t = CL::x_zero();
  if (CL::Old::aff_is_zero(q)) return t;
  if (w) return pp_scale<F>(q, *w);
  CL::x_madd(t, CL::load_affine(q, CL::MONT256, false)); // (the identity += Q: a copy)
  return t;
}

// one output of the butterfly from T: P + T, or with `minus` P − T = −(T − P)
template <class F>
PP_HD typename CurveL<F>::X pp_side(const typename CurveL<F>::X& t, const typename CurveL<F>::Old::A& p, bool minus)
{
  typedef CurveL<F> CL;
  typename CL::X acc = t;
  if (!CL::Old::aff_is_zero(p)) CL::x_madd(acc, CL::load_affine(p, CL::MONT256, minus));
  return minus ? x_neg<F>(acc) : acc;
}

// sum = P + w·Q, diff = P − w·Q (w null: w = 1).  P, Q: the file's form, the identity all zero.
template <class F>
PP_HD void pp_butterfly(const typename CurveL<F>::Old::A& p, const typename CurveL<F>::Old::A& q, const ZcDigits* w, typename CurveL<F>::X* sum, typename CurveL<F>::X* diff)
{
  const typename CurveL<F>::X t = pp_twiddled<F>(q, w);
  *sum = pp_side<F>(t, p, false);
  *diff = pp_side<F>(t, p, true);
}

// the host's whole butterfly in the file's form: C ec.h's curve, F its lazy field
template <class C, class F>
PP_HD void pp_butterfly_affine(const typename C::A& p, const typename C::A& q, const fe* w, typename C::A* sum, typename C::A* diff)
{
  typedef CurveL<F> CL;
  typename CL::X s, d;
  ZcDigits dg;
  if (w) dg = zc29::zc_recode(*w);
  pp_butterfly<F>(p, q, w ? &dg : nullptr, &s, &d);
  *sum = C::p_to_affine(C::x_to_projective(CL::x_store(s)));
  *diff = C::p_to_affine(C::x_to_projective(CL::x_store(d)));
}

} // namespace pp29
} // namespace bn254
