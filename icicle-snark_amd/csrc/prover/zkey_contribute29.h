// zkey_contribute29.h — one point of groth16_zkey_contribute (zkey_contribute.hip), host and device: k·P for a
// scalar k that every lane of the kernel shares.  zc_scale_g1_kernel runs one lane per point of sections 8 and 9 through zc_scale;
// the host scales the header's δ₁ and δ₂ and the record's commitment with the same text, and the F29_CHECK host build
// (tests/zkey_contribute29_check.cpp) compiles it.
//
//   zc_recode(k)          k < r in standard form → its non-adjacent form Σ dᵢ·2ⁱ, dᵢ ∈ {−1, 0, 1}, no two neighbours non-zero, as two
//                         bit masks (bit i of `nonzero`: dᵢ ≠ 0; of `negative`: dᵢ = −1) and the length (the top digit's index + 1;
//                         0 for k = 0).  With h = 3k, dᵢ = h_{i+1} − k_{i+1}: nonzero = (h ⊕ k) ≫ 1, negative = (k ∧ ¬h) ≫ 1 — no
//                         branch on a bit of k.  k < r < 2^254, so h < 2^256 fits eight words and the length is at most 255
//                         (k = 3·2^252 < r: h = 9·2^252, the form is 2^254 − 2^252).
//   zc_scale(P, digits)   [k]·P for P affine as the .zkey holds it (packed Montgomery-256) and NOT the identity: a left-to-right
//                         walk, one x_dbl per digit and one x_madd of P or −P per non-zero digit — on average a third of them.
//                         The masks are read a word per 32 steps with the loop counter as the index: in a kernel they arrive by
//                         value in the argument struct, the index is the same in every lane, and the words stay in scalar
//                         registers — no per-lane scalar, no scratch.
//   zc_mul_affine(P, k)   the host's whole path: recode, scale, back to the file's form (the identity in, or k = 0: all zero).
//
// BOUNDS.  Everything is ec29.h's XYZZ layer under its own invariant (X: N, < 7p for G1, < 2p for G2; Y, ZZ, ZZZ: N, < 2p): x_madd
// and x_dbl take and return it.  P and −P come from load_affine(·, MONT256, negate): canonical words from memory, negated there
// (p − y), then from_mont256 — N, < 1.01p per coordinate.  The caller has run classify_g1 / classify_g2 (zkey_check29.h) on the
// words first: coordinates below q, on the curve, so the canonical operand from_mont256's bound is stated for.  The accumulator
// starts as the identity: the leading x_dbl returns it, the first x_madd copies P.  x_madd's rare branches are exact: acc = −P
// before a digit −1 (k = r − 2: the prefix is (r − 1)/2·2) doubles through x_dbl_affine_exact, and no prefix of a form of k < r is
// ≡ 0 or makes acc = ∓P before a digit ±1 otherwise, so k = 1, 2 and r − 1 take the common path.
//
// The walk's length and its additions depend on k, which groth16_zkey_contribute keeps secret (δ′⁻¹): the same for every lane, so
// nothing diverges, but the kernel's duration is not independent of it.  Stated, not hidden.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../ec29.h"

#if defined(__HIPCC__)
#define ZC_HD __host__ __device__ inline
#else
#define ZC_HD inline
#endif

namespace bn254 {
namespace zc29 {

struct ZcDigits {
  uint32_t nonzero[8], negative[8]; // 2 × 32 bytes: bit i ↔ digit i
  int32_t len;                      // ≤ 255
};

ZC_HD ZcDigits zc_recode(const fe& k)
{
  uint32_t h[8]; // 3k < 2^256
  uint64_t carry = 0;
  for (int i = 0; i < 8; i++) {
    const uint64_t t = 3ull * k.l[i] + carry;
    h[i] = (uint32_t)t;
    carry = t >> 32;
  }
  ZcDigits d;
  d.len = 0;
  for (int i = 0; i < 8; i++) {
    const uint32_t nz = h[i] ^ k.l[i], ng = k.l[i] & ~h[i];
    const uint32_t nz_up = i < 7 ? h[i + 1] ^ k.l[i + 1] : 0u, ng_up = i < 7 ? k.l[i + 1] & ~h[i + 1] : 0u;
    d.nonzero[i] = nz >> 1 | nz_up << 31;
    d.negative[i] = ng >> 1 | ng_up << 31;
    if (d.nonzero[i]) d.len = 32 * i + 32 - __builtin_clz(d.nonzero[i]);
  }
  return d;
}

// [k]·P, k by its digits (len ≥ 1 for a point; len = 0 gives the identity), P not the identity
template <class CL>
ZC_HD typename CL::X zc_scale(const typename CL::Old::A& base, const ZcDigits& d)
{
  const typename CL::A pos = CL::load_affine(base, CL::MONT256, false), neg = CL::load_affine(base, CL::MONT256, true);
  typename CL::X acc = CL::x_zero();
  if (d.len <= 0) return acc;
  const int top = (d.len - 1) >> 5;
  for (int w = top; w >= 0; w--) {
    const uint32_t nz = d.nonzero[w], ng = d.negative[w];
    for (int b = w == top ? ((d.len - 1) & 31) : 31; b >= 0; b--) {
      acc = CL::x_dbl(acc);
      if ((nz >> b) & 1u) CL::x_madd(acc, (ng >> b) & 1u ? neg : pos);
    }
  }
  return acc;
}

// k·P in the file's form from the file's form: affine, packed Montgomery-256, the identity all zero.  C: ec.h's curve, CL: its lazy layer.
template <class C, class CL>
ZC_HD typename C::A zc_mul_affine(const typename C::A& base, const fe& k)
{
  if (C::aff_is_zero(base)) return base;
  return C::p_to_affine(C::x_to_projective(CL::x_store(zc_scale<CL>(base, zc_recode(k)))));
}

} // namespace zc29
} // namespace bn254
