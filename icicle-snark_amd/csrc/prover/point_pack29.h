// point_pack29.h — the PACKED form of a point of a powers-of-tau file: x and one bit of y, host and device from one text.
// groth16_ptau_pack / groth16_ptau_unpack and groth16_points_pack / _unpack (ptau_pack.hip) run one lane per point through it, the
// host side section 6, and the F29_CHECK host build (tests/point_pack29_check.cpp) compiles the same text.  DESIGN.md §7j.
//
// THE FORM.  A point of the file is affine, canonical Montgomery-256, little-endian, the identity all zero (zkey_check29.h).
//   G1, 32 bytes   x exactly as the file holds it.  q < 2^254, so bits 254 and 255 of the word — bits 6 and 7 of byte 31 — are free:
//                  bit 7 of byte 31 = sign(y), bit 6 of byte 31 = the identity flag.  The identity is the flag alone, 00 … 00 40.
//   G2, 64 bytes   x as the file holds it, c0 then c1; the same two flag bits in byte 63 (the top of c1).  c0 has no flag bits.
//   sign(y), Fq    1 iff the STANDARD-form integer of y is above (q − 1)/2.  Not defined on the Montgomery representative.
//   sign(y), Fq2   the sign of y.c1 when y.c1 ≠ 0, else the sign of y.c0.
// −y = q − y and q is odd: y and −y have opposite signs unless y = 0, so (x, sign) names one point.  pack and unpack are inverse
// bijections between sound file-form points and valid packed words.
//
//   pk_sign_g1 / pk_sign_g2 (mont[2])        the sign of a file-form point's y.  Behind classify_g1 / classify_g2 only: canonical words.
//   pk_pack_g1 / pk_pack_g2 (mont[2], word)  the packed word of a SOUND point (classify = 0; the identity included)
//   pk_sqrt_fq (a, &root)                    root = a^((q+1)/4) as a·a^((q−3)/4); true iff root² = a, compared canonically
//   pk_sqrt_fq2 (a, &root)                   the complex method, below; true iff root² = a, compared canonically
//   pk_unpack_g1 / pk_unpack_g2 (word, mont[2])   0 and the file-form point, or GROTH16_ZKEY_NONCANONICAL / _OFF_CURVE / _OFF_SUBGROUP
//                                            (zkey_check29.h's values) and nothing written.  In this order:
//      1 the flags: an identity flag with any other bit set, the sign bit included, is NONCANONICAL; the flag alone is the identity
//      2 x < q by Fq::is_canonical — an integer comparison — BEFORE any lazy operation sees it: NONCANONICAL
//      3 rhs = x³ + 3, on the twist x³ + 3/ξ (pairing29.h's b_twist, g2_on_twist's constant)
//      4 the root: none is OFF_CURVE
//      5 a root of 0 with the sign bit set is NONCANONICAL (−0 = 0: the word with the clear bit is the point's only one)
//      6 negate to match the sign bit
//      7 G2: g2_in_subgroup_fast, which wants a point on the twist and not the identity — it is: OFF_SUBGROUP
//      8 canonical Montgomery-256 words
//
// THE EXPONENT.  q ≡ 3 (mod 4).  One exponent serves every root: e = (q − 3)/4, 252 bits, a compile-time constant and the same in
// every lane.  pk_pow_e walks it two bits per step from a constant mask indexed by the loop counter (f29::inv's walk): 252 squares
// and 97 products (two for a², a³; 95 non-zero digits), the operand of a step's product chosen by selects among three values — no
// table indexed at run time, no branch that differs between lanes.  With t = a^e:  a·t = a^((q+1)/4), the root when there is one,
// and a·t² = a^((q−1)/2) = ±1 — so t is ±1/(a·t), the root's inverse, for free.
//
// THE Fq2 ROOT (complex method; Fq2 = Fq[u]/(u² + 1)).  For a = a0 + a1·u:
//      n = a0² + a1²,  s = n^((q+1)/4),  δ = (a0 + s)/2   — δ = a0 when a1 = 0 (there s = ±a0 could make δ = 0)
//      t = δ^e,  x0 = δ·t,  h = a1·t/2
//      x0² = δ   (δ a residue):      root = x0 + h·u        since 1/x0 = t and the imaginary part is a1/(2·x0)
//      x0² = −δ  (δ a non-residue):  root = −h + x0·u       since 1/x0 = −t, and with δ′ = (a0 − s)/2 = −a1²/(4δ) the real part is
//                                                            a1/(2·x0), a root of δ′, and the imaginary part a1/(2·real) = x0
// (−1 is a non-residue and δ·δ′ = −a1²/4, so exactly one of δ, δ′ is a residue when n is one; a1 = 0: root = x0 or x0·u.)
// Two walks, no inversion.  When a is no square n is no residue, s is not its root and the result is nonsense — so, WHATEVER the
// branch, the function ends by squaring its result and comparing it with a: no path can emit a wrong point, it can only refuse.
//
// BOUNDS ("I2" = limbs N, value < 2p, Montgomery-261: pairing29.h's invariant; lt2 = reduce_lt2p ∘ norm takes limbs < 2^32 − 2^3, < 8p).
//   X = from_mont256(x)          x canonical (step 2): p·p < 147 p²                                         → N, < 1.01p   (I2)
//   G1 rhs = lt2(X²·X + 3)       sqr 4 p², mul 2.1 p²; three_m limb-wise < 3·2^29, < 3p; sum limbs < 2^31, < 4.1p → I2
//   G2 rhs                       f2_sqr, f2_mul, f2_add of I2 values                                         → I2
//   pk_pow_e(a), a I2            a2 = sqr(a), a3 = mul(a2, a), r = sqr(sqr(r)), mul(r, ·): operands I2, 4 p²   → I2
//   pk_sqrt_fq                   root = mul(a, t), sqr(root): I2 operands; canon takes N, < 16p
//   pk_sqrt_fq2                  n = lt2(a0² + a1²): limbs < 2^30, < 2.1p → I2;  a0 + s: limbs < 2^30, < 4p → lt2 → I2;
//                                two_inv canonical; fq_neg → I2; f2_sqr takes N, < 5p
//   sign                         mul(y, one_std): 2 p² → N, < 1.02p → canon → the standard-form integer, compared limb by limb
//   step 6                       fq_neg / f2_neg of I2 → I2 (0 ↦ p, which canon and to_mont256 bring back to 0)
//   step 8                       to_mont256 takes any I2 value
#pragma once
#include "zkey_check29.h"

namespace bn254 {
namespace pk29 {

using p29::F2;

constexpr uint32_t PK_SIGN_BIT = 1u << 31, PK_IDENTITY_BIT = 1u << 30; // of a word's l[7]: bits 7 and 6 of its last byte

// canonical comparison of two values N, < 16p
FF_HD bool pk_eq(const fe9& a, const fe9& b)
{
  const fe9 ca = f29::canon(a), cb = f29::canon(b);
  bool eq = true;
  for (int j = 0; j < 9; j++) eq = eq && ca.l[j] == cb.l[j];
  return eq;
}
FF_HD bool pk_is_zero(const fe9& a) { return f29::is_zero_canon(f29::canon(a)); } // a N, < 16p
FF_HD fe9 pk_select(bool c, const fe9& a, const fe9& b)
{
  fe9 r;
  for (int j = 0; j < 9; j++) r.l[j] = c ? a.l[j] : b.l[j];
  return r;
}

// a^((q − 3)/4); a I2 → I2
P29_HD fe9 pk_pow_e(const fe9& a)
{
  constexpr uint32_t E[8] = {0xb61f3f51u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u, 0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu}; // (q − 3)/4 < 2^252
  const fe9 a2 = f29::sqr(a), a3 = f29::mul(a2, a);
  fe9 r = f29::one_m();
#pragma unroll 1
  for (int i = 125; i >= 0; i--) {
    r = f29::sqr(f29::sqr(r));
    const uint32_t d = (E[i >> 4] >> ((i & 15) * 2)) & 3u; // the same in every lane
    if (d) r = f29::mul(r, pk_select(d == 1, a, pk_select(d == 2, a2, a3)));
  }
  return r;
}

// a I2.  *root = a^((q+1)/4) (I2); true iff it is a root of a.  0 ↦ 0, true.
P29_HD bool pk_sqrt_fq(const fe9& a, fe9* root)
{
  *root = f29::mul(a, pk_pow_e(a));
  return pk_eq(f29::sqr(*root), a);
}

// a I2 per component.  *root I2; true iff root² = a.  The header has the method.
P29_HD bool pk_sqrt_fq2(const F2& a, F2* root)
{
  const bool a1_zero = pk_is_zero(a.c1);
  const fe9 n = p29::lt2(f29::add(f29::sqr(a.c0), f29::sqr(a.c1))); // limbs < 2^30, < 2.1p → I2
  fe9 s;
  (void)pk_sqrt_fq(n, &s); // (no root: s is nonsense and the last comparison refuses)
  const fe9 delta = pk_select(a1_zero, a.c0, f29::mul(p29::lt2(f29::add(a.c0, s)), p29::two_inv()));
  const fe9 t = pk_pow_e(delta);
  const fe9 x0 = f29::mul(delta, t);
  const bool residue = pk_eq(f29::sqr(x0), delta);
  const fe9 h = f29::mul(f29::mul(a.c1, t), p29::two_inv());
  const fe9 nh = p29::fq_neg(h);
  root->c0 = pk_select(residue, x0, nh);
  root->c1 = pk_select(residue, h, x0);
  const F2 sq = p29::f2_sqr(*root);
  return pk_eq(sq.c0, a.c0) && pk_eq(sq.c1, a.c1);
}

// the sign of a lazy Montgomery-261 value (N, < 2p): its standard-form integer against (q − 1)/2
FF_HD bool pk_sign_fq(const fe9& y)
{
  constexpr uint32_t HALF[9] = {0xc3e7ea3u, 0x1082305bu, 0xe3951a7u, 0x16a9168u, 0xac2ecbcu, 0x116da060u, 0x5370a0u, 0x72e131au, 0x183227u}; // (q − 1)/2
  const fe9 s = f29::canon(f29::mul(y, f29::one_std()));
  bool gt = false; // s > HALF, from the lowest limb up: a higher limb that differs overrides
  for (int j = 0; j < 9; j++) gt = s.l[j] > HALF[j] || (s.l[j] == HALF[j] && gt);
  return gt;
}
FF_HD bool pk_sign_fq2(const F2& y) { return pk_sign_fq(pk_select(pk_is_zero(y.c1), y.c0, y.c1)); }

// file-form points that classify_g1 / classify_g2 have passed (canonical words)
P29_HD bool pk_sign_g1(const fe mont[2]) { return pk_sign_fq(f29::from_mont256(mont[1])); }
P29_HD bool pk_sign_g2(const fe2 mont[2]) { return pk_sign_fq2(Fq2_29::load_mont256(mont[1])); }

FF_HD fe pk_zero_word()
{
  fe w;
  for (int i = 0; i < 8; i++) w.l[i] = 0;
  return w;
}
P29_HD void pk_pack_g1(const fe mont[2], fe* word)
{
  *word = mont[0];
  if (p29::mont_is_zero(mont[0]) && p29::mont_is_zero(mont[1])) word->l[7] = PK_IDENTITY_BIT;
  else if (pk_sign_g1(mont)) word->l[7] |= PK_SIGN_BIT;
}
P29_HD void pk_pack_g2(const fe2 mont[2], fe2* word)
{
  *word = mont[0];
  if (p29::mont_is_zero(mont[0].c0) && p29::mont_is_zero(mont[0].c1) && p29::mont_is_zero(mont[1].c0) && p29::mont_is_zero(mont[1].c1)) word->c1.l[7] = PK_IDENTITY_BIT;
  else if (pk_sign_g2(mont)) word->c1.l[7] |= PK_SIGN_BIT;
}

P29_HD int pk_unpack_g1(const fe& word, fe mont[2])
{
  const bool sign = (word.l[7] & PK_SIGN_BIT) != 0;
  fe x = word;
  x.l[7] &= ~(PK_SIGN_BIT | PK_IDENTITY_BIT);
  if (word.l[7] & PK_IDENTITY_BIT) {
    if (sign || !p29::mont_is_zero(x)) return p29::ZK_NONCANONICAL;
    mont[0] = mont[1] = pk_zero_word();
    return p29::ZK_SOUND;
  }
  if (!Fq::is_canonical(x)) return p29::ZK_NONCANONICAL;
  const fe9 X = f29::from_mont256(x);
  const fe9 three = f29::add(f29::dbl(f29::one_m()), f29::one_m());               // limbs < 3·2^29, < 3p
  const fe9 rhs = p29::lt2(f29::add(f29::mul(f29::sqr(X), X), three));            // limbs < 2^31, < 4.1p → I2
  fe9 y;
  if (!pk_sqrt_fq(rhs, &y)) return p29::ZK_OFF_CURVE;
  if (pk_is_zero(y) && sign) return p29::ZK_NONCANONICAL;
  y = pk_select(pk_sign_fq(y) != sign, p29::fq_neg(y), y);
  mont[0] = x;
  mont[1] = f29::to_mont256(y);
  return p29::ZK_SOUND;
}

P29_HD int pk_unpack_g2(const fe2& word, fe2 mont[2])
{
  const bool sign = (word.c1.l[7] & PK_SIGN_BIT) != 0;
  fe2 x = word;
  x.c1.l[7] &= ~(PK_SIGN_BIT | PK_IDENTITY_BIT);
  if (word.c1.l[7] & PK_IDENTITY_BIT) {
    if (sign || !p29::mont_is_zero(x.c0) || !p29::mont_is_zero(x.c1)) return p29::ZK_NONCANONICAL;
    mont[0].c0 = mont[0].c1 = mont[1].c0 = mont[1].c1 = pk_zero_word();
    return p29::ZK_SOUND;
  }
  if (!Fq::is_canonical(x.c0) || !Fq::is_canonical(x.c1)) return p29::ZK_NONCANONICAL;
  const F2 X = Fq2_29::load_mont256(x);
  const F2 rhs = p29::f2_add(p29::f2_mul(p29::f2_sqr(X), X), p29::b_twist());
  F2 y;
  if (!pk_sqrt_fq2(rhs, &y)) return p29::ZK_OFF_CURVE;
  if (pk_is_zero(y.c0) && pk_is_zero(y.c1) && sign) return p29::ZK_NONCANONICAL;
  const bool flip = pk_sign_fq2(y) != sign;
  y = {pk_select(flip, p29::fq_neg(y.c0), y.c0), pk_select(flip, p29::fq_neg(y.c1), y.c1)};
  if (!p29::g2_in_subgroup_fast(X, y)) return p29::ZK_OFF_SUBGROUP;
  mont[0] = x;
  mont[1] = Fq2_29::store_mont256(y);
  return p29::ZK_SOUND;
}

} // namespace pk29
} // namespace bn254
