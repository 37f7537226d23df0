// pairing29.h — BN254 optimal-ate pairing on the lazy radix-2^29 field (ff29.h / ec29.h), host and device.
//
// The same algorithm, tower and basis as the host pairing (prover/pairing.cpp): Fq2 = Fq[u]/(u²+1),
// Fq6 = Fq2[v]/(v³−ξ), Fq12 = Fq6[w]/(w²−v), ξ = 9+u; the Miller loop over the signed digits of 6x+2 with D-twist
// lines in homogeneous projective coordinates, the two Frobenius correction steps, and the final exponentiation
// (easy part, then the Fuentes-Castañeda–Knapp–Rodríguez-Henríquez hard part).  Every intermediate is the same field
// element as on the host, so canonical outputs agree bit for bit (tests/test_pairing29.py).  Used by the batched
// verifier (prover/verify_batch.hip): one lane per pairing / per proof.
//
// BOUNDS.  One invariant for every stored Fq2 / Fq6 / Fq12 coefficient ("I2"):  limbs N (l[0..7] < 2^29),
// value < 2·p, Montgomery form with R' = 2^261.  Every operation below takes I2 inputs and returns I2 outputs:
//   mul        Fq2_29::mul (ec29.h): a I2, b I2 → per component a0·b0 + a1·(3p − b1): 2·2 + 2·3 = 10 p² < 147 p²;
//              columns 9·(2^58 + 2^59) + 9·2^58 + 2^35 < 2^64                                   → N, < 1.07·p
//   sqr        Fq2_29::sqr_n: needs components N, < 5p (I2 is tighter)                        → N, < 2p
//   mul_fq     two f29::mul of I2 operands (4 p²)                                              → N, < 1.03·p
//   add / dbl  limb-wise: limbs < 2^30, value < 4p  → lt2 (norm + two conditional subtractions) → I2
//   sub        a + 3p − b (sub<3,1>: b N, b_8 ≤ (2p)_8 ≤ (3p)_8 − 1): limbs < 2^29 + 2^30, < 5p → lt2 → I2
//   neg        3p − b (neg<3,1>, same condition on b): < 3p                                   → lt2 → I2
//   inv        f29::inv_ds takes N, < 16p and returns N, < 2p
// lt2 = f29::reduce_lt2p(f29::norm(·)) needs limbs < 2^32 − 2^3 and value < 8p; both hold above with room.  Only the
// Fq2 level reduces: Fq6 / Fq12 formulas are compositions of the Fq2 operations and inherit the invariant.
// `F29_CHECK` host builds assert every column, limb and value condition (tests/pairing29_check.cpp).
#pragma once
#include "ec29.h"

#if defined(__HIPCC__)
#define P29_HD __host__ __device__ inline
#else
#define P29_HD inline
#endif

namespace bn254 {
namespace p29 {

typedef fe9x2 F2;
struct F6 {
  F2 c0, c1, c2;
};
struct F12 {
  F6 c0, c1;
};
struct Line { // evaluated at P as  a·y_P + b·x_P·w + c·v·w  (sparse Fq12: slots c0.c0, c1.c0, c1.c1)
  F2 a, b, c;
};
struct G2P { // homogeneous projective point on the twist
  F2 X, Y, Z;
};

// ---- constants (Montgomery-261, N, canonical; generated with Python big integers, checked through the pairing
// results by tests/test_pairing29.py) -----------------------------------------------------------------------------------
#define P29_F2(name, ...)                                                                                              \
  FF_HD F2 name()                                                                                                      \
  {                                                                                                                    \
    constexpr uint32_t c[18] = {__VA_ARGS__};                                                                          \
    F2 r;                                                                                                              \
    for (int i = 0; i < 9; i++) {                                                                                      \
      r.c0.l[i] = c[i];                                                                                                \
      r.c1.l[i] = c[9 + i];                                                                                            \
    }                                                                                                                  \
    return r;                                                                                                          \
  }
// Frobenius coefficients: g1_k = ξ^(k(p−1)/6), g2_k = ξ^(k(p²−1)/6), g3_k = ξ^(k(p³−1)/6)
P29_F2(g1_1, 0xa0c2399u, 0x1aa2357cu, 0x149b22du, 0x487bf1bu, 0xb89bb5eu, 0x1313c7e1u, 0x1d61fdb5u, 0x60c56b5u, 0x2e0560u, 0x1bc6cc33u, 0x177dfb71u, 0x161dd8abu, 0x180969du, 0x58d47f5u, 0x1ab975b5u, 0x1c26a2du, 0x1cd88219u, 0x9b83u)
P29_F2(g1_2, 0x4a59190u, 0x6f504d9u, 0xbf870bbu, 0x171ffd5cu, 0x1ac4d17du, 0x4be36d5u, 0xbceec27u, 0x1a83a513u, 0x2492b3u, 0x11142ef1u, 0xb31acc7u, 0x1d5818bcu, 0x180afc17u, 0x1a63177eu, 0x15765b3bu, 0x118f742eu, 0x63a509au, 0x135e4eu)
P29_F2(g1_3, 0x1b1f0678u, 0x373fb06u, 0x13170fbdu, 0x185d74b7u, 0x241131fu, 0x16e18435u, 0x1ef3b6ceu, 0x1f06f02u, 0x1d46bdu, 0x19a647d5u, 0x19fdefabu, 0x1d925d1au, 0xd1f6c5fu, 0x8ac6cc5u, 0x1fa5621au, 0x134f06feu, 0x9a72816u, 0x15871du)
P29_F2(g1_4, 0x1081f85eu, 0x139a3585u, 0x124aed48u, 0x34ce260u, 0x19e166e5u, 0xb172958u, 0xd2df880u, 0xde46877u, 0x167751u, 0xf616a78u, 0x5940429u, 0x181bb386u, 0x66e257bu, 0xe66254u, 0xc12b5cdu, 0xef6c029u, 0x1c2232e3u, 0x6f9f8u)
P29_F2(g1_5, 0x7461d8cu, 0x434a6b0u, 0x14f8b697u, 0xb0aa80fu, 0x118b92dfu, 0x471333du, 0x18c6d066u, 0x7d8f7b0u, 0x10a3f0u, 0x1eb54987u, 0x8d56d1eu, 0xc80f1d8u, 0x1536f380u, 0x6b4b4a7u, 0x82bcd3cu, 0x19349170u, 0x17aea9fcu, 0x817f6u)
P29_F2(g2_1, 0xe4983b2u, 0xb774393u, 0x3d607b6u, 0xfdad48bu, 0x1d262e9bu, 0x1644f52u, 0x11b94d87u, 0x1a3314f3u, 0x24594fu, 0, 0, 0, 0, 0, 0, 0, 0, 0)
P29_F2(g2_2, 0x18ccb791u, 0x175b1c3au, 0xb83d6e2u, 0xe8ed071u, 0x1282bee2u, 0x4220e84u, 0x1fe4017fu, 0x15084d4au, 0x169119u, 0, 0, 0, 0, 0, 0, 0, 0, 0)
P29_F2(g2_3, 0x3003126u, 0xce8395eu, 0x420727bu, 0x1891eb7u, 0xae269bfu, 0x598fff2u, 0xed19539u, 0x9315e8bu, 0x229c18u, 0, 0, 0, 0, 0, 0, 0, 0, 0)
P29_F2(g2_4, 0xa337995u, 0x158d1d23u, 0x189c9b98u, 0x12fa4e45u, 0x185faadcu, 0x176f16du, 0xeed93bau, 0x14291140u, 0xc0afeu, 0, 0, 0, 0, 0, 0, 0, 0, 0)
P29_F2(g2_5, 0x1fb045b6u, 0x9a9447bu, 0x10eecc6cu, 0x1446525fu, 0x3031a95u, 0x1eb9323cu, 0xc2dfc1u, 0x1953d8e9u, 0x19d334u, 0, 0, 0, 0, 0, 0, 0, 0, 0)
P29_F2(g3_1, 0xe6a3d3du, 0xe0034bcu, 0x1d2fc927u, 0x167e071du, 0x7ccd695u, 0x4b45d3du, 0xe70688eu, 0x1e41c930u, 0x103828u, 0xf4e6b31u, 0x5dd85eau, 0x16ca0ad7u, 0x19d17c36u, 0x1bae3e83u, 0x1bf781fu, 0x30191b5u, 0x10c0063eu, 0x133cf9u)
P29_F2(g3_2, 0x136caecdu, 0x19c70818u, 0x1dae30d1u, 0x28eb786u, 0xbee8f49u, 0x1a51d4beu, 0x135c7d00u, 0x11fdec39u, 0xcad5fu, 0x6e485d6u, 0x1a0e1cafu, 0x10aa918bu, 0x4618e04u, 0x7ab5997u, 0x1790c244u, 0x6cbab85u, 0x1ee779f9u, 0x266696u)
P29_F2(g3_3, 0x1d5df6cfu, 0x1d9065afu, 0x95b9391u, 0xa77ae19u, 0x1344c658u, 0xbf9bc8bu, 0x1b32a72u, 0xc6bb731u, 0x131d91u, 0x1ed6b572u, 0x706710au, 0x1ee04634u, 0x15b5b670u, 0xcd96cb2u, 0x335dea6u, 0xd57da42u, 0x4b4fe1du, 0x1add31u)
P29_F2(g3_4, 0xaf866c4u, 0x68222a0u, 0x1d8c6ce8u, 0x28befbu, 0x12de19ccu, 0x1193e6bau, 0x9d0a776u, 0x1b6142e1u, 0x14766fu, 0x9d402f7u, 0xa994a07u, 0x169567b7u, 0x9218b7fu, 0x1b0b8541u, 0x32ce2a0u, 0xf936727u, 0x16ad3976u, 0xbaf8cu)
P29_F2(g3_5, 0x314d9feu, 0xe0dd877u, 0x18eb90b3u, 0x6a988e8u, 0xd6b9fe0u, 0x25b9f1eu, 0x161fcb32u, 0xed57bb5u, 0x14445bu, 0x1b3b7638u, 0x1086ac9cu, 0x57c4a00u, 0x1b93c320u, 0x22ad2d0u, 0xcace295u, 0x226f886u, 0xee880a1u, 0x12c9d7u)
P29_F2(b_twist, 0xb489658u, 0xcfd255u, 0xfdb9a77u, 0x2ce89f7u, 0x33a0d4u, 0x1a768545u, 0x6ee3ddcu, 0x106a7dc1u, 0x19316bu, 0x1b9fece0u, 0x7ecccd1u, 0x1069f1c7u, 0xcdf64f3u, 0x154cbe1u, 0xdd22ac0u, 0x6eba4e8u, 0x1929a235u, 0x283739u) // 3/ξ
P29_F2(xi, 0x1069329bu, 0x12f4a0b0u, 0x1fe70d2u, 0x601df46u, 0x14b33a91u, 0x19dc5bfu, 0x1f31e9c5u, 0x11c8b884u, 0x1b414au, F29_ONE_M) // 9 + u
F29_CONST(two_inv, 0x16fce4b4u, 0xa904407u, 0xa626a11u, 0x12109375u, 0x1014a498u, 0x100ec0c7u, 0x93e16a4u, 0x9c376eeu, 0x1f1642u) // 1/2
#undef P29_F2

// signed digits (NAF), little endian: 6x+2 (66 digits) and x (63 digits), x = 4965661367192848881
constexpr int ATE_LEN = 66;
constexpr signed char ATE[ATE_LEN] = {0, 0, 0, 1, 0, 1, 0, -1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, -1, 0, 0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0,
                                      1, 0, -1, 0, 0, 1, 0, 0, 0, 0, 0, -1, 0, 0, -1, 0, 1, 0, -1, 0, 0, 0, -1, 0, -1, 0, 0, 0, 1, 0, -1, 0, 1};
constexpr int X_LEN = 63;
constexpr signed char XNAF[X_LEN] = {1, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1, 0, -1, 0, 1, 0, 1, 0, 1, 0, 0, 1, 0,
                                     0, 0, 1, 0, -1, 0, -1, 0, -1, 0, 1, 0, 1, 0, 0, -1, 0, 1, 0, 1, 0, -1, 0, 0, 1, 0, 1, 0, 0, 0, 1};
// lines of one Miller loop: a doubling line per step i = ATE_LEN−2 … 0, an addition line per non-zero digit, two corrections
constexpr int count_lines()
{
  int n = 2;
  for (int i = ATE_LEN - 2; i >= 0; i--) n += ATE[i] ? 2 : 1;
  return n;
}
constexpr int N_LINES = count_lines();

// ---- Fq2 (invariant I2 in and out, see the header) ----------------------------------------------------------------------
FF_HD fe9 lt2(const fe9& a) { return f29::reduce_lt2p(f29::norm(a)); }
FF_HD F2 f2_zero() { return Fq2_29::zero(); }
FF_HD F2 f2_one() { return Fq2_29::one(); }
FF_HD F2 f2_add(const F2& a, const F2& b) { return {lt2(f29::add(a.c0, b.c0)), lt2(f29::add(a.c1, b.c1))}; }
FF_HD F2 f2_dbl(const F2& a) { return {lt2(f29::dbl(a.c0)), lt2(f29::dbl(a.c1))}; }
FF_HD F2 f2_sub(const F2& a, const F2& b) { return {lt2(f29::sub<3, 1>(a.c0, b.c0)), lt2(f29::sub<3, 1>(a.c1, b.c1))}; }
FF_HD fe9 fq_neg(const fe9& a) { return lt2(f29::neg<3, 1>(a)); }
FF_HD F2 f2_neg(const F2& a) { return {fq_neg(a.c0), fq_neg(a.c1)}; }
FF_HD F2 f2_conj(const F2& a) { return {a.c0, fq_neg(a.c1)}; }
FF_HD F2 f2_mul(const F2& a, const F2& b) { return Fq2_29::mul(a, b); }
FF_HD F2 f2_sqr(const F2& a) { return Fq2_29::sqr_n(a); }
FF_HD F2 f2_mul_fq(const F2& a, const fe9& s) { return {f29::mul(a.c0, s), f29::mul(a.c1, s)}; }
FF_HD F2 f2_mul_xi(const F2& a) { return f2_mul(a, xi()); }
FF_HD F2 f2_triple(const F2& a) { return f2_add(f2_dbl(a), a); }
P29_HD F2 f2_inv(const F2& a) // (a0 − a1·u) / (a0² + a1²)
{
  const fe9 t = f29::inv_ds(f29::norm(f29::add(f29::sqr(a.c0), f29::sqr(a.c1)))); // N, < 4p in; N, < 2p out
  return {f29::mul(a.c0, t), f29::mul(f29::neg<3, 1>(a.c1), t)};               // (3p − a1 < 3p, limbs < 2^30): 6 p²
}
FF_HD fe9 fq_canon(const fe9& a) { return f29::canon(a); }
FF_HD F2 f2_canon(const F2& a) { return {f29::canon(a.c0), f29::canon(a.c1)}; }

// ---- Fq6 -------------------------------------------------------------------------------------------------------------------
FF_HD F6 f6_add(const F6& a, const F6& b) { return {f2_add(a.c0, b.c0), f2_add(a.c1, b.c1), f2_add(a.c2, b.c2)}; }
FF_HD F6 f6_sub(const F6& a, const F6& b) { return {f2_sub(a.c0, b.c0), f2_sub(a.c1, b.c1), f2_sub(a.c2, b.c2)}; }
FF_HD F6 f6_neg(const F6& a) { return {f2_neg(a.c0), f2_neg(a.c1), f2_neg(a.c2)}; }
FF_HD F6 f6_mul_v(const F6& a) { return {f2_mul_xi(a.c2), a.c0, a.c1}; } // × v
P29_HD F6 f6_mul(const F6& a, const F6& b) // Karatsuba, as pairing.cpp
{
  const F2 v0 = f2_mul(a.c0, b.c0), v1 = f2_mul(a.c1, b.c1), v2 = f2_mul(a.c2, b.c2);
  const F2 t0 = f2_sub(f2_sub(f2_mul(f2_add(a.c1, a.c2), f2_add(b.c1, b.c2)), v1), v2);
  const F2 t1 = f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c1), f2_add(b.c0, b.c1)), v0), v1);
  const F2 t2 = f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c2), f2_add(b.c0, b.c2)), v0), v2);
  return {f2_add(v0, f2_mul_xi(t0)), f2_add(t1, f2_mul_xi(v2)), f2_add(t2, v1)};
}
// a · (B + C·v):  (a0·B + ξ·a2·C) + (a0·C + a1·B)·v + (a1·C + a2·B)·v²
P29_HD F6 f6_mul_01(const F6& a, const F2& B, const F2& C)
{
  return {f2_add(f2_mul(a.c0, B), f2_mul_xi(f2_mul(a.c2, C))), f2_add(f2_mul(a.c0, C), f2_mul(a.c1, B)),
          f2_add(f2_mul(a.c1, C), f2_mul(a.c2, B))};
}
FF_HD F6 f6_mul_f2(const F6& a, const F2& s) { return {f2_mul(a.c0, s), f2_mul(a.c1, s), f2_mul(a.c2, s)}; }
P29_HD F6 f6_inv(const F6& a)
{
  const F2 c0 = f2_sub(f2_sqr(a.c0), f2_mul_xi(f2_mul(a.c1, a.c2)));
  const F2 c1 = f2_sub(f2_mul_xi(f2_sqr(a.c2)), f2_mul(a.c0, a.c1));
  const F2 c2 = f2_sub(f2_sqr(a.c1), f2_mul(a.c0, a.c2));
  const F2 t = f2_add(f2_mul_xi(f2_add(f2_mul(a.c2, c1), f2_mul(a.c1, c2))), f2_mul(a.c0, c0));
  const F2 ti = f2_inv(t);
  return {f2_mul(c0, ti), f2_mul(c1, ti), f2_mul(c2, ti)};
}

// ---- Fq12 ------------------------------------------------------------------------------------------------------------------
FF_HD F12 f12_one() { return {{f2_one(), f2_zero(), f2_zero()}, {f2_zero(), f2_zero(), f2_zero()}}; }
P29_HD F12 f12_mul(const F12& a, const F12& b)
{
  const F6 v0 = f6_mul(a.c0, b.c0), v1 = f6_mul(a.c1, b.c1);
  const F6 c1 = f6_sub(f6_sub(f6_mul(f6_add(a.c0, a.c1), f6_add(b.c0, b.c1)), v0), v1);
  return {f6_add(v0, f6_mul_v(v1)), c1};
}
P29_HD F12 f12_sqr(const F12& a) // complex squaring: (a0+a1)(a0+v·a1) − a0a1 − v·a0a1  +  2·a0a1·w
{
  const F6 ab = f6_mul(a.c0, a.c1);
  const F6 t = f6_mul(f6_add(a.c0, a.c1), f6_add(a.c0, f6_mul_v(a.c1)));
  return {f6_sub(f6_sub(t, ab), f6_mul_v(ab)), f6_add(ab, ab)};
}
FF_HD F12 f12_conj(const F12& a) { return {a.c0, f6_neg(a.c1)}; } // a^(p^6)
P29_HD F12 f12_inv(const F12& a)
{
  const F6 t = f6_sub(f6_mul(a.c0, a.c0), f6_mul_v(f6_mul(a.c1, a.c1)));
  const F6 ti = f6_inv(t);
  return {f6_mul(a.c0, ti), f6_neg(f6_mul(a.c1, ti))};
}
// f · (A + B·w + C·v·w), the sparse product of a line (slots c0.c0 = A, c1.c0 = B, c1.c1 = C): 15 Fq2 products, not 18
P29_HD F12 f12_mul_sparse(const F12& f, const F2& A, const F2& B, const F2& C)
{
  const F6 v0 = f6_mul_f2(f.c0, A);
  const F6 v1 = f6_mul_01(f.c1, B, C);
  const F6 c1 = f6_sub(f6_sub(f6_mul_01(f6_add(f.c0, f.c1), f2_add(A, B), C), v0), v1);
  return {f6_add(v0, f6_mul_v(v1)), c1};
}
// Frobenius^k, k = 1, 2, 3: the coefficient of ω^m (ω = w, v = ω², ω⁶ = ξ) is conjugated k times and scaled by ξ^(m(p^k−1)/6)
P29_HD F12 f12_frob(const F12& a, int k)
{
  auto fr = [k](const F2& x) { return (k & 1) ? f2_conj(x) : x; };
  F2 g[6];
  if (k == 1) { g[1] = g1_1(); g[2] = g1_2(); g[3] = g1_3(); g[4] = g1_4(); g[5] = g1_5(); }
  else if (k == 2) { g[1] = g2_1(); g[2] = g2_2(); g[3] = g2_3(); g[4] = g2_4(); g[5] = g2_5(); }
  else { g[1] = g3_1(); g[2] = g3_2(); g[3] = g3_3(); g[4] = g3_4(); g[5] = g3_5(); }
  F12 r;
  r.c0.c0 = fr(a.c0.c0);
  r.c0.c1 = f2_mul(fr(a.c0.c1), g[2]);
  r.c0.c2 = f2_mul(fr(a.c0.c2), g[4]);
  r.c1.c0 = f2_mul(fr(a.c1.c0), g[1]);
  r.c1.c1 = f2_mul(fr(a.c1.c1), g[3]);
  r.c1.c2 = f2_mul(fr(a.c1.c2), g[5]);
  return r;
}
P29_HD F12 f12_exp_x(const F12& f) // f^x for f in the cyclotomic subgroup (inverse = conjugate); XNAF's top digit is 1
{
  const F12 finv = f12_conj(f);
  F12 res = f;
  for (int i = X_LEN - 2; i >= 0; i--) {
    res = f12_sqr(res);
    if (XNAF[i] > 0) res = f12_mul(res, f);
    else if (XNAF[i] < 0) res = f12_mul(res, finv);
  }
  return res;
}
P29_HD bool f12_eq_canon(const F12& a, const F12& b) // a, b I2: compares canonical representatives
{
  const fe9* x = reinterpret_cast<const fe9*>(&a);
  const fe9* y = reinterpret_cast<const fe9*>(&b);
  bool eq = true;
  for (int i = 0; i < 12; i++) {
    const fe9 cx = f29::canon(x[i]), cy = f29::canon(y[i]);
    for (int j = 0; j < 9; j++) eq = eq && cx.l[j] == cy.l[j];
  }
  return eq;
}
P29_HD F12 f12_canon(const F12& a)
{
  F12 r;
  const fe9* x = reinterpret_cast<const fe9*>(&a);
  fe9* y = reinterpret_cast<fe9*>(&r);
  for (int i = 0; i < 12; i++) y[i] = f29::canon(x[i]);
  return r;
}
// 12 standard-form canonical coefficients (bn254_fq12_t layout) ↔ lazy
P29_HD void f12_store_std(const F12& a, fe* out)
{
  const fe9* x = reinterpret_cast<const fe9*>(&a);
  for (int i = 0; i < 12; i++) out[i] = f29::pack(f29::canon(f29::mul(x[i], f29::one_std())));
}

// ---- final exponentiation: f^((p^12 − 1)/r) ---------------------------------------------------------------------------------
P29_HD F12 final_exp(const F12& f)
{
  // easy part f^((p⁶−1)(p²+1))
  F12 r = f12_mul(f12_conj(f), f12_inv(f));
  r = f12_mul(f12_frob(r, 2), r);
  // hard part (Fuentes-Castañeda et al.), exponent a multiple of (p⁴ − p² + 1)/r — step for step as pairing.cpp
  const F12 y0 = f12_conj(f12_exp_x(r)); // r^(−x)
  const F12 y1 = f12_sqr(y0);
  const F12 y2 = f12_sqr(y1);
  F12 y3 = f12_mul(y2, y1);
  const F12 y4 = f12_conj(f12_exp_x(y3));
  const F12 y5 = f12_sqr(y4);
  F12 y6 = f12_conj(f12_exp_x(y5));
  y3 = f12_conj(y3);
  y6 = f12_conj(y6);
  const F12 y7 = f12_mul(y6, y4);
  const F12 y8 = f12_mul(y7, y3);
  const F12 y9 = f12_mul(y8, y1);
  const F12 y10 = f12_mul(y8, y4);
  const F12 y11 = f12_mul(y10, r);
  const F12 y12 = f12_frob(y9, 1);
  const F12 y13 = f12_mul(y12, y11);
  const F12 y14 = f12_mul(f12_frob(y8, 2), y13);
  const F12 y15 = f12_frob(f12_mul(f12_conj(r), y9), 3);
  return f12_mul(y15, y14);
}

// ---- D-twist lines (homogeneous projective, as pairing.cpp line_double / line_add) --------------------------------------
P29_HD Line line_double(G2P& R)
{
  const fe9 h2 = two_inv();
  const F2 a = f2_mul_fq(f2_mul(R.X, R.Y), h2);
  const F2 b = f2_sqr(R.Y), c = f2_sqr(R.Z);
  const F2 e = f2_mul(b_twist(), f2_triple(c));
  const F2 f = f2_triple(e);
  const F2 g = f2_mul_fq(f2_add(b, f), h2);
  const F2 h = f2_sub(f2_sqr(f2_add(R.Y, R.Z)), f2_add(b, c));
  const F2 i = f2_sub(e, b);
  const F2 j = f2_sqr(R.X);
  const F2 e2 = f2_sqr(e);
  R.X = f2_mul(a, f2_sub(b, f));
  R.Y = f2_sub(f2_sqr(g), f2_triple(e2));
  R.Z = f2_mul(b, h);
  return {f2_neg(h), f2_triple(j), i};
}
P29_HD Line line_add(G2P& R, const F2& qx, const F2& qy)
{
  const F2 theta = f2_sub(R.Y, f2_mul(qy, R.Z));
  const F2 lambda = f2_sub(R.X, f2_mul(qx, R.Z));
  const F2 c = f2_sqr(theta), d = f2_sqr(lambda);
  const F2 e = f2_mul(lambda, d), f = f2_mul(R.Z, c), g = f2_mul(R.X, d);
  const F2 h = f2_sub(f2_add(e, f), f2_dbl(g));
  R.X = f2_mul(lambda, h);
  R.Y = f2_sub(f2_mul(theta, f2_sub(g, h)), f2_mul(e, R.Y));
  R.Z = f2_mul(R.Z, e);
  const F2 j = f2_sub(f2_mul(theta, qx), f2_mul(lambda, qy));
  return {lambda, f2_neg(theta), j};
}
// f ← f · (a·y_P + b·x_P·w + c·v·w)
P29_HD void mul_line(F12& f, const Line& l, const fe9& px, const fe9& py) { f = f12_mul_sparse(f, f2_mul_fq(l.a, py), f2_mul_fq(l.b, px), l.c); }
// Q1 = π(Q), Q2 = −π²(Q) of the two correction steps
P29_HD void frob_points(const F2& qx, const F2& qy, F2& q1x, F2& q1y, F2& q2x, F2& q2y)
{
  q1x = f2_mul(f2_conj(qx), g1_2());
  q1y = f2_mul(f2_conj(qy), g1_3());
  q2x = f2_mul(f2_conj(q1x), g1_2());
  q2y = f2_neg(f2_mul(f2_conj(q1y), g1_3()));
}

// All N_LINES lines of Q's Miller loop, in the order the loop consumes them (the fixed γ₂ / δ₂ of a verification key)
P29_HD void precompute_lines(const F2& qx, const F2& qy, Line* out)
{
  G2P R = {qx, qy, f2_one()};
  const F2 nqy = f2_neg(qy);
  int k = 0;
  for (int i = ATE_LEN - 2; i >= 0; i--) {
    out[k++] = line_double(R);
    if (ATE[i] == 1) out[k++] = line_add(R, qx, qy);
    else if (ATE[i] == -1) out[k++] = line_add(R, qx, nqy);
  }
  F2 q1x, q1y, q2x, q2y;
  frob_points(qx, qy, q1x, q1y, q2x, q2y);
  out[k++] = line_add(R, q1x, q1y);
  out[k++] = line_add(R, q2x, q2y);
}

// Miller loop of e(P0, Q0)·e(P1, ·)·e(P2, ·): Q0's lines are computed on the way, pairs 1 and 2 read theirs from tables made
// by precompute_lines; one shared Fq12 squaring per step.  A pair whose flag is false contributes 1 (an identity input).
// P coordinates and Q0 I2.
P29_HD F12 multi_miller(bool use0, const fe9& p0x, const fe9& p0y, const F2& q0x, const F2& q0y, bool use1, const fe9& p1x,
                        const fe9& p1y, const Line* L1, bool use2, const fe9& p2x, const fe9& p2y, const Line* L2)
{
  G2P R = {q0x, q0y, f2_one()};
  const F2 nqy = f2_neg(q0y);
  F12 f = f12_one();
  int k = 0;
  for (int i = ATE_LEN - 2; i >= 0; i--) {
    if (i != ATE_LEN - 2) f = f12_sqr(f); // f = 1 before the first step
    if (use0) mul_line(f, line_double(R), p0x, p0y);
    if (use1) mul_line(f, L1[k], p1x, p1y);
    if (use2) mul_line(f, L2[k], p2x, p2y);
    k++;
    if (ATE[i]) {
      if (use0) mul_line(f, line_add(R, q0x, ATE[i] > 0 ? q0y : nqy), p0x, p0y);
      if (use1) mul_line(f, L1[k], p1x, p1y);
      if (use2) mul_line(f, L2[k], p2x, p2y);
      k++;
    }
  }
  if (use0) {
    F2 q1x, q1y, q2x, q2y;
    frob_points(q0x, q0y, q1x, q1y, q2x, q2y);
    mul_line(f, line_add(R, q1x, q1y), p0x, p0y);
    mul_line(f, line_add(R, q2x, q2y), p0x, p0y);
  }
  for (int t = 0; t < 2; t++, k++) {
    if (use1) mul_line(f, L1[k], p1x, p1y);
    if (use2) mul_line(f, L2[k], p2x, p2y);
  }
  return f;
}

// e(P, Q) for P, Q not the identity (I2 affine coordinates)
P29_HD F12 pairing(const fe9& px, const fe9& py, const F2& qx, const F2& qy)
{
  return final_exp(multi_miller(true, px, py, qx, qy, false, px, py, nullptr, false, px, py, nullptr));
}

// ---- group checks / public input of the verifier ------------------------------------------------------------------------------
// [r]·Q = O for an affine twist point Q (I2, not the identity): XYZZ double-and-add over the 254 bits of r (ec29.h), the same
// test as the host's g2_valid (plain [r]·Q, no endomorphism shortcut)
P29_HD bool g2_in_subgroup(const F2& qx, const F2& qy)
{
  const G2L::A q = {qx, qy};
  G2L::X acc = G2L::x_zero();
  for (int i = 253; i >= 0; i--) {
    acc = G2L::x_dbl(acc);
    if ((FrP::MOD[i >> 5] >> (i & 31)) & 1u) G2L::x_madd(acc, q);
  }
  return G2L::x_is_zero(acc);
}
// y² = x³ + 3/ξ on the twist (I2 coordinates)
P29_HD bool g2_on_twist(const F2& x, const F2& y)
{
  const F2 l = f2_canon(f2_sqr(y)), r = f2_canon(f2_add(f2_mul(f2_sqr(x), x), b_twist()));
  bool eq = true;
  for (int j = 0; j < 9; j++) eq = eq && l.c0.l[j] == r.c0.l[j] && l.c1.l[j] == r.c1.l[j];
  return eq;
}
// XYZZ (ec29.h G1 bounds: X N < 7p, others N < 2p), not the identity → affine I2 with one inversion: I = (ZZ·ZZZ)⁻¹,
// x = X·I·ZZZ, y = Y·I·ZZ
P29_HD void g1_to_affine(const G1L::X& p, fe9& x, fe9& y)
{
  const fe9 I = f29::inv_ds(f29::mul(p.zz, p.zzz));
  x = f29::mul(p.x, f29::mul(I, p.zzz)); // 7·2 p² < 147 p²
  y = f29::mul(p.y, f29::mul(I, p.zz));
}


// cpub = IC₀ + Σ_j s_j·IC_{j+1}: one shared doubling per bit over all public signals (Straus), XYZZ on ec29.h's G1 layer.
// ic: affine I2 (ic_zero marks identities); s_j = sc[j·stride], standard form (< r, checked by the parser).  False: cpub = O.
P29_HD bool public_input(const G1L::A* ic, const uint8_t* ic_zero, int n_pub, const fe* sc, size_t stride, fe9& x, fe9& y)
{
  G1L::X acc = G1L::x_zero();
  for (int i = 253; i >= 0; i--) {
    acc = G1L::x_dbl(acc);
    for (int j = 0; j < n_pub; j++)
      if (!ic_zero[j + 1] && ((sc[(size_t)j * stride].l[i >> 5] >> (i & 31)) & 1u)) G1L::x_madd(acc, ic[j + 1]);
  }
  if (!ic_zero[0]) G1L::x_madd(acc, ic[0]);
  if (G1L::x_is_zero(acc)) return false;
  g1_to_affine(acc, x, y);
  return true;
}

// what one verification key contributes to every proof: γ₂ / δ₂ lines, the target conj(e(α₁, β₂)) (canonical); made by
// make_verify_key below, which prover/verify_host.h (PreparedKey) calls in its two halves
struct VerifyKey29 {
  Line gamma[N_LINES], delta[N_LINES];
  F12 target;
  int use_gamma, use_delta; // 0 when γ₂ / δ₂ is the identity (its pairings are 1)
  int n_pub;
};
FF_HD bool std_is_zero(const fe& a)
{
  uint32_t o = 0;
  for (int i = 0; i < 8; i++) o |= a.l[i];
  return o == 0;
}
// (0, 0), the identity encoding of a standard-form affine point: p = {x, y}
FF_HD bool g1_std_is_zero(const fe* p) { return std_is_zero(p[0]) && std_is_zero(p[1]); }
FF_HD bool g2_std_is_zero(const fe2* q) { return std_is_zero(q[0].c0) && std_is_zero(q[0].c1) && std_is_zero(q[1].c0) && std_is_zero(q[1].c1); }
// one Groth16 proof, points in standard form (canonical, on their curves: the parser checked that; (0, 0) = identity):
//   e(−A, B) · e(cpub, γ₂) · e(C, δ₂) = conj(e(α₁, β₂))
// returns 1 accepted, 0 rejected, −2 when B lies outside the order-r subgroup (the host verifier's code for a bad point)
P29_HD int verify_proof(const VerifyKey29& vk, const G1L::A* ic, const uint8_t* ic_zero, const fe* a, const fe2* b, const fe* c,
                        const fe* sc, size_t stride)
{
  const bool a_zero = g1_std_is_zero(a);
  const bool b_zero = g2_std_is_zero(b);
  const bool c_zero = g1_std_is_zero(c);
  const F2 bx = Fq2_29::load_std(b[0]), by = Fq2_29::load_std(b[1]);
  if (!b_zero && !g2_in_subgroup(bx, by)) return -2;
  fe9 px, py;
  const bool use1 = public_input(ic, ic_zero, vk.n_pub, sc, stride, px, py) && vk.use_gamma;
  const fe9 ax = f29::from_std(a[0]), nay = fq_neg(f29::from_std(a[1]));
  const fe9 cx = f29::from_std(c[0]), cy = f29::from_std(c[1]);
  const F12 f = multi_miller(!a_zero && !b_zero, ax, nay, bx, by, use1, px, py, vk.gamma, !c_zero && vk.use_delta, cx, cy, vk.delta);
  return f12_eq_canon(final_exp(f), vk.target) ? 1 : 0;
}
// the per-key part, on the host (or a single lane): α₁, β₂, γ₂, δ₂ standard form, (0, 0) = identity.  In two halves, because the
// target costs a pairing that only the per-item verifier compares with (prover/verify_host.h: PreparedKey asks for it late).
P29_HD void make_verify_lines(const fe2* gamma, const fe2* delta, int n_pub, VerifyKey29* vk)
{
  vk->use_gamma = !g2_std_is_zero(gamma);
  vk->use_delta = !g2_std_is_zero(delta);
  if (vk->use_gamma) precompute_lines(Fq2_29::load_std(gamma[0]), Fq2_29::load_std(gamma[1]), vk->gamma);
  if (vk->use_delta) precompute_lines(Fq2_29::load_std(delta[0]), Fq2_29::load_std(delta[1]), vk->delta);
  vk->n_pub = n_pub;
}
P29_HD void make_verify_target(const fe* alpha, const fe2* beta, VerifyKey29* vk)
{
  const F12 e = (g1_std_is_zero(alpha) || g2_std_is_zero(beta))
                  ? f12_one()
                  : pairing(f29::from_std(alpha[0]), f29::from_std(alpha[1]), Fq2_29::load_std(beta[0]), Fq2_29::load_std(beta[1]));
  vk->target = f12_canon(f12_conj(e));
}
P29_HD void make_verify_key(const fe* alpha, const fe2* beta, const fe2* gamma, const fe2* delta, int n_pub, VerifyKey29* vk)
{
  make_verify_lines(gamma, delta, n_pub, vk);
  make_verify_target(alpha, beta, vk);
}

// ---- randomised batch verification (prover/verify_combined.hip) ------------------------------------------------------------
// For secret random zᵢ an all-valid batch of one key satisfies
//   Πᵢ e(−zᵢ·Aᵢ, Bᵢ) · e(Σᵢ zᵢ·cpubᵢ, γ₂) · e(Σᵢ zᵢ·Cᵢ, δ₂) · e((Σᵢ zᵢ)·α₁, β₂) = 1
// and a batch with an invalid item fails it except with probability ≤ 2⁻¹²⁷ (128-bit zᵢ ≠ 0).  Per proof that is one subgroup
// test of B, one 128-bit G1 multiplication and one single-pair Miller loop (combined_lane); the Miller values are multiplied
// together and the three fixed-G2 pairs and the one final exponentiation are paid once per batch (combined_accept).

// ψ = twist⁻¹ ∘ Frobenius ∘ twist on an XYZZ twist point: (x, y) ↦ (conj(x)·g1_2, conj(y)·g1_3), frob_points' Q1, applied to
// x = X/ZZ, y = Y/ZZZ — conjugation is a field automorphism, so ZZ and ZZZ are conjugated and nothing else.
// BOUNDS: coordinates I2 in (a G2 XYZZ coordinate is N, < 2p: ec29.h); f2_conj → I2, f2_mul of I2 operands → N, < 1.07p: I2 out.
// The identity (ZZ all zero) is returned untouched: conj(0) would be the non-zero limb pattern of p.
P29_HD G2L::X g2_psi(const G2L::X& p)
{
  if (G2L::x_is_zero(p)) return p;
  return {f2_mul(f2_conj(p.x), g1_2()), f2_mul(f2_conj(p.y), g1_3()), f2_conj(p.zz), f2_conj(p.zzz)};
}
// Q ∈ G2 for an affine twist point Q (I2, on the twist, not the identity), by the endomorphism: accepts iff
//   [x+1]Q + ψ([x]Q) + ψ²([x]Q) = ψ³([2x]Q),      x = 4965661367192848881
// — one 63-bit multiplication (signed digits XNAF, top digit 1) instead of g2_in_subgroup's 254-bit one.  ψ satisfies
// X² − tX + q on the twist and acts as q on G2; P(X) = (x+1) + xX + xX² − 2xX³ has P(q) ≡ 0 mod r, and the norm of P(ψ) in
// Z[ψ] is prime to the cofactor, so the kernel of P(ψ) in E′(F_q²) is exactly G2 (tests/test_pairing29_combined.py does that
// computation with integers).  The right side is 2·ψ(ψ²([x]Q)): ψ is a homomorphism.
// BOUNDS: every point is built by ec29.h's x_dbl / x_madd / x_add (G2: coordinates N, < 2p in and out) and g2_psi (I2 → I2);
// the affine operands ±Q are I2 (f2_neg → I2); the negated Y of the right side is f2_neg of an I2 value → I2.
P29_HD bool g2_in_subgroup_fast(const F2& qx, const F2& qy)
{
  const G2L::A q = {qx, qy}, nq = {qx, f2_neg(qy)};
  G2L::X xq = {qx, qy, f2_one(), f2_one()};
  for (int i = X_LEN - 2; i >= 0; i--) {
    xq = G2L::x_dbl(xq);
    if (XNAF[i] > 0) G2L::x_madd(xq, q);
    else if (XNAF[i] < 0) G2L::x_madd(xq, nq);
  }
  if (G2L::x_is_zero(xq)) return false; // [x]Q = O: the equation reads Q = O, and Q is not the identity
  G2L::X lhs = xq;
  G2L::x_madd(lhs, q); // [x+1]Q
  const G2L::X p1 = g2_psi(xq), p2 = g2_psi(p1);
  lhs = G2L::x_add(G2L::x_add(lhs, p1), p2);
  G2L::X rhs = G2L::x_dbl(g2_psi(p2));
  if (!G2L::x_is_zero(rhs)) rhs.y = f2_neg(rhs.y);
  return G2L::x_is_zero(G2L::x_add(lhs, rhs));
}
// [z]·P, z < 2^bits given as 32-bit words (little endian), P affine I2 and not the identity: double-and-add on ec29.h's G1
// XYZZ layer (its bounds: X N, < 7p, the others N, < 2p; an affine operand I2).  O for z ≡ 0 mod r.
P29_HD G1L::X g1_mul_bits(const G1L::A& p, const uint32_t* z, int bits)
{
  G1L::X acc = G1L::x_zero();
  const int top = (bits - 1) >> 5;
  for (int w = top; w >= 0; w--) {
    const uint32_t zw = z[w]; // one load per 32 steps
    for (int b = w == top ? ((bits - 1) & 31) : 31; b >= 0; b--) {
      acc = G1L::x_dbl(acc);
      if ((zw >> b) & 1u) G1L::x_madd(acc, p);
    }
  }
  return acc;
}
// Miller loop of the one pair (P, Q), neither the identity (I2 affine coordinates): multi_miller with only pair 0
P29_HD F12 miller_single(const fe9& px, const fe9& py, const F2& qx, const F2& qy)
{
  return multi_miller(true, px, py, qx, qy, false, px, py, nullptr, false, px, py, nullptr);
}
// One proof's share of the combined equation: f = the Miller value of ([z](−A), B), 1 when A or B is the identity (as
// verify_proof drops that pair).  a, b standard form, canonical, on their curves, (0, 0) = identity; 0 < z < 2^128 (four words).
// False when B ≠ O lies outside the order-r subgroup (f = 1 then).
// BOUNDS: −A = (from_std x, fq_neg(from_std y)): I2; g1_mul_bits → XYZZ, not O (z ≢ 0 mod r and A has order r; f stays 1
// otherwise); g1_to_affine → products of f29::mul: N, < 1.1p: I2 as multi_miller wants its P coordinates.
P29_HD bool combined_lane(const fe* a, const fe2* b, const uint32_t* z, F12& f)
{
  const bool a_zero = g1_std_is_zero(a);
  const bool b_zero = g2_std_is_zero(b);
  f = f12_one();
  const F2 bx = Fq2_29::load_std(b[0]), by = Fq2_29::load_std(b[1]);
  if (!b_zero && !g2_in_subgroup_fast(bx, by)) return false;
  if (a_zero || b_zero) return true;
  const G1L::A na = {f29::from_std(a[0]), fq_neg(f29::from_std(a[1]))};
  const G1L::X za = g1_mul_bits(na, z, 128);
  if (G1L::x_is_zero(za)) return true;
  fe9 x, y;
  g1_to_affine(za, x, y);
  f = miller_single(x, y, bx, by);
  return true;
}
// The batch's tail (host): prod = Πᵢ of the lanes' Miller values (I2); u = n_pub + 1 scalars mod r in standard form, u₀ = Σ zᵢ,
// u_{j+1} = Σᵢ zᵢ·sᵢⱼ; sc = Σᵢ zᵢ·Cᵢ (standard-form affine, (0, 0) = O); ic1 / ic1_zero = n_pub + 2 entries, the key's IC
// shifted by one behind an identity entry (ic1_zero[0] = 1), so that public_input's Straus sum gives S_pub = Σⱼ uⱼ·ICⱼ;
// gamma / delta = the key's precomputed lines, nullptr for an identity γ₂ / δ₂.  True iff
//   prod · e(S_pub, γ₂) · e(S_C, δ₂) · e(u₀·α₁, β₂) = 1.
// An identity key point or an identity sum drops its pair, as verify_proof does per proof.  In two steps, so that a caller can
// run the first — which does not need prod — while the lanes are still at work: combined_tail_miller gives the Miller value t
// of the three fixed-G2 pairs, combined_finish decides prod·t.
// BOUNDS: u₀·α₁ through g1_mul_bits / g1_to_affine and S_pub through public_input: I2 affine; S_C from_std: canonical;
// β₂ load_std: canonical; f12_mul and final_exp take and return I2.
P29_HD F12 combined_tail_miller(const fe* alpha, const fe2* beta, const Line* gamma, const Line* delta, const G1L::A* ic1, const uint8_t* ic1_zero,
                                int n_pub, const fe* u, const fe* sc)
{
  const bool az = g1_std_is_zero(alpha);
  const bool bz = g2_std_is_zero(beta);
  fe9 ax = f29::one_m(), ay = ax, px = ax, py = ax;
  bool use0 = !az && !bz;
  if (use0) {
    const G1L::X ua = g1_mul_bits({f29::from_std(alpha[0]), f29::from_std(alpha[1])}, u[0].l, 254);
    use0 = !G1L::x_is_zero(ua);
    if (use0) g1_to_affine(ua, ax, ay);
  }
  const bool use1 = public_input(ic1, ic1_zero, n_pub + 1, u, 1, px, py) && gamma;
  const bool use2 = !g1_std_is_zero(sc) && delta;
  const F2 bx = Fq2_29::load_std(beta[0]), by = Fq2_29::load_std(beta[1]);
  return multi_miller(use0, ax, ay, bx, by, use1, px, py, gamma, use2, f29::from_std(sc[0]), f29::from_std(sc[1]), delta);
}
P29_HD bool combined_finish(const F12& prod, const F12& t) { return f12_eq_canon(final_exp(f12_mul(prod, t)), f12_one()); }
P29_HD bool combined_accept(const F12& prod, const fe* alpha, const fe2* beta, const Line* gamma, const Line* delta, const G1L::A* ic1,
                            const uint8_t* ic1_zero, int n_pub, const fe* u, const fe* sc)
{
  return combined_finish(prod, combined_tail_miller(alpha, beta, gamma, delta, ic1, ic1_zero, n_pub, u, sc));
}

} // namespace p29
} // namespace bn254
