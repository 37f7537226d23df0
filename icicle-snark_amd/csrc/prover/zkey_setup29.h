// zkey_setup29.h — the scalars of groth16_setup (zkey_setup.hip), host and device: the discrete logarithm of every
// point of a Groth16 proving key made directly from toxic waste (τ, α, β, γ, δ).  synth.key_scalars is the definition.  The kernels
// run one lane per Lagrange value, per (matrix, wire) column and per wire through the FF_HD functions below; the host derives the
// shared values with zs_derive and fills the two tables of ω with zs_fill_tables; the F29_CHECK host build
// (tests/zkey_setup29_check.cpp) compiles the same text.
//
// n = 2^p the circuit's domain, ω its root of unity, g = ω_{2n} (g² = ω, gⁿ = −1).
//   zs_root(p)                 ω_{2^p}, standard form: the 2^28-th root squared down (the value the library's NTT domain uses)
//   zs_toxic_check(t, p)       0, or the first fault: scalar by scalar τ … δ a value ≥ r (ZS_RANGE) or 0 (ZS_ZERO), then τ^(2n) = 1
//                              (ZS_DOMAIN): τ in the domain makes τ − ωʲ vanish, τ in the coset g·domain makes τ/g − ωʲ vanish.
//   zs_table_bits(p)           k = (p + 1)/2: j < 2^p splits into j ≫ k < 2^(p−k) and j mod 2^k; lo[i] = ω^i, hi[i] = ω^(i·2^k)
//   zs_lagrange(x, hi, lo, c)  w = hi·lo = ωʲ (Montgomery); w·(x − w)⁻¹ by Fermat (Fr::inv, a lane-uniform exponent), times c in
//                              STANDARD form: the standard form of c·ωʲ/(x − ωʲ), canonical.
//                                row 0:  x = τ,    c = (τⁿ − 1)/n                      →  L_j(τ)
//                                row 1:  x = τ/g,  c = ((τ/g)ⁿ − 1)/n · (τⁿ − 1)/(−2δ)  →  L_j(τ/g)·(τⁿ − 1)/(−2δ), section 9's H_j
//   zs_term(e, vals, L)        one term of a column: v·L_row, v the handle's Montgomery coefficient (Fr::mul(v·R, L) = v·L, standard
//                              form), a public-binding row's coefficient 1.  L_row is row 0 at the term's constraint.
//   zs_column_sum(…)           Σ zs_term over positions [lo, hi) of a column list
//   zs_comb(a, b, c, α, β)     β·a + α·b + c, α and β Montgomery, the rest standard: standard
//   zs_quot(comb, inv)         comb·γ⁻¹ or comb·δ⁻¹, the inverse Montgomery: standard
//
// BOUNDS.  Everything is ff.h's Fr on canonical words: the tables and the derived values are Fr::mul's output (below r), Fr::add
// and Fr::sub take and return canonical operands, the handle's coefficients are canonical by its load.  x − ωʲ is never 0 (the
// toxic check), so Fr::inv never sees 0.  Field addition is exact: a column's sum does not depend on the order of its terms or on
// how it was cut.  No lazy-limb arithmetic is entered from here: the F29_CHECK build has no bound to fire, and asserts that none did.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "ptau_contribute29.h"
#include "zkey_new29.h"

namespace bn254 {
namespace zs29 {

using zn29::ZnEntry;

enum { ZS_OK = 0, ZS_RANGE = 1, ZS_ZERO = 2, ZS_DOMAIN = 3 };
constexpr uint32_t ZS_MAX_POWER = 27; // g = ω_{2n} needs 2n ≤ 2^28

FF_HD uint32_t zs_table_bits(uint32_t p) { return (p + 1) / 2; }

FF_HD fe zs_lagrange(const fe& x_mont, const fe& hi_mont, const fe& lo_mont, const fe& c_std)
{
  const fe w = Fr::mul(hi_mont, lo_mont);
  return Fr::mul(Fr::mul(w, Fr::inv(Fr::sub(x_mont, w))), c_std);
}

FF_HD fe zs_term(const ZnEntry& e, const fe* vals, const fe* L)
{
  const fe l = L[e.row];
  return e.term == zn29::ZN_BINDING ? l : Fr::mul(vals[e.term], l);
}
FF_HD fe zs_column_sum(const ZnEntry* entries, uint32_t lo, uint32_t hi, const fe* vals, const fe* L)
{
  fe acc = Fr::zero();
  for (uint32_t q = lo; q < hi; q++) acc = Fr::add(acc, zs_term(entries[q], vals, L));
  return acc;
}

FF_HD fe zs_comb(const fe& a, const fe& b, const fe& c, const fe& alpha_mont, const fe& beta_mont)
{
  return Fr::add(Fr::add(Fr::mul(beta_mont, a), Fr::mul(alpha_mont, b)), c);
}
FF_HD fe zs_quot(const fe& comb, const fe& inv_mont) { return Fr::mul(comb, inv_mont); }

// ---- the host's side
inline fe zs_root(uint32_t p) // p ≤ 28
{
  // the primitive 2^28-th root of unity of BN254's scalar field
  fe w = {{0x725b19f0u, 0x9bd61b6eu, 0x41112ed4u, 0x402d111eu, 0x8ef62abcu, 0x00e0a7ebu, 0xa58a7e85u, 0x2a3c09f0u}};
  w = Fr::to_mont(w);
  for (uint32_t i = p; i < 28; i++) w = Fr::sqr(w);
  return Fr::from_mont(w);
}

// toxic: τ, α, β, γ, δ as 32-byte little-endian words.  *which (may be null): the scalar at fault, 0 … 4
inline int zs_toxic_check(const uint8_t toxic160[160], uint32_t p, int* which)
{
  fe t[5];
  memcpy(t, toxic160, 160);
  int kind = ZS_OK, at = 0;
  for (int i = 0; i < 5 && !kind; i++) {
    at = i;
    if (!Fr::is_canonical(t[i])) kind = ZS_RANGE;
    else if (Fr::is_zero(t[i])) kind = ZS_ZERO;
  }
  if (!kind) {
    fe x = Fr::to_mont(t[0]);
    for (uint32_t i = 0; i <= p; i++) x = Fr::sqr(x); // τ^(2n)
    if (Fr::eq(x, Fr::one_mont())) kind = ZS_DOMAIN, at = 0;
    explicit_bzero(&x, sizeof x);
  }
  explicit_bzero(t, sizeof t);
  if (which) *which = at;
  return kind;
}

// what every lane shares.  Secret: the caller wipes it.
struct ZsDerived {
  fe x_mont[2];                        // τ, τ/g
  fe c_std[2];                         // the two rows' constants (above)
  fe alpha_mont, beta_mont;
  fe gamma_inv_mont, delta_inv_mont;
  fe head1[3], head2[3];               // α, β, δ and β, γ, δ in standard form: the first scalars of the G1 and the G2 array
};
// toxic has passed zs_toxic_check for p
inline void zs_derive(const uint8_t toxic160[160], uint32_t p, ZsDerived* d)
{
  fe t[5];
  memcpy(t, toxic160, 160);
  const fe one_m = Fr::one_mont();
  const fe tau_m = Fr::to_mont(t[0]);
  fe tn = tau_m; // τⁿ
  for (uint32_t i = 0; i < p; i++) tn = Fr::sqr(tn);
  fe n_m = one_m; // n
  for (uint32_t i = 0; i < p; i++) n_m = Fr::dbl(n_m);
  const fe n_inv = Fr::inv(n_m);
  const fe g_inv = Fr::inv(Fr::to_mont(zs_root(p + 1)));
  const fe z = Fr::sub(tn, one_m);                                                       // τⁿ − 1
  const fe zc = Fr::sub(Fr::neg(tn), one_m);                                             // (τ/g)ⁿ − 1 = −τⁿ − 1
  const fe m2d_inv = Fr::inv(Fr::neg(Fr::dbl(Fr::to_mont(t[4]))));                       // (−2δ)⁻¹
  d->x_mont[0] = tau_m;
  d->x_mont[1] = Fr::mul(tau_m, g_inv);
  d->c_std[0] = Fr::from_mont(Fr::mul(z, n_inv));
  d->c_std[1] = Fr::from_mont(Fr::mul(Fr::mul(zc, n_inv), Fr::mul(z, m2d_inv)));
  d->alpha_mont = Fr::to_mont(t[1]);
  d->beta_mont = Fr::to_mont(t[2]);
  d->gamma_inv_mont = Fr::inv(Fr::to_mont(t[3]));
  d->delta_inv_mont = Fr::inv(Fr::to_mont(t[4]));
  d->head1[0] = t[1], d->head1[1] = t[2], d->head1[2] = t[4];
  d->head2[0] = t[2], d->head2[1] = t[3], d->head2[2] = t[4];
  explicit_bzero(t, sizeof t);
}

// lo[i] = ω^i for i in [first, last) of 2^k, hi[i] = ω^(i·2^k) for i in [first, last) of 2^(p−k): ranges, to be filled side by side
inline void zs_fill_lo(uint32_t p, size_t first, size_t last, fe* lo) { pc29::pc_fill_powers(Fr::to_mont(zs_root(p)), Fr::one_mont(), first, last, lo); }
inline void zs_fill_hi(uint32_t p, size_t first, size_t last, fe* hi)
{
  pc29::pc_fill_powers(pc29::pc_pow(Fr::to_mont(zs_root(p)), (uint64_t)1 << zs_table_bits(p)), Fr::one_mont(), first, last, hi);
}

} // namespace zs29
} // namespace bn254
