// ptau_verify29.h — the scalars of groth16_ptau_verify's Lagrange equations (ptau_verify.hip), host and device: what
// one lane computes for one element of a prepared section (λ_e) and of its source (d_i), and the seed-derived values both are made
// from.  The kernels run one lane per element through pv_lagrange_scalar and pv_power_scalar; the host derives x, y, μ_p, C, T with
// pv_derive and fills the four small tables with ptau_contribute29.h's pc_fill_powers; the F29_CHECK host build
// (tests/ptau_verify29_check.cpp) compiles the same text.
//
// The equation, per section pair (S the source, B its prepared section; pmax = power + 1 for 2 → 12, power for the others):
//     Σ_e λ_e·B_e = Σ_{i < min(|S|, 2^pmax)} d_i·S_i
//   x            SHA-256(seed ‖ "icicle-snark ptau verify v1" ‖ LE32(c)) read as a big-endian integer, mod r, for the first c = 0, 1, …
//                with x ≠ 0 and x^(2^(power+1)) ≠ 1: x lies in no domain of the file, so no denominator below is zero.  y = x⁻¹.
//   μ_p          combined_coefficient(seed, 2^32 + p), p ≤ power + 1: 128 bits, never 0 (sha256.h).
//   Ω            the root of unity of order 2^(power+1); ω_p^j = Ω^(j·2^(power+1−p)).
//   λ_e          element e of B is element j = e + 1 − 2^p of block p = ⌊log₂(e + 1)⌋:
//                λ_e = C[p]·(x − Ω^(j·2^(power+1−p)))⁻¹,  C[p] = μ_p·(x^(2^p) − 1)
//   d_i          q = the least p with 2^p > i:  d_i = y^(i+1)·T[q],  T[q] = Σ_{p=q}^{pmax} μ_p·x^(2^p)
// Why it holds: f(X) = Σ_{i<n} x^(n−1−i)·X^i = (x^n − X^n)/(x − X), so f(ω^j) = (x^n − 1)/(x − ω^j) for ω^n = 1, and a block that is
// the inverse transform of its source satisfies Σ_j f(ω^j)·B_j = Σ_i x^(n−1−i)·S_i whatever S is — the zero-extended source of
// section 12's last block included.  Summed over the blocks with the multipliers μ_p, the right side collects, for source element
// i, Σ_{p: 2^p > i} μ_p·x^(2^p − 1 − i) = y^(i+1)·T[q].
//
//   pv_block_of(e)            p = ⌊log₂(e + 1)⌋
//   pv_lagrange_exponent(…)   t = j·2^(power+1−p) < 2^(power+1): Ω^t = hi[t ≫ k]·lo[t mod 2^k], lo[j] = Ω^j, hi[m] = Ω^(m·2^k)
//   pv_lagrange_scalar(…)     from the two entries: w = hi·lo (Montgomery), (x − w)⁻¹ by Fermat (Fr::inv, Montgomery in and out), times
//                             C[p] in STANDARD form: (a·R)·c·R⁻¹ = a·c, the MSM's form, canonical (Fr::mul reduces below r)
//   pv_first_block_over(i)    q
//   pv_power_scalar(…)        y^(i+1) = hi[i ≫ k]·lo[i mod 2^k] with lo[j] = y^j and hi[m] = y·y^(m·2^k) (ptau-contribute's scheme with
//                             c = y), Montgomery; times T[q] in standard form: standard form, canonical
// k = pc_table_bits(power); both index ranges are below 2^(power+1), so hi has 2^(power+1−k) entries and lo 2^k.
//
// BOUNDS.  Everything is ff.h's Fr on canonical words: the tables are Fr::mul's output (below r), Fr::sub takes and returns
// canonical operands, C and T are built from Fr::mul and Fr::add.  x − Ω^t is never 0 (x's choice), so Fr::inv never sees 0.  No
// lazy-limb arithmetic is entered from here: the F29_CHECK build has no bound to fire, and asserts that none did.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "ptau_contribute29.h"
#include "sha256.h"

namespace bn254 {
namespace pv29 {

constexpr uint32_t PV_BLOCKS = 29; // p ≤ power + 1 ≤ 28
// one value per block: a kernel takes it inside its argument struct and looks its lane's entry up there
struct PvBlockTable {
  fe v[PV_BLOCKS];
};

PP_HD uint32_t pv_block_of(uint64_t e) { return 63u - (uint32_t)__builtin_clzll(e + 1); }
PP_HD uint32_t pv_first_block_over(uint64_t i) { return i ? 64u - (uint32_t)__builtin_clzll(i) : 0u; }

PP_HD uint64_t pv_lagrange_exponent(uint64_t e, uint32_t power, uint32_t* p)
{
  *p = pv_block_of(e);
  const uint64_t j = e + 1 - ((uint64_t)1 << *p);
  return j << (power + 1 - *p);
}
PP_HD fe pv_lagrange_scalar(const fe& x_mont, const fe& hi_mont, const fe& lo_mont, const fe& c_std)
{
  return Fr::mul(Fr::inv(Fr::sub(x_mont, Fr::mul(hi_mont, lo_mont))), c_std);
}
PP_HD fe pv_power_scalar(const fe& hi_mont, const fe& lo_mont, const fe& t_std) { return Fr::mul(Fr::mul(hi_mont, lo_mont), t_std); }

// ---- the host's side: the seed-derived values
const char PV_TAG[] = "icicle-snark ptau verify v1";

// a big-endian integer of 32 bytes mod r, by Horner's rule in additions
inline fe pv_fr_from_be32(const uint8_t b[32])
{
  fe acc = Fr::zero();
  for (int i = 0; i < 32; i++) {
    for (int k = 0; k < 8; k++) acc = Fr::dbl(acc);
    fe d = Fr::zero();
    d.l[0] = b[i];
    acc = Fr::add(acc, d);
  }
  return acc;
}

struct PvDerived {
  uint32_t tries;                // the c that gave x
  fe x_mont, y_mont;             // Montgomery form
  PvBlockTable mu, c, t12, t13;  // standard form; entries above power + 1 are 0.  t12: pmax = power + 1; t13: pmax = power
};

inline void pv_derive(const uint8_t seed[32], uint32_t power, PvDerived* d)
{
  memset(d, 0, sizeof *d);
  const fe one_m = Fr::one_mont();
  fe xp[PV_BLOCKS]; // x^(2^p), Montgomery
  for (uint32_t c = 0;; c++) {
    uint8_t msg[32 + sizeof PV_TAG - 1 + 4], digest[32];
    memcpy(msg, seed, 32);
    memcpy(msg + 32, PV_TAG, sizeof PV_TAG - 1);
    for (int k = 0; k < 4; k++) msg[32 + sizeof PV_TAG - 1 + k] = (uint8_t)(c >> (8 * k));
    isnark::sha256(msg, sizeof msg, digest);
    const fe x = pv_fr_from_be32(digest);
    if (Fr::is_zero(x)) continue;
    xp[0] = Fr::to_mont(x);
    for (uint32_t p = 1; p <= power + 1; p++) xp[p] = Fr::sqr(xp[p - 1]);
    if (Fr::eq(xp[power + 1], one_m)) continue;
    d->tries = c;
    break;
  }
  d->x_mont = xp[0];
  d->y_mont = Fr::inv(xp[0]);
  fe term[PV_BLOCKS]; // μ_p·x^(2^p), standard form
  for (uint32_t p = 0; p <= power + 1; p++) {
    isnark::combined_coefficient(seed, ((uint64_t)1 << 32) + p, (uint8_t*)&d->mu.v[p]);
    d->c.v[p] = Fr::mul(d->mu.v[p], Fr::sub(xp[p], one_m)); // μ·((x^(2^p) − 1)·R)·R⁻¹
    term[p] = Fr::mul(d->mu.v[p], xp[p]);
  }
  fe acc = Fr::zero();
  for (uint32_t p = power + 2; p-- > 0;) {
    acc = Fr::add(acc, term[p]);
    d->t12.v[p] = acc;
    d->t13.v[p] = p <= power ? Fr::sub(acc, term[power + 1]) : Fr::zero();
  }
}

} // namespace pv29
} // namespace bn254
