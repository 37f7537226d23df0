// zkey_setup29_check.cpp — host-side checked build of csrc/prover/zkey_setup29.h (the scalars of groth16_setup).
// Test infrastructure: compiled with g++ -DF29_CHECK by tests/test_zkey_setup29.py while every bound of ff29.h / ec29.h is asserted.
// zs29_last_failure() names the first violated bound ("" when none fired).
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../icicle-snark_amd/csrc/prover/zkey_setup29.h"

using namespace bn254;
using namespace bn254::zs29;

extern "C" const char* zs29_last_failure() { return f29::g_check_failure ? f29::g_check_failure : ""; }
extern "C" void zs29_reset() { f29::g_check_failure = nullptr; }

extern "C" int zs29_toxic_check(const uint8_t* toxic160, uint32_t p, int* which) { return zs_toxic_check(toxic160, p, which); }
extern "C" void zs29_root(uint32_t p, fe* out) { *out = zs_root(p); }

// the lane of zs_lagrange_kernel for (row, j) of the domain 2^p, as the host and the kernel split the work: zs_derive's values, the
// two table entries of j filled by zs_fill_lo / zs_fill_hi, zs_lagrange.  out: standard form.
extern "C" void zs29_lagrange(const uint8_t* toxic160, uint32_t p, uint32_t row, uint32_t j, fe* out)
{
  ZsDerived d;
  zs_derive(toxic160, p, &d);
  const uint32_t k = zs_table_bits(p);
  std::vector<fe> lo((size_t)1 << k), hi((size_t)1 << (p - k));
  zs_fill_lo(p, 0, lo.size(), lo.data());
  zs_fill_hi(p, 0, hi.size(), hi.data());
  *out = zs_lagrange(d.x_mont[row], hi[j >> k], lo[j & ((1u << k) - 1)], d.c_std[row]);
}

// A column's sum as the kernels form it: n_terms entries {row, term} (term 0xffffffff: a public-binding row), the coefficients
// standard form below r (made Montgomery here, as the handle keeps them), L standard form.  piece = 0: one walk over all positions,
// as a light column's lane; piece > 0: items of `piece` positions, each cut into 64 lane slices whose sums are added by the tree
// zs_item_kernel runs, and the items' sums added as zs_combine_kernel adds them.
extern "C" void zs29_column(const uint32_t* entries, uint32_t n_terms, const fe* vals_std, uint32_t n_vals, const fe* L, uint32_t piece, fe* out)
{
  std::vector<fe> vals(n_vals);
  for (uint32_t i = 0; i < n_vals; i++) vals[i] = Fr::to_mont(vals_std[i]);
  const ZnEntry* e = (const ZnEntry*)entries;
  if (!piece) {
    *out = zs_column_sum(e, 0, n_terms, vals.data(), L);
    return;
  }
  const uint32_t WG = 64;
  fe total = Fr::zero();
  for (uint32_t ilo = 0; ilo < n_terms; ilo += piece) {
    const uint32_t ihi = ilo + piece < n_terms ? ilo + piece : n_terms;
    const uint32_t per = (ihi - ilo + WG - 1) / WG;
    fe sh[WG];
    for (uint32_t t = 0; t < WG; t++) {
      const uint32_t lo = ilo + t * per < ihi ? ilo + t * per : ihi, hi = lo + per < ihi ? lo + per : ihi;
      sh[t] = zs_column_sum(e, lo, hi, vals.data(), L);
    }
    for (uint32_t half = WG / 2; half; half >>= 1)
      for (uint32_t t = 0; t < half; t++) sh[t] = Fr::add(sh[t], sh[t + half]);
    total = Fr::add(total, sh[0]);
  }
  *out = total;
}

// comb = β·a + α·b + c, ic = comb·γ⁻¹, cq = comb·δ⁻¹ from zs_derive's values; a, b, c and the results standard form
extern "C" void zs29_outputs(const uint8_t* toxic160, uint32_t p, const fe* a, const fe* b, const fe* c, fe* comb, fe* ic, fe* cq)
{
  ZsDerived d;
  zs_derive(toxic160, p, &d);
  *comb = zs_comb(*a, *b, *c, d.alpha_mont, d.beta_mont);
  *ic = zs_quot(*comb, d.gamma_inv_mont);
  *cq = zs_quot(*comb, d.delta_inv_mont);
}
// the six head scalars zs_derive hands to the arrays: α β δ, β γ δ
extern "C" void zs29_heads(const uint8_t* toxic160, uint32_t p, fe* head1, fe* head2)
{
  ZsDerived d;
  zs_derive(toxic160, p, &d);
  for (int i = 0; i < 3; i++) head1[i] = d.head1[i], head2[i] = d.head2[i];
}
