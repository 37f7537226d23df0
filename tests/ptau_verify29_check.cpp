// ptau_verify29_check.cpp — host-side checked build of csrc/prover/ptau_verify29.h (the scalars of groth16_ptau_verify's Lagrange
// equations: the seed-derived values, and what one lane computes from the two small tables).  Test infrastructure: compiled with g++
// -DF29_CHECK by tests/test_ptau_verify29.py.  pv29_last_failure() names the first violated bound ("" when none fired).
#include <stddef.h>
#include <stdint.h>

#include "../icicle-snark_amd/csrc/prover/ptau_verify29.h"

using namespace bn254;
using namespace bn254::pv29;

extern "C" const char* pv29_last_failure() { return f29::g_check_failure ? f29::g_check_failure : ""; }
extern "C" void pv29_reset() { f29::g_check_failure = nullptr; }
extern "C" uint32_t pv29_table_bits(uint32_t power) { return pc29::pc_table_bits(power); }

// x, y in standard form; mu, c, t12, t13: 29 entries each, standard form; returns the c that gave x
extern "C" uint32_t pv29_derive(const uint8_t* seed, uint32_t power, fe* x, fe* y, fe* mu, fe* c, fe* t12, fe* t13)
{
  PvDerived d;
  pv_derive(seed, power, &d);
  *x = Fr::from_mont(d.x_mont);
  *y = Fr::from_mont(d.y_mont);
  for (uint32_t p = 0; p < PV_BLOCKS; p++) mu[p] = d.mu.v[p], c[p] = d.c.v[p], t12[p] = d.t12.v[p], t13[p] = d.t13.v[p];
  return d.tries;
}
// the tables as the host builds them: lo[j] = base^j, j < 2^k; hi[m] = start·base^(m·2^k), m < n_hi; base and start standard form, below
// r (y and y for the powers of y, Ω and 1 for the roots).  Filled in two ranges each, as side-by-side workers would.
extern "C" void pv29_tables(const fe* base, const fe* start, uint32_t k, uint32_t n_hi, fe* lo, fe* hi)
{
  const size_t n_lo = (size_t)1 << k;
  const fe one_m = Fr::one_mont(), base_m = Fr::to_mont(*base), step_m = pc29::pc_pow(base_m, n_lo), start_m = Fr::to_mont(*start);
  pc29::pc_fill_powers(base_m, one_m, 0, n_lo / 2, lo);
  pc29::pc_fill_powers(base_m, one_m, n_lo / 2, n_lo, lo);
  pc29::pc_fill_powers(step_m, start_m, 0, n_hi / 2, hi);
  pc29::pc_fill_powers(step_m, start_m, n_hi / 2, n_hi, hi);
}
// lane i of a source: d_i, standard form; t: the 29 entries of T
extern "C" void pv29_power(const fe* lo, const fe* hi, uint32_t k, uint64_t i, const fe* t, fe* out)
{
  *out = pv_power_scalar(hi[i >> k], lo[i & (((uint64_t)1 << k) - 1)], t[pv_first_block_over(i)]);
}
// lane e of a prepared section: λ_e, standard form; x standard form, c: the 29 entries of C.  Returns the table index of Ω's power.
extern "C" uint64_t pv29_lagrange(const fe* lo, const fe* hi, uint32_t k, uint32_t power, uint64_t e, const fe* x, const fe* c, fe* out)
{
  uint32_t p;
  const uint64_t t = pv_lagrange_exponent(e, power, &p);
  *out = pv_lagrange_scalar(Fr::to_mont(*x), hi[t >> k], lo[t & (((uint64_t)1 << k) - 1)], c[p]);
  return t;
}
