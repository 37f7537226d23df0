// ptau_contribute29_check.cpp — host-side checked build of csrc/prover/ptau_contribute29.h (one lane of groth16_ptau_contribute: the
// scalar c·τ′^i from the two tables, and the walk over it).  Test infrastructure: compiled with g++ -DF29_CHECK by
// tests/test_ptau_contribute29.py while every bound of ff29.h / ec29.h is asserted.  pc29_last_failure() names the first violated
// bound ("" when none fired).
#include <stddef.h>
#include <stdint.h>

#include "../icicle-snark_amd/csrc/prover/ptau_contribute29.h"

using namespace bn254;
using namespace bn254::pc29;

extern "C" const char* pc29_last_failure() { return f29::g_check_failure ? f29::g_check_failure : ""; }
extern "C" void pc29_reset() { f29::g_check_failure = nullptr; }
extern "C" uint32_t pc29_table_bits(uint32_t power) { return pc_table_bits(power); }

// the tables as the host builds them: lo[j] = τ′^j, j < 2^k; hi[m] = c·τ′^(m·2^k), m < n_hi; τ′ and c standard form, below r.  Filled in
// two ranges each, as side-by-side workers would.
extern "C" void pc29_tables(const fe* tau, const fe* c, uint32_t k, uint32_t n_hi, fe* lo, fe* hi)
{
  const size_t n_lo = (size_t)1 << k;
  const fe one_m = Fr::to_mont(Fr::one_std()), tau_m = Fr::to_mont(*tau), step_m = pc_pow(tau_m, n_lo), c_m = Fr::to_mont(*c);
  pc_fill_powers(tau_m, one_m, 0, n_lo / 2, lo);
  pc_fill_powers(tau_m, one_m, n_lo / 2, n_lo, lo);
  pc_fill_powers(step_m, c_m, 0, n_hi / 2, hi);
  pc_fill_powers(step_m, c_m, n_hi / 2, n_hi, hi);
}
// lane i's scalar, standard form
extern "C" void pc29_scalar(const fe* lo, const fe* hi, uint32_t k, uint64_t i, fe* out) { *out = pc_lane_scalar(hi[i >> k], lo[i & (((uint64_t)1 << k) - 1)]); }
// lane i's point in the file's form (affine, Montgomery-256, the identity all zero)
extern "C" void pc29_lane_g1(const G1::A* p, const fe* lo, const fe* hi, uint32_t k, uint64_t i, G1::A* out)
{
  *out = pc_lane_affine<G1, Fq29>(*p, hi[i >> k], lo[i & (((uint64_t)1 << k) - 1)]);
}
extern "C" void pc29_lane_g2(const G2::A* p, const fe* lo, const fe* hi, uint32_t k, uint64_t i, G2::A* out)
{
  *out = pc_lane_affine<G2, Fq2_29>(*p, hi[i >> k], lo[i & (((uint64_t)1 << k) - 1)]);
}
