// r1cs_check_check.cpp — host-side build of csrc/prover/r1cs_check.h (the per-constraint evaluation of groth16_witness_check).
// Test infrastructure: compiled with g++ by tests/test_r1cs_check_host.py, which builds the rows in Python and compares with
// Python integers.  -DR1CS_CHECK records the first Fr::mul operand that is not canonical (the bound the header states):
// r1cs_chk_last_failure() names it, "" when none was seen.
#include <stddef.h>
#include <stdint.h>

#include "../icicle-snark_amd/csrc/prover/r1cs_check.h"

using namespace bn254;

extern "C" const char* r1cs_chk_last_failure() { return isnark::g_r1cs_check_failure ? isnark::g_r1cs_check_failure : ""; }
extern "C" void r1cs_chk_reset() { isnark::g_r1cs_check_failure = nullptr; }

// cols[t] and Montgomery vals[t] from standard-form coefficients, as the load's fill kernel makes them (value < r first)
extern "C" int r1cs_chk_fill(const uint32_t* wires, const fe* std_vals, uint32_t n_terms, uint32_t n_wires, uint32_t* cols, fe* vals)
{
  for (uint32_t t = 0; t < n_terms; t++) {
    if (wires[t] >= n_wires) return -1;
    if (!Fr::is_canonical(std_vals[t])) return -2;
    cols[t] = wires[t];
    vals[t] = Fr::to_mont(std_vals[t]);
  }
  return 0;
}

// out96 = a ‖ b ‖ c (standard form) of constraint j; returns 1 when it holds, 0 when not
extern "C" int r1cs_chk_constraint(const uint32_t* rowptr, const uint32_t* cols, const fe* vals, const fe* w, uint32_t j, fe* out96)
{
  const isnark::R1csRows r = isnark::r1cs_eval(rowptr, cols, vals, w, j);
  out96[0] = r.a;
  out96[1] = r.b;
  out96[2] = r.c;
  return isnark::r1cs_holds(r) ? 1 : 0;
}

extern "C" int r1cs_chk_value_in_range(const fe* v) { return isnark::r1cs_value_in_range(*v) ? 1 : 0; }
