// r1cs_check.h — one R1CS constraint evaluated at a witness, host and device: groth16_witness_check's kernel (r1cs_check.hip) runs
// one lane per constraint through r1cs_eval / r1cs_holds, and the checked host build (tests/r1cs_check_check.cpp) compiles the
// same text.
//
//   rowptr[3m + 1]   in terms: row 3j + k is linear combination k (0 A, 1 B, 2 C) of constraint j
//   cols[t], vals[t] term t: its wire, and its coefficient in Montgomery form (canonical, < r)
//   w[i]             the witness (or any vector in its place), standard form, canonical
// Fr::mul(val·R, w) = val·w in standard form (as qap_spmv_kernel), so the three sums come out in standard form; a·b is brought
// back with r2(): mul(mul(a, b), R²) = a·b·R⁻¹·R²·R⁻¹ = a·b.  Every operand of a mul is canonical — vals by the load's range test
// and to_mont, w by the witness range kernel that runs first, the sums by add's reduction — which is what Fr's bounds assume.
// An empty row (count 0) is 0; a wire named twice sums.
#pragma once
#include <stdint.h>

#include "../ff.h"

namespace isnark {

// the checked host build: every operand of a mul must be canonical, the first that is not is recorded
#if defined(R1CS_CHECK) && !defined(__HIPCC__)
inline const char* g_r1cs_check_failure = nullptr;
#define R1CS_CANONICAL(x, what) ((void)(bn254::Fr::is_canonical(x) || ::isnark::g_r1cs_check_failure || (::isnark::g_r1cs_check_failure = what)))
#else
#define R1CS_CANONICAL(x, what) ((void)0)
#endif

struct R1csRows {
  bn254::fe a, b, c;
};

// a = A_j·w, b = B_j·w, c = C_j·w.  The three rows advance in lockstep so that the dependent loads (rowptr → wire → witness) of
// all three are in flight together: the column loads of the three rows are issued first, then the coefficients, then the gathers.
// A row that has ended loads nothing (its lanes are masked off for its three loads) and adds nothing.
FF_HD R1csRows r1cs_eval(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ cols, const bn254::fe* __restrict__ vals, const bn254::fe* __restrict__ w, uint32_t j)
{
  using bn254::fe;
  using bn254::Fr;
  const uint32_t r0 = 3 * j;
  uint32_t ka = rowptr[r0], kb = rowptr[r0 + 1], kc = rowptr[r0 + 2];
  const uint32_t ha = kb, hb = kc, hc = rowptr[r0 + 3];
  R1csRows r = {Fr::zero(), Fr::zero(), Fr::zero()};
  while (ka < ha || kb < hb || kc < hc) {
    const bool da = ka < ha, db = kb < hb, dc = kc < hc;
    uint32_t ca = 0, cb = 0, cc = 0;
    fe va = Fr::zero(), vb = Fr::zero(), vc = Fr::zero(), wa = Fr::zero(), wb = Fr::zero(), wc = Fr::zero();
    if (da) ca = cols[ka];
    if (db) cb = cols[kb];
    if (dc) cc = cols[kc];
    if (da) va = vals[ka];
    if (db) vb = vals[kb];
    if (dc) vc = vals[kc];
    if (da) wa = w[ca];
    if (db) wb = w[cb];
    if (dc) wc = w[cc];
    R1CS_CANONICAL(va, "coefficient of A"), R1CS_CANONICAL(vb, "coefficient of B"), R1CS_CANONICAL(vc, "coefficient of C");
    R1CS_CANONICAL(wa, "witness value read by A"), R1CS_CANONICAL(wb, "witness value read by B"), R1CS_CANONICAL(wc, "witness value read by C");
    if (da) r.a = Fr::add(r.a, Fr::mul(va, wa)); // coef·R ⊗ w = coef·w
    if (db) r.b = Fr::add(r.b, Fr::mul(vb, wb));
    if (dc) r.c = Fr::add(r.c, Fr::mul(vc, wc));
    ka++;
    kb++;
    kc++;
  }
  return r;
}

// (A_j·w)·(B_j·w) = C_j·w
FF_HD bool r1cs_holds(const R1csRows& r)
{
  using bn254::Fr;
  R1CS_CANONICAL(r.a, "row sum a"), R1CS_CANONICAL(r.b, "row sum b"), R1CS_CANONICAL(r.c, "row sum c");
  return Fr::eq(Fr::mul(Fr::mul(r.a, r.b), Fr::r2()), r.c);
}

// a witness value as the .wtns holds it is any 256-bit pattern: the range test is a plain comparison with r, no field operation
FF_HD bool r1cs_value_in_range(const bn254::fe& v) { return bn254::Fr::is_canonical(v); }

} // namespace isnark
