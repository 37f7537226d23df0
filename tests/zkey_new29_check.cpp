// zkey_new29_check.cpp — host-side checked build of csrc/prover/zkey_new29.h (the per-column sums of groth16_zkey_new).
// Test infrastructure: compiled with g++ -DF29_CHECK by tests/test_zkey_new29.py while every bound of ff29.h / ec29.h is asserted.
// zn29_last_failure() names the first violated bound ("" when none fired).
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../icicle-snark_amd/csrc/prover/zkey_new29.h"

using namespace bn254;
using namespace bn254::zn29;

extern "C" const char* zn29_last_failure() { return f29::g_check_failure ? f29::g_check_failure : ""; }
extern "C" void zn29_reset() { f29::g_check_failure = nullptr; }

// v standard form, below r → |v| in w[8], its bit length; returns the sign (1: v stands for −|v|)
extern "C" int zn29_signed_short(const fe* v, uint32_t* w, int* bits)
{
  const ZnShort s = zn_signed_short(*v);
  for (int i = 0; i < 8; i++) w[i] = s.w[i];
  *bits = s.bits;
  return s.neg ? 1 : 0;
}

// The sum of a column as the kernels form it: nl = 1 or 3 lists (list k: lens[k] entries {row, term} at entries[k], its bases —
// affine, packed Montgomery-256, as the .ptau holds them — at bases[k]), the coefficients standard form below r (made Montgomery
// here, as the handle keeps them).  piece = 0: one walk over all positions, as a light column's lane; piece > 0: positions in
// slices of `piece`, each walked on its own and the sums added in order with x_add, as a heavy column's items are.
// out: the affine sum in the file's form (Montgomery-256, the identity all zero).
template <class C, class CL>
static void column(int nl, const void* const* bases, const uint32_t* const* entries, const uint32_t* lens, const fe* vals_std, uint32_t n_vals, uint32_t piece, typename C::A* out)
{
  std::vector<fe> vals(n_vals);
  for (uint32_t i = 0; i < n_vals; i++) vals[i] = Fr::to_mont(vals_std[i]);
  ZnList<CL> ls[3];
  uint32_t total = 0;
  for (int k = 0; k < 3; k++) {
    const int src = k < nl ? k : 0;
    ls[k] = {(const ZnEntry*)entries[src], k < nl ? lens[k] : 0u, (const typename C::A*)bases[src]};
    total += ls[k].len;
  }
  typename CL::X acc = CL::x_zero();
  if (!piece) piece = total ? total : 1;
  for (uint32_t lo = 0; lo < total; lo += piece) {
    const uint32_t hi = lo + piece < total ? lo + piece : total;
    typename CL::X part;
    if (nl == 1) {
      const ZnList<CL> one[1] = {ls[0]};
      part = zn_walk<CL, 1>(one, vals.data(), lo, hi);
    } else {
      part = zn_walk<CL, 3>(ls, vals.data(), lo, hi);
    }
    acc = CL::x_add(acc, part);
  }
  *out = C::p_to_affine(C::x_to_projective(CL::x_store(acc)));
}

extern "C" void zn29_column_g1(int nl, const void* const* bases, const uint32_t* const* entries, const uint32_t* lens, const fe* vals_std, uint32_t n_vals, uint32_t piece, G1::A* out)
{
  column<G1, G1L>(nl, bases, entries, lens, vals_std, n_vals, piece, out);
}
extern "C" void zn29_column_g2(int nl, const void* const* bases, const uint32_t* const* entries, const uint32_t* lens, const fe* vals_std, uint32_t n_vals, uint32_t piece, G2::A* out)
{
  column<G2, G2L>(nl, bases, entries, lens, vals_std, n_vals, piece, out);
}
