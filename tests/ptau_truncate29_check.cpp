// ptau_truncate29_check.cpp — host-side checked build of csrc/prover/ptau_truncate29.h (one lane of groth16_ptau_truncate's fix-up: the
// scalar ω′^j/2n′ from the two tables, its signed digits, the walk over Q's table, B − T).  Test infrastructure: compiled with g++
// -DF29_CHECK by tests/test_ptau_truncate29.py while every bound of ff29.h / ec29.h is asserted.  pt29_last_failure() names the first
// violated bound ("" when none fired).
#include <stddef.h>
#include <stdint.h>

#include "../icicle-snark_amd/csrc/prover/ptau_truncate29.h"

using namespace bn254;
using namespace bn254::pt29;

extern "C" const char* pt29_last_failure() { return f29::g_check_failure ? f29::g_check_failure : ""; }
extern "C" void pt29_reset() { f29::g_check_failure = nullptr; }
extern "C" uint32_t pt29_table_bits(uint32_t power) { return pc29::pc_table_bits(power); }
extern "C" void pt29_geometry(int32_t out[5])
{
  out[0] = PT_C, out[1] = PT_WINDOWS, out[2] = PT_ROW, out[3] = PT_TABLE_POINTS, out[4] = PT_LDS_BYTES;
}

// the scalars' tables as ptau_truncate.hip builds them: lo[i] = w^i, i < 2^k; hi[m] = ninv·w^(m·2^k), m < n_hi; w the root of order 2n′ and
// ninv = 1/2n′ in standard form.  Two ranges each, as side-by-side workers fill them.
extern "C" void pt29_tables(const fe* w, const fe* ninv, uint32_t k, uint32_t n_hi, fe* lo, fe* hi)
{
  const size_t n_lo = (size_t)1 << k;
  const fe one_m = Fr::to_mont(Fr::one_std()), w_m = Fr::to_mont(*w), step_m = pc29::pc_pow(w_m, n_lo), c_m = Fr::to_mont(*ninv);
  pc29::pc_fill_powers(w_m, one_m, 0, n_lo / 2, lo);
  pc29::pc_fill_powers(w_m, one_m, n_lo / 2, n_lo, lo);
  pc29::pc_fill_powers(step_m, c_m, 0, n_hi / 2, hi);
  pc29::pc_fill_powers(step_m, c_m, n_hi / 2, n_hi, hi);
}
extern "C" void pt29_scalar(const fe* lo, const fe* hi, uint32_t k, uint64_t j, fe* out) { *out = pc29::pc_lane_scalar(hi[j >> k], lo[j & (((uint64_t)1 << k) - 1)]); }

// the PT_WINDOWS digits of s, low window first, and the carry left behind the last
extern "C" uint32_t pt29_digits(const fe* s, int32_t* out)
{
  uint32_t reg[8], carry = 0;
  for (int i = 0; i < 8; i++) reg[i] = s->l[i];
  for (int w = 0; w < PT_WINDOWS; w++) out[w] = pt_next_digit(reg, carry);
  return carry;
}

extern "C" void pt29_fill_table(const G1::A* q, G1::A* table) { pt_fill_table(*q, table); }
// [s]·Q from the table, in the file's form
extern "C" void pt29_walk(const fe* s, const G1::A* table, G1::A* out)
{
  const PtArrayFetch fetch = {table};
  *out = pt_file_form(pt_walk(*s, fetch));
}
// B − [hi·lo]·Q, in the file's form
extern "C" void pt29_lane(const G1::A* b, const fe* hi_mont, const fe* lo_mont, const G1::A* table, G1::A* out) { *out = pt_lane_affine(*b, *hi_mont, *lo_mont, table); }
// a table entry back in the file's form
extern "C" void pt29_entry(const G1::A* table, uint32_t i, G1::A* out)
{
  G1L::X x = G1L::x_zero();
  G1L::x_madd(x, G1L::load_affine(table[i], G1L::INTERNAL, false));
  *out = pt_file_form(x);
}
