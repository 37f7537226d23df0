// zkey_contribute29_check.cpp — host-side checked build of csrc/prover/zkey_contribute29.h (the shared-scalar multiplication of
// groth16_zkey_contribute).  Test infrastructure: compiled with g++ -DF29_CHECK by tests/test_zkey_contribute29.py while every
// bound of ff29.h / ec29.h is asserted.  zc29_last_failure() names the first violated bound ("" when none fired).
#include <stddef.h>
#include <stdint.h>

#include "../icicle-snark_amd/csrc/prover/zkey_contribute29.h"

using namespace bn254;
using namespace bn254::zc29;

extern "C" const char* zc29_last_failure() { return f29::g_check_failure ? f29::g_check_failure : ""; }
extern "C" void zc29_reset() { f29::g_check_failure = nullptr; }

// k standard form, below r → the two masks (eight words each); returns the length
extern "C" int zc29_recode(const fe* k, uint32_t* nonzero, uint32_t* negative)
{
  const ZcDigits d = zc_recode(*k);
  for (int i = 0; i < 8; i++) nonzero[i] = d.nonzero[i], negative[i] = d.negative[i];
  return d.len;
}

// k·P in the file's form (affine, Montgomery-256, the identity all zero): the kernel's walk for G1, the host path that scales
// the header's δ₂ for G2
extern "C" void zc29_mul_g1(const G1::A* base, const fe* k, G1::A* out) { *out = zc_mul_affine<G1, G1L>(*base, *k); }
extern "C" void zc29_mul_g2(const G2::A* base, const fe* k, G2::A* out) { *out = zc_mul_affine<G2, G2L>(*base, *k); }
