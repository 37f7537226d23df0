// point_pack29_check.cpp — host-side checked build of csrc/prover/point_pack29.h (the packed point form of groth16_ptau_pack /
// groth16_ptau_unpack: signs, roots, both encodings).  Test infrastructure: compiled with g++ -DF29_CHECK by
// tests/test_point_pack29.py while every bound of ff29.h / ec29.h / pairing29.h is asserted.  pk29_last_failure() names the first
// violated bound ("" when none fired); pk29_products() counts the lazy multiplications and squarings run so far.
#include <stddef.h>
#include <stdint.h>

#include "../icicle-snark_amd/csrc/prover/point_pack29.h"

using namespace bn254;

extern "C" const char* pk29_last_failure() { return f29::g_check_failure ? f29::g_check_failure : ""; }
extern "C" void pk29_reset() { f29::g_check_failure = nullptr; }
extern "C" unsigned long pk29_products() { return f29::g_check_products; }

// file-form points (affine, packed Montgomery-256, x then y) that classify has passed
extern "C" int pk29_sign_g1(const fe* mont) { return pk29::pk_sign_g1(mont) ? 1 : 0; }
extern "C" int pk29_sign_g2(const fe2* mont) { return pk29::pk_sign_g2(mont) ? 1 : 0; }

// a and the root as canonical Montgomery-256 words; 1 when *root is a root of a
extern "C" int pk29_sqrt_fq(const fe* a, fe* root)
{
  fe9 r;
  const bool ok = pk29::pk_sqrt_fq(f29::from_mont256(*a), &r);
  *root = f29::to_mont256(r);
  return ok ? 1 : 0;
}
extern "C" int pk29_sqrt_fq2(const fe2* a, fe2* root)
{
  p29::F2 r;
  const bool ok = pk29::pk_sqrt_fq2(Fq2_29::load_mont256(*a), &r);
  *root = Fq2_29::store_mont256(r);
  return ok ? 1 : 0;
}

// pack as the kernels do: the lane test first; its kind when the point is faulty (nothing written)
extern "C" int pk29_pack_g1(const fe* mont, fe* word)
{
  if (const int kind = p29::classify_g1(mont)) return kind;
  pk29::pk_pack_g1(mont, word);
  return 0;
}
extern "C" int pk29_pack_g2(const fe2* mont, fe2* word)
{
  if (const int kind = p29::classify_g2(mont)) return kind;
  pk29::pk_pack_g2(mont, word);
  return 0;
}
extern "C" int pk29_unpack_g1(const fe* word, fe* mont) { return pk29::pk_unpack_g1(*word, mont); }
extern "C" int pk29_unpack_g2(const fe2* word, fe2* mont) { return pk29::pk_unpack_g2(*word, mont); }
