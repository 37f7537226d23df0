// ptau_prepare29_check.cpp — host-side checked build of csrc/prover/ptau_prepare29.h (the butterfly of groth16_ptau_prepare's
// transform over curve points).  Test infrastructure: compiled with g++ -DF29_CHECK by tests/test_ptau_prepare29.py while every
// bound of ff29.h / ec29.h is asserted.  pp29_last_failure() names the first violated bound ("" when none fired).
#include <stddef.h>
#include <stdint.h>

#include "../icicle-snark_amd/csrc/prover/ptau_prepare29.h"

using namespace bn254;
using namespace bn254::pp29;

extern "C" const char* pp29_last_failure() { return f29::g_check_failure ? f29::g_check_failure : ""; }
extern "C" void pp29_reset() { f29::g_check_failure = nullptr; }

// sum = P + w·Q, diff = P − w·Q in the file's form (affine, Montgomery-256, the identity all zero); w standard form, below r, or
// null for level 0 (w = 1, no multiplication)
extern "C" void pp29_butterfly_g1(const G1::A* p, const G1::A* q, const fe* w, G1::A* sum, G1::A* diff) { pp_butterfly_affine<G1, Fq29>(*p, *q, w, sum, diff); }
extern "C" void pp29_butterfly_g2(const G2::A* p, const G2::A* q, const fe* w, G2::A* sum, G2::A* diff) { pp_butterfly_affine<G2, Fq2_29>(*p, *q, w, sum, diff); }
