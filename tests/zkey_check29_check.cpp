// zkey_check29_check.cpp — host-side checked build of csrc/prover/zkey_check29.h (the per-point tests of groth16_zkey_check).
// Test infrastructure: compiled with g++ -DF29_CHECK by tests/test_zkey_check29.py while every bound of ff29.h / ec29.h /
// pairing29.h is asserted.  zk29_last_failure() names the first violated bound ("" when none fired); zk29_products() counts the
// lazy multiplications and squarings run so far, so a test can show that a rejected coordinate never reached one.
#include <stddef.h>
#include <stdint.h>

#include "../icicle-snark_amd/csrc/prover/zkey_check29.h"

using namespace bn254;

extern "C" const char* zk29_last_failure() { return f29::g_check_failure ? f29::g_check_failure : ""; }
extern "C" void zk29_reset() { f29::g_check_failure = nullptr; }
extern "C" unsigned long zk29_products() { return f29::g_check_products; }

// a point as the .zkey holds it: affine, packed Montgomery-256, x then y
extern "C" int zk29_classify_g1(const fe* mont) { return p29::classify_g1(mont); }
extern "C" int zk29_classify_g2(const fe2* mont) { return p29::classify_g2(mont); }
