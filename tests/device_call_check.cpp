// device_call_check.cpp — host-side build of the pure host pieces the key tools share: circuit_domain (prover_internal.h),
// words_zero / same_point / pairing_eq (verify_host.h) and PtauRanges::verdict (ptau_ranges.h).  Test infrastructure: compiled with
// g++ against the HIP headers and linked with the product library (the host pairing and the point conversions are its exports) by
// tests/test_device_call_host.py, which compares with tests/groth16_dlog_model.py.  With -DDEVICE_CALL_CHECK_MAIN it is a program
// of its own that runs the same functions on the library's generators, for a sanitizer build.
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../icicle-snark_amd/csrc/prover/prover_internal.h"
#include "../icicle-snark_amd/csrc/prover/ptau_ranges.h"
#include "../icicle-snark_amd/csrc/prover/verify_host.h"

namespace pv = isnark::prover;
namespace vb = isnark::vb;

// the prover's error channel, here: the last text
static char g_text[512];
int isnark::prover::fail(int code, const char* fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_text, sizeof g_text, fmt, ap);
  va_end(ap);
  return code;
}

extern "C" uint64_t dc_circuit_domain(uint64_t n_constraints, uint64_t n_public, uint32_t* log2) { return pv::circuit_domain(n_constraints, n_public, log2); }
extern "C" int dc_words_zero(const void* p, size_t bytes) { return vb::words_zero(p, bytes); }
// standard-form points of the C ABI: affine (0, 0) and projective z = 0 are the identity
extern "C" int dc_pairing_eq(const bn254_affine_t* a1, const bn254_g2_affine_t* a2, const bn254_affine_t* b1, const bn254_g2_affine_t* b2) { return vb::pairing_eq(*a1, *a2, *b1, *b2); }
extern "C" int dc_same_point_g1(const bn254_projective_t* l, const bn254_projective_t* r) { return vb::same_point(*l, *r); }
extern "C" int dc_same_point_g2(const bn254_g2_projective_t* l, const bn254_g2_projective_t* r) { return vb::same_point(*l, *r); }
// the return code of the verdict over first[5] for a domain 2^k, its text to `text`
extern "C" int dc_ptau_verdict(const unsigned long long* first, uint32_t k, char* text, size_t cap)
{
  g_text[0] = 0;
  PtauRanges r;
  r.k = k;
  const int rc = r.verdict(first);
  snprintf(text, cap, "%s", g_text);
  return rc;
}

#ifdef DEVICE_CALL_CHECK_MAIN
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      return 1;                                                   \
    }                                                             \
  } while (0)

int main()
{
  uint32_t k = 99;
  EXPECT(pv::circuit_domain(0, 0, &k) == 1 && k == 0);
  EXPECT(pv::circuit_domain(3, 1, &k) == 8 && k == 3);
  EXPECT(pv::circuit_domain((1ull << 28) - 1, 1, &k) == (1ull << 29) && k == 29);

  const uint8_t zeros[33] = {}, tail[33] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
  EXPECT(vb::words_zero(zeros, 33) && vb::words_zero(tail, 32) && !vb::words_zero(tail, 33) && vb::words_zero(tail, 0));

  // G, 2G, and 2G again from its affine form with z = 1: another representation of the same point
  bn254_projective_t g, g2x, g2x_again, id;
  bn254_generator(&g);
  bn254_ecadd(&g, &g, &g2x);
  const bn254_affine_t a2 = vb::affine_or_zero(g2x);
  memset(&g2x_again, 0, sizeof g2x_again);
  g2x_again.x = a2.x, g2x_again.y = a2.y, g2x_again.z.limbs[0] = 1;
  memset(&id, 0, sizeof id);
  EXPECT(vb::same_point(g2x, g2x_again) && !vb::same_point(g, g2x) && vb::same_point(id, id) && !vb::same_point(id, g));
  bn254_g2_projective_t h, h2x, hid;
  bn254_g2_generator(&h);
  bn254_g2_ecadd(&h, &h, &h2x);
  memset(&hid, 0, sizeof hid);
  EXPECT(vb::same_point(h, h) && !vb::same_point(h, h2x) && vb::same_point(hid, hid) && !vb::same_point(hid, h));

  // e(2G₁, G₂) = e(G₁, 2G₂) ≠ e(G₁, G₂); the identity on both sides holds, on one side fails
  const bn254_affine_t g1a = vb::g1_generator_affine(), zero1 = vb::affine_or_zero(id);
  const bn254_g2_affine_t g2a = vb::g2_generator_affine(), h2a = vb::affine_or_zero(h2x), zero2 = vb::affine_or_zero(hid);
  EXPECT(vb::pairing_eq(a2, g2a, g1a, h2a));
  EXPECT(!vb::pairing_eq(a2, g2a, g1a, g2a));
  EXPECT(vb::pairing_eq(zero1, g2a, g1a, zero2) && vb::pairing_eq(g1a, zero2, zero1, zero2));
  EXPECT(!vb::pairing_eq(zero1, g2a, g1a, g2a) && !vb::pairing_eq(g1a, g2a, g1a, zero2));
  // the Montgomery forms come back to the standard ones
  const bn254::G1::A gm = vb::g1_generator_mont();
  const bn254::G1::A gs = {bn254::Fq::from_mont(gm.x), bn254::Fq::from_mont(gm.y)};
  EXPECT(memcmp(&gs, &g1a, sizeof gs) == 0);
  const bn254::G2::A hm = vb::g2_generator_mont();
  const bn254::G2::A hs = {bn254::Fq2Ops::from_mont(hm.x), bn254::Fq2Ops::from_mont(hm.y)};
  EXPECT(memcmp(&hs, &g2a, sizeof hs) == 0);

  unsigned long long first[PtauRanges::N] = {NO_FAULT, NO_FAULT, NO_FAULT, NO_FAULT, NO_FAULT};
  char text[256];
  EXPECT(dc_ptau_verdict(first, 5, text, sizeof text) == 0 && !text[0]);
  first[4] = 7ull << 3 | 2;
  EXPECT(dc_ptau_verdict(first, 5, text, sizeof text) == pv::ERR_FORMAT);
  EXPECT(strcmp(text, "ptau: section 12, block 6, element 7: the point is not on the curve") == 0);
  puts("device_call_check ok");
  return 0;
}
#endif
