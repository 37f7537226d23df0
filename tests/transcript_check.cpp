// transcript_check.cpp — host-side checked build of csrc/prover/transcript.h (the Fiat–Shamir transcript of a ceremony contribution:
// the hashes to a scalar, the challenge of a digest, the walk over a section of records).  Test infrastructure: compiled with
// g++ -DF29_CHECK by tests/test_transcript_host.py as a shared object, and once more with -DTRANSCRIPT_MAIN -fsanitize=address,undefined
// as a program of its own that runs the walker and fr_from_be over its arguments, every input in a heap block of exactly its size.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../icicle-snark_amd/csrc/prover/transcript.h"

using namespace bn254;
using namespace isnark::transcript;

namespace {
struct Sec {
  const uint8_t* p;
  uint64_t size;
};
// `present` = 0: no section.  out = {rc, count, bad, records}
void walk(const uint8_t* p, uint64_t size, int present, uint64_t fixed, uint64_t name_len_off, uint32_t out[4])
{
  const Sec s = {p, size};
  std::vector<Record> recs;
  out[0] = (uint32_t)walk_records(present ? &s : (const Sec*)nullptr, (size_t)fixed, (size_t)name_len_off, recs, &out[1], &out[2]);
  out[3] = (uint32_t)recs.size();
}
} // namespace

extern "C" const char* ts_last_failure() { return f29::g_check_failure ? f29::g_check_failure : ""; }
// W(msg) to out; 1 when the whole buffer (the message and the appended byte) is zero afterwards
extern "C" int ts_wide_hash(const uint8_t* msg, size_t len, fe* out)
{
  std::vector<uint8_t> x(msg, msg + len);
  *out = wide_hash(x);
  if (x.size() != len + 1) return 0;
  for (uint8_t b : x)
    if (b) return 0;
  return 1;
}
extern "C" void ts_fr_from_be(const uint8_t* b, size_t len, fe* out) { *out = fr_from_be(b, len); }
extern "C" void ts_challenge(const uint8_t digest[32], fe* out) { *out = challenge_from_digest(digest); }
extern "C" void ts_walk(const uint8_t* p, uint64_t size, int present, uint64_t fixed, uint64_t name_len_off, uint32_t out[4]) { walk(p, size, present, fixed, name_len_off, out); }

#ifdef TRANSCRIPT_MAIN
// arguments, a line of output each:  w:<fixed>:<name_len_off>:<hex of the section | ->  →  "rc count bad records"
//                                    b:<hex of a big-endian integer>                     →  the 64 hex digits of fr_from_be, big-endian
static uint8_t* exact_block(const std::string& hex, size_t* n)
{
  *n = hex.size() / 2;
  uint8_t* p = (uint8_t*)malloc(*n); // (an empty input: a block of no bytes, which the sanitizer lets nobody read)
  for (size_t i = 0; i < *n; i++) p[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
  return p;
}
int main(int argc, char** argv)
{
  for (int a = 1; a < argc; a++) {
    const std::string arg = argv[a];
    if (arg.compare(0, 2, "w:") == 0) {
      const size_t c1 = arg.find(':', 2), c2 = arg.find(':', c1 + 1);
      const uint64_t fixed = strtoull(arg.substr(2, c1 - 2).c_str(), nullptr, 10), off = strtoull(arg.substr(c1 + 1, c2 - c1 - 1).c_str(), nullptr, 10);
      const std::string hex = arg.substr(c2 + 1);
      const int present = hex != "-";
      size_t n = 0;
      uint8_t* p = present ? exact_block(hex, &n) : nullptr;
      uint32_t out[4];
      walk(p, n, present, fixed, off, out);
      printf("%u %u %u %u\n", out[0], out[1], out[2], out[3]);
      free(p);
    } else if (arg.compare(0, 2, "b:") == 0) {
      size_t n = 0;
      uint8_t* p = exact_block(arg.substr(2), &n);
      const fe v = fr_from_be(p, n);
      for (int k = 7; k >= 0; k--) printf("%08x", v.l[k]);
      printf("\n");
      free(p);
    } else {
      return 2;
    }
  }
  return ts_last_failure()[0] ? 3 : 0;
}
#endif
