// beacon_walk_check.cpp — csrc/prover/transcript.h's walk over a section of records, over BEACON records (bit 31 of the stored name_len
// word, 36 bytes behind the name: DESIGN.md §7o), as a program of its own.  Test infrastructure: tests/test_beacon_host.py builds it
// with g++ -DF29_CHECK -fsanitize=address,undefined and runs it as a child process over its arguments, every section in a heap
// block of exactly its size; every trailer the walk hands out is read (list_beacons) and one chain step's tail is hashed, so a
// pointer or a length that leaves the block is seen.
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
struct Info {
  uint32_t index;
  uint8_t hash[32];
  uint32_t iter_exp;
};
uint8_t* exact_block(const std::string& hex, size_t* n)
{
  *n = hex.size() / 2;
  uint8_t* p = (uint8_t*)malloc(*n);
  for (size_t i = 0; i < *n; i++) p[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
  return p;
}
} // namespace

// arguments, a line of output each:
//   w:<fixed>:<name_len_off>:<hex of the section>  →  "rc count bad records beacons sum-of-iter_exp"
//   d:<iter_exp>:<hex of 32 bytes>                 →  the 64 hex digits of beacon_digest
int main(int argc, char** argv)
{
  for (int a = 1; a < argc; a++) {
    const std::string arg = argv[a];
    const size_t c1 = arg.find(':', 2), c2 = arg.compare(0, 2, "w:") == 0 ? arg.find(':', c1 + 1) : c1;
    if (c1 == std::string::npos || c2 == std::string::npos) return 2;
    size_t n = 0;
    uint8_t* p = exact_block(arg.substr(c2 + 1), &n);
    if (arg.compare(0, 2, "w:") == 0) {
      const size_t fixed = (size_t)strtoull(arg.substr(2, c1 - 2).c_str(), nullptr, 10), off = (size_t)strtoull(arg.substr(c1 + 1, c2 - c1 - 1).c_str(), nullptr, 10);
      const Sec s = {p, n};
      std::vector<Record> recs;
      uint32_t count, bad;
      const int rc = walk_records(&s, fixed, off, recs, &count, &bad);
      std::vector<Info> infos(recs.size() + 1);
      const int beacons = list_beacons(recs, infos.data(), infos.size());
      uint64_t sum = 0;
      for (int i = 0; i < beacons; i++) sum += infos[i].iter_exp;
      // what a chain_step reads of each record that the walk handed out
      std::vector<uint8_t> m;
      for (const Record& r : recs) append(m, r.p, off), append(m, r.p + off, hashed_tail(r));
      uint8_t h[32];
      if (!m.empty()) isnark::sha256(m.data(), m.size(), h); // (the library hashes no empty message)
      printf("%d %u %u %zu %d %llu\n", rc, count, bad, recs.size(), beacons, (unsigned long long)sum);
    } else if (arg.compare(0, 2, "d:") == 0 && n == 32) {
      uint8_t out[32];
      beacon_digest(p, (uint32_t)strtoul(arg.substr(2, c1 - 2).c_str(), nullptr, 10), out);
      for (int k = 0; k < 32; k++) printf("%02x", out[k]);
      printf("\n");
    } else {
      return 2;
    }
    free(p);
  }
  return f29::g_check_failure ? 3 : 0;
}
