// wtns_pack_check.cpp — the host reader and decoder of a packed witness (wtnz_layout, containers.cpp; wz_decode_host and
// wz_decode_value, csrc/prover/wtns_pack.h) as a stand-alone program over a byte-mutation corpus.  Test infrastructure: built with
// the host's AddressSanitizer and UBSan and run by tests/test_wtns_pack_host.py; host code only, it never touches a GPU.
//
//   wtns_pack_check SEED.wtnz ...    every seed is a valid packed witness.  For each: the seed itself must be accepted and decode
//   clean; then every byte of the image is replaced by each of eight values, one at a time, and every prefix of at most 600 bytes is
//   cut — each mutant copied into a heap block of exactly its size, so that a read one byte outside it is the sanitizer's.  Whatever
//   the reader accepts is decoded whole and in every 7-element window.  Prints the counts; exit 0 unless an accepted SEED misbehaves.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "prover/prover_internal.h"
#include "prover/wtns_pack.h"

namespace pv = isnark::prover;
using namespace bn254;

static unsigned long g_accepted = 0, g_refused = 0, g_faulty = 0;

// the image in a heap block of exactly its size; 1 accepted and clean, 0 refused or faulty
static int run(const uint8_t* image, size_t len)
{
  uint8_t* exact = (uint8_t*)malloc(len ? len : 1);
  memcpy(exact, image, len);
  pv::WtnzLayout L;
  int clean = 0;
  if (pv::wtnz_layout(exact, len, &L) != 0 || pv::wtnz_is_bn254(L) != 0) {
    g_refused++;
  } else {
    g_accepted++;
    wz::WzView view;
    view.n = L.n_witness, view.codes = L.codes, view.dir = L.dir, view.payload = L.payload;
    uint8_t* out = (uint8_t*)malloc((size_t)L.n_witness * 32 + 1);
    uint64_t element = 0, faults = 0;
    const int kind = wz::wz_decode_host(view, 0, L.n_witness, out, &element, &faults);
    if (kind) g_faulty++;
    clean = kind == 0;
    for (uint64_t first = 0; first + 7 <= L.n_witness; first += 61) { // windows, as the prover's public signals are decoded
      uint8_t win[7 * 32];
      const int wk = wz::wz_decode_host(view, first, 7, win, &element, &faults);
      if (clean && (wk || memcmp(win, out + 32 * first, sizeof win) != 0)) {
        printf("a window at %llu differs from the whole decode\n", (unsigned long long)first);
        exit(2);
      }
    }
    free(out);
  }
  free(exact);
  return clean;
}

int main(int argc, char** argv)
{
  static const uint8_t subst[8] = {0x00, 0x01, 0x20, 0x21, 0x40, 0x7f, 0x80, 0xff};
  for (int a = 1; a < argc; a++) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) {
      printf("cannot read %s\n", argv[a]);
      return 2;
    }
    std::vector<uint8_t> seed;
    uint8_t chunk[4096];
    for (size_t got; (got = fread(chunk, 1, sizeof chunk, f)) > 0;) seed.insert(seed.end(), chunk, chunk + got);
    fclose(f);
    if (!run(seed.data(), seed.size())) {
      printf("%s: the seed itself is refused or faulty: %s\n", argv[a], pv::last_error_text());
      return 2;
    }
    std::vector<uint8_t> m = seed;
    // the table, the header, the codes and the directory lie in the first bytes; the payload's bytes are sampled
    for (size_t i = 0; i < m.size(); i += (i < 1200 ? 1 : 13)) {
      const uint8_t keep = m[i];
      for (uint8_t s : subst) {
        if (s == keep) continue;
        m[i] = s;
        run(m.data(), m.size());
      }
      m[i] = keep;
    }
    for (size_t cut = 0; cut < seed.size() && cut <= 600; cut++) run(seed.data(), cut);
  }
  printf("accepted %lu (of them faulty %lu) refused %lu\n", g_accepted, g_faulty, g_refused);
  return 0;
}
