// msm_sort_plan_check.cpp — host check of csrc/msm_sort_plan.h: the shape msm_sort.hip allocates and enqueues for one digit sort
// (msm_sort_shape), over the combinations of tests/msm_recode_check.cpp's sweep and an entries hint of 0 and L.
// Test infrastructure: a stand-alone program built by tests/test_msm_sort_plan_host.py with g++, once plainly and once with
// -fsanitize=address,undefined.
//
//   msm_sort_plan_check sweep                                both workspace layouts (order, disjoint regions, what the zeroing kernels
//                                                            take as one run, alignment, totals) and each path's own conditions;
//                                                            prints the counts and one combination per path; exit status 1 on a miss
//   msm_sort_plan_check shape L,c_cfg,tab,bits,pf,hint ...   prints "path pb low c W large_thr" of each, one line per argument
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "../icicle-snark_amd/csrc/msm_sort_plan.h"

using namespace isnark;

namespace {

const char* const PATH_NAME[3] = {"staged", "two-level", "global"};

int g_failures = 0;
void fail(const SortShape& sh, uint32_t L, int c_cfg, int tab, int bits, int pf, uint64_t hint, const char* what)
{
  if (g_failures++ < 12)
    fprintf(stderr, "FAIL %s: L=%u c_cfg=%d tab=%d bits=%d pf=%d hint=%llu -> c=%d W=%d tab=%d path=%s pb=%d low=%d low_bits=%d\n", what, L, c_cfg, tab, bits, pf, (unsigned long long)hint, sh.g.c,
            sh.g.W, sh.g.tab, PATH_NAME[sh.path], sh.pb, sh.low, sh.low_bits);
}

// regions (offset, words) in the order stated: each starts where the one before ends (`packed`) or no earlier
bool in_order(const std::vector<std::pair<size_t, size_t>>& r, bool packed)
{
  size_t end = 0;
  for (const auto& x : r) {
    if (packed ? x.first != end : x.first < end) return false;
    end = x.first + x.second;
  }
  return true;
}

int sweep()
{
  std::vector<uint32_t> Ls = {1, 2, 255, 256, 257};
  for (int k = 0; k <= 24; k++) {
    Ls.push_back(1u << k);
    Ls.push_back((1u << k) + 1);
  }
  const int tabs[] = {0, 1, 13, 14, 15, 16, 17, 18, 19, 20}, bitss[] = {0, 1, 13, 64, 128, 253, 254}, pfs[] = {1, 2, 3, 8};
  uint64_t combos = 0, reached[3] = {0, 0, 0}, errors = 0;
  std::string first[3];
  for (uint32_t L : Ls)
    for (int c_cfg = 0; c_cfg <= 24; c_cfg++)
      for (int tab : tabs)
        for (int bits : bitss)
          for (int pf : pfs)
            for (uint64_t hint : {(uint64_t)0, (uint64_t)L}) {
              const SortShape sh = msm_sort_shape(L, c_cfg, 0, tab, bits, pf, hint);
              auto bad = [&](const char* what) { fail(sh, L, c_cfg, tab, bits, pf, hint, what); };
              combos++;
              const MsmGeom g = msm_geometry_plan(L, c_cfg, tab, bits, pf);
              if (memcmp(&g, &sh.g, sizeof g)) bad("geometry");
              const uint32_t nb = g.NBb * (uint32_t)g.Wb;
              if (sh.nbuckets != nb) bad("nbuckets");
              if (sh.err != ICICLE_SUCCESS) {
                errors++;
                const int idx_bits = g.tab ? g.IB + ilog2_ceil((uint64_t)g.W) : ilog2_ceil((L ? (uint64_t)L : 1) * g.pf);
                if (sh.err != ICICLE_INVALID_ARGUMENT || idx_bits <= 31 || !strstr(sh.msg, "exceed the 31-bit point index of a sort entry")) bad("error");
                continue;
              }
              // threshold and item cap: ≤ entries / CHUNK full chunks and one partial chunk for each of the < entries / thr large buckets
              if (sh.nentries != (uint64_t)L * g.W || sh.large_thr < 64 || sh.item_cap < sh.nentries / MSM_LARGE_CHUNK + sh.nentries / sh.large_thr + 1) bad("threshold or item cap");
              const uint64_t avg3 = ((hint ? hint : g.tab ? (uint64_t)L * g.W : (uint64_t)L * g.pf) / g.NB + 1) * 3; // three times the average bucket, floor 64
              if (sh.large_thr != (avg3 < 64 ? 64 : avg3)) bad("threshold");
              if (sh.nblocks != (nb + SCAN_B - 1) / SCAN_B || sh.om % ORDER_BINS || sh.om < nb || sh.om - nb >= (uint32_t)ORDER_BINS || sh.oblk != sh.om / ORDER_BINS || sh.oscan != (sh.om + SCAN_B - 1) / SCAN_B)
                bad("scan or size-order blocks");
              // ---- first layout: counts … large_items
              const auto& w = sh.ws;
              const size_t np = sh.nparts;
              if (!in_order({{w.counts, nb}, {w.offsets, nb}, {w.cursor, nb}, {w.large_list, nb}, {w.order, nb}, {w.large_first, nb}, {w.n_large, 4}, {w.tickets, TK}, {w.s2tickets, S2TK},
                             {w.bsum, sh.nblocks}, {w.part_count, np}, {w.part_start, np + 1}, {w.part_cursor, np}, {w.blockhist, sh.om}, {w.obsum, sh.oscan}},
                            true) ||
                  w.counts != 0)
                bad("workspace order");
              const size_t head = w.obsum + sh.oscan, items_end = w.large_items + 2 * (size_t)sh.item_cap;
              if (w.large_items < head || w.large_items - head > 1 || (w.large_items & 1)) bad("large_items: behind obsum, 8-byte aligned");
              if (items_end > w.total || w.total - items_end > 2) bad("workspace total");
              // one zeroing run each: counts | offsets | cursor (3·nb), n_large … part_count, and the staged histogram's n_large | tickets | its own
              if (w.cursor + nb != w.counts + 3 * (size_t)nb || w.part_count + np != w.n_large + 4 + TK + S2TK + sh.nblocks + np || w.s2tickets + S2TK != w.n_large + 4 + TK + S2TK) bad("zeroed runs");
              // ---- the paths
              reached[sh.path]++;
              if (first[sh.path].empty()) {
                char buf[160];
                snprintf(buf, sizeof buf, "path %s L=%u c_cfg=%d tab=%d bits=%d pf=%d hint=%llu c=%d W=%d", PATH_NAME[sh.path], L, c_cfg, tab, bits, pf, (unsigned long long)hint, g.c, g.W);
                first[sh.path] = buf;
              }
              if (sh.NP << sh.low_bits != g.NBb || sh.nparts << sh.low_bits != nb || sh.low_bits < 0) bad("partitions");
              if (sh.two_level_ok != (sh.idx_bits + sh.low_bits <= 31 && sh.low_bits <= 7 && np * 8 <= 128 * 1024)) bad("two-level conditions");
              if (sh.path == SORT_TWO_LEVEL && !sh.two_level_ok) bad("two-level path without its conditions");
              if (sh.path == SORT_GLOBAL && sh.two_level_ok) bad("global path where the two-level one fits");
              if (sh.path == SORT_STAGED) {
                const size_t P = (size_t)1 << sh.pb, NL = (size_t)1 << sh.low, R = sh.ntiles;
                if (!g.tab || g.W > 16 || sh.nentries < (1u << 17) || sh.pb > 12 || sh.low < 0 || sh.low > 10 || P * NL != nb || sh.lds_a > S2_LDS_MAX || sh.lds_b > S2_LDS_MAX) bad("staged conditions");
                // what the kernels index: pass A 2P + 1 counters and a tile's entries, pass B 2NL + 1 counters, a row table and a chunk; entries
                // carry low | window | index in tile
                if (sh.lds_a < (2 * P + 1 + (size_t)S2_TILE * g.W) * 4 || sh.lds_b < (2 * NL + 1 + R + 1 + S2_CHUNK) * 4 || S2_LOW_SHIFT + sh.low > 31 || g.W > (1 << (S2_LOW_SHIFT - S2_W_SHIFT)))
                  bad("staged LDS or entry fields");
                if (R != (L + S2_TILE - 1) / S2_TILE || (sh.nentries >> sh.pb) > 28000 || sh.maxchunks < sh.nentries / S2_CHUNK + P) bad("tiles, partition size or chunks");
                const auto& s = sh.s2;
                const size_t n_ch = sh.maxchunks * NL;
                if (!in_order({{s.cnt, R * P}, {s.off, R * P}, {s.partial, S2_RG * P}, {s.pstart, P + 1}, {s.cfirst, P + 1}, {s.chist, n_ch}, {s.coff, n_ch}, {s.bh, ORDER_BINS * P}, {s.keytot, ORDER_BINS}}, true) ||
                    s.cnt != 0 || s.total != s.keytot + ORDER_BINS)
                  bad("staged workspace");
              } else if (sh.s2.total) bad("staged workspace without the staged path");
            }
  for (int k = 0; k < 3; k++) printf("%s\n", first[k].empty() ? "(path not reached)" : first[k].c_str());
  printf("combinations %llu staged %llu two_level %llu global %llu errors %llu failures %d\n", (unsigned long long)combos, (unsigned long long)reached[0], (unsigned long long)reached[1],
         (unsigned long long)reached[2], (unsigned long long)errors, g_failures);
  return g_failures || !reached[0] || !reached[1] || !reached[2] ? 1 : 0;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
  if (argc >= 3 && !strcmp(argv[1], "shape")) {
    for (int k = 2; k < argc; k++) {
      unsigned L;
      int c_cfg, tab, bits, pf;
      unsigned long long hint;
      if (sscanf(argv[k], "%u,%d,%d,%d,%d,%llu", &L, &c_cfg, &tab, &bits, &pf, &hint) != 6) return 2;
      const SortShape sh = msm_sort_shape(L, c_cfg, 0, tab, bits, pf, hint);
      if (sh.err != ICICLE_SUCCESS) printf("error %s\n", sh.msg);
      else printf("%s %d %d %d %d %u\n", PATH_NAME[sh.path], sh.pb, sh.low, sh.g.c, sh.g.W, sh.large_thr);
    }
    return 0;
  }
  fprintf(stderr, "usage: %s sweep | shape L,c_cfg,tab,bits,pf,hint ...\n", argv[0]);
  return 2;
}
