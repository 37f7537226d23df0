// msm_sort_plan.h — the shape of one digit sort, apart from the kernels and the code that launches them (msm_sort.hip), so that
// a host build can walk it over every geometry: tests/msm_sort_plan_check.cpp.
//
//  msm_sort_shape   geometry (msm_recode.h), large-bucket threshold and item cap, the sort path with its partition and LDS
//                   sizes, and both workspaces as named word offsets — or the error msm_sort_run returns
#pragma once
#include <stdio.h>

#include "msm_recode.h"

namespace isnark {

constexpr int SCAN_T = 256, SCAN_E = 8, SCAN_B = SCAN_T * SCAN_E;
constexpr int ORDER_BINS = 256;
constexpr int S2_TILE = 1024;    // scalars per tile (pass A): a row = (tile, all W ≤ 16 windows) stages ≤ 64 KiB of entries in LDS
constexpr int S2_CHUNK = 12288;  // entries per chunk (pass B): 48 KiB of LDS
constexpr int S2_LI_BITS = 10, S2_W_SHIFT = 10, S2_LOW_SHIFT = 14;
// Workgroup size of the three big kernels (partition, chunk histogram, placement): 512 threads when the sort has the GPU to itself
// or shares it with the transforms, 256 (`crowded`) when it runs beside the bucket accumulations — a 512-thread workgroup needs two
// free wave slots with 64 registers each on ALL FOUR SIMDs of a CU at once, and beside three 136-register accumulation waves per
// SIMD (104 registers left) that happens only when waves retire in step: H's sort took 9 ms beside the witness accumulations
// (0.45 ms alone; its partition pass alone 4.9–5.3 ms) and had become what H's accumulation waits for.  One wave per SIMD fits the
// gap: 2.9 ms (profiles/r05_ab_sort_wg256.txt).  The witness sort keeps 512: beside the transforms the smaller groups slow the
// front end by 0.14 ms.
constexpr int S2_THREADS_WIDE = 512, S2_THREADS_CROWDED = 256;
constexpr int S2_RG = 32;        // row groups of the column scan
constexpr int S2_GRP = 16;       // lanes that copy one run
constexpr uint32_t S2_LONG = 192; // a run above this is copied by the whole workgroup
constexpr size_t S2_LDS_MAX = 76 * 1024; // two workgroups per CU; ≤ 66 KiB at the benchmark sizes (room next to one NTT workgroup)
constexpr uint32_t TK = MSM_TICKET_SLOTS * 64;
constexpr uint32_t S2TK = 4; // tickets of the LDS-staged path's own last-workgroup steps (column scan, order scan)

// staged: LDS-staged (table mode, ≥ 2^17 entries: partitions of ≤ 28 K entries, ≤ 1024 buckets each); two-level: partitions in
// global memory, counts and offsets out of the partitions; global: one histogram with an atomic per digit
enum SortPath { SORT_STAGED = 0, SORT_TWO_LEVEL, SORT_GLOBAL };

struct SortShape {
  eIcicleError err; // ≠ ICICLE_SUCCESS: `msg` is the call's error text
  char msg[112];
  MsmGeom g;
  uint32_t nbuckets, large_thr, item_cap;
  uint64_t nentries;
  SortPath path;
  bool two_level_ok; // the two-level path's conditions hold: its scatter buffer is set up, and the staged path uses it when it runs instead
  // bucket index = partition | low bits (≤ 128 buckets per partition; ≤ 8192 partitions: two u32 per partition in LDS)
  int low_bits, idx_bits;
  uint32_t NP, nparts;
  uint32_t nblocks;         // scan blocks over the buckets
  uint32_t oblk, om, oscan; // size-order pass: workgroups, padded bucket count, scan blocks
  // staged path: 2^pb partitions of 2^low buckets, tiles of S2_TILE scalars, chunks of S2_CHUNK entries, dynamic LDS of passes A and B
  int pb, low;
  uint32_t ntiles, maxchunks;
  size_t lds_a, lds_b;
  // workspace of every path, in words: counts … cursor [nbuckets each] | large_list | order | large_first | n_large[4] | tickets[TK] |
  // s2tickets[S2TK] | bsum[nblocks] | part_count[nparts] | part_start[nparts + 1] | part_cursor[nparts] | blockhist[om] | obsum[oscan] |
  // (one word when that leaves large_items odd) | large_items[2·item_cap] (8-byte aligned); `total` is what is allocated
  struct {
    size_t counts, offsets, cursor, large_list, order, large_first, n_large, tickets, s2tickets, bsum, part_count, part_start, part_cursor, blockhist, obsum, large_items, total;
  } ws;
  // the staged path's own: cnt[R][P] | off[R][P] | partial[S2_RG][P] | pstart[P + 1] | cfirst[P + 1] | chist | coff [maxchunks][NL] | order hist [ORDER_BINS][P] | keytot[ORDER_BINS]
  struct {
    size_t cnt, off, partial, pstart, cfirst, chist, coff, bh, keytot, total;
  } s2;
};

inline SortShape msm_sort_shape(uint32_t L, int c_cfg, int lbf, int tab, int bits, int pf, uint64_t entries_hint)
{
  SortShape sh;
  memset(&sh, 0, sizeof sh);
  sh.g = msm_geometry_plan(L, c_cfg, tab, bits, pf);
  const MsmGeom& g = sh.g;
  const uint32_t nb = sh.nbuckets = g.NBb * (uint32_t)g.Wb;
  // Large-bucket threshold.  One thread sums one bucket, so the accumulation kernel lasts as long as its longest chain: buckets
  // with more than `thr` entries go to the workgroup-per-chunk kernels instead.  The reference takes large_bucket_factor (10) ×
  // the average (cuda_msm.cuh:205-220); here the default is 3 × the average with a floor of 64 — uniform scalars have no bucket
  // beyond 2 × the average, while witnesses of real circuits (0/1 wires, bytes, small packed values) put hundreds of entries
  // into the low buckets of the first window: with 10 × / floor 512 the synthetic stand-in circuits spent 2 ms (G1) / 6.5 ms (G2)
  // in 500-addition chains of single threads (prove 11.2 → 6.3 ms at 1.0 M constraints, 14.1 → 8.3 ms at 1.4 M; 1.6 M uniform:
  // unchanged).  The caller's large_bucket_factor (ConfigExtension) is honoured when given.
  constexpr uint32_t large_floor = 64u;
  const uint64_t avg = (entries_hint ? entries_hint : g.tab ? (uint64_t)L * g.W : (uint64_t)L * g.pf) / g.NB + 1;
  uint32_t thr = (uint32_t)(avg * (uint64_t)(lbf > 0 ? lbf : 3));
  if (thr < large_floor) thr = large_floor;
  sh.large_thr = thr;
  sh.nblocks = (nb + SCAN_B - 1) / SCAN_B;
  const uint64_t nentries = sh.nentries = (uint64_t)L * g.W;
  sh.low_bits = (g.c - 1) > 8 ? (g.c - 1) - 8 : 0;
  if (g.tab) {
    sh.low_bits = tab_low_bits(g.c, g.IB, g.W);
    if (sh.low_bits < 0) sh.low_bits = 7; // forced c that does not fit: the two-level test below fails and the global-histogram path runs
  }
  sh.NP = g.NBb >> sh.low_bits;
  const uint32_t nparts = sh.nparts = nb >> sh.low_bits;
  sh.idx_bits = g.tab ? g.IB + ilog2_ceil((uint64_t)g.W) : ilog2_ceil((L ? (uint64_t)L : 1) * g.pf);
  if (sh.idx_bits > 31) {
    snprintf(sh.msg, sizeof sh.msg, "msm: %u scalars x precompute_factor %d exceed the 31-bit point index of a sort entry", L, g.pf);
    sh.err = ICICLE_INVALID_ARGUMENT;
    return sh;
  }
  sh.two_level_ok = sh.idx_bits + sh.low_bits <= 31 && sh.low_bits <= 7 && (size_t)nparts * 8 <= 128 * 1024;
  sh.oblk = (nb + ORDER_BINS - 1) / ORDER_BINS;
  sh.om = sh.oblk * ORDER_BINS;
  sh.oscan = (sh.om + SCAN_B - 1) / SCAN_B;
  // work items of large buckets: ≤ entries/CHUNK full chunks + one partial chunk per large bucket (≤ entries/thr of those)
  sh.item_cap = (uint32_t)(nentries / MSM_LARGE_CHUNK + nentries / thr + 2);
  size_t o = 0;
  auto take = [&o](size_t words) { const size_t at = o; o += words; return at; };
  sh.ws.counts = take(nb); sh.ws.offsets = take(nb); sh.ws.cursor = take(nb); sh.ws.large_list = take(nb); sh.ws.order = take(nb); sh.ws.large_first = take(nb);
  sh.ws.n_large = take(4); sh.ws.tickets = take(TK); sh.ws.s2tickets = take(S2TK); sh.ws.bsum = take(sh.nblocks);
  sh.ws.part_count = take(nparts); sh.ws.part_start = take((size_t)nparts + 1); sh.ws.part_cursor = take(nparts);
  sh.ws.blockhist = take(sh.om); sh.ws.obsum = take(sh.oscan);
  sh.ws.large_items = o + (o & 1);
  sh.ws.total = o + 2 * (size_t)sh.item_cap + 2;

  sh.path = sh.two_level_ok ? SORT_TWO_LEVEL : SORT_GLOBAL;
  if (g.tab && nentries >= (1u << 17) && g.W <= 16) { // (2^20 until round 5: with nine launches the staged path is no slower than the two-level one down to the witness heads and 8-way shards)
    while ((nentries >> sh.pb) > 28000) sh.pb++;
    sh.low = (g.c - 1) - sh.pb;
    if (sh.low > 10) {
      sh.pb += sh.low - 10;
      sh.low = 10;
    }
    sh.ntiles = (L + S2_TILE - 1) / S2_TILE;
    sh.maxchunks = (uint32_t)(nentries / S2_CHUNK) + (1u << sh.pb);
    sh.lds_a = ((size_t)2 * (1u << sh.pb) + 1 + (size_t)S2_TILE * g.W) * 4;
    sh.lds_b = ((size_t)2 * (1u << (sh.low > 0 ? sh.low : 0)) + 1 + sh.ntiles + 1 + S2_CHUNK) * 4;
    if (sh.low >= 0 && sh.pb <= 12 && (1u << sh.pb) * (uint64_t)(1u << sh.low) == nb && sh.lds_a <= S2_LDS_MAX && sh.lds_b <= S2_LDS_MAX && S2_LOW_SHIFT + sh.low <= 31 &&
        (size_t)(1u << sh.pb) * 4 <= 64 * 1024)
      sh.path = SORT_STAGED;
  }
  if (sh.path == SORT_STAGED) {
    const size_t P = (size_t)1 << sh.pb, n_cnt = sh.ntiles * P, n_ch = ((size_t)sh.maxchunks) << sh.low;
    o = 0;
    sh.s2.cnt = take(n_cnt); sh.s2.off = take(n_cnt); sh.s2.partial = take(S2_RG * P); sh.s2.pstart = take(P + 1); sh.s2.cfirst = take(P + 1);
    sh.s2.chist = take(n_ch); sh.s2.coff = take(n_ch); sh.s2.bh = take(ORDER_BINS * P); sh.s2.keytot = take(ORDER_BINS);
    sh.s2.total = o;
  }
  return sh;
}

} // namespace isnark
