// ntt_plan_check.cpp — host check of csrc/ntt_plan.h: the plan ntt.hip enqueues for a transform (ntt_plan, plan29, bounds29), over
// every size, domain, direction, batch and kernel family.
// Test infrastructure: a stand-alone program built by tests/test_ntt_plan_host.py with g++, once plainly and once with
// -fsanitize=address,undefined.
//
//   ntt_plan_check sweep    every plan: bits, LDS, grid, the load and store maps as bijections, the radix-2^29 bounds level by level
//                           as the kernels consume them, and — up to 2^17 — the plan EXECUTED on the host over the 31-bit prime
//                           2013265921 and held against the direct DFT.  Prints the counts; failures first, and exit status 1.
//   ntt_plan_check table    one line per log n and direction: family, bits, tiles, shrink_last and end bound per pass, and the
//                           smallest batch-3 log n with the one-dimensional grid
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../icicle-snark_amd/csrc/ntt_plan.h"

using namespace isnark::ntt;

namespace {

constexpr uint64_t Q = 2013265921ull; // 15·2^27 + 1; 31 generates its multiplicative group
constexpr int Q_LOG = 27;
uint64_t mulq(uint64_t a, uint64_t b) { return a * b % Q; }
uint64_t powq(uint64_t a, uint64_t e)
{
  uint64_t r = 1;
  for (; e; e >>= 1, a = mulq(a, a))
    if (e & 1) r = mulq(r, a);
  return r;
}

int g_failures = 0;
void fail(int logn, int dom, bool inverse, int batch, bool allow29, const char* what, const std::string& detail = "")
{
  if (g_failures++ < 12) fprintf(stderr, "FAIL %s: logn=%d domain=%d inverse=%d batch=%d allow29=%d  %s\n", what, logn, dom, (int)inverse, batch, (int)allow29, detail.c_str());
}

uint64_t tiles_of(const PassParams& p, int logn) { return (1ull << logn) >> (p.log_r + p.log_c); }

// position of element (tile b, row r, column c) in a pass's source (store = false) or destination
uint64_t pos_of(const PassParams& p, uint64_t b, uint64_t r, uint64_t c, bool store)
{
  const uint64_t b_hi = b >> p.tiles_per_group_log, b_lo = b & ((1ull << p.tiles_per_group_log) - 1);
  return store ? b_hi * p.out_hi + b_lo * p.out_lo + r * p.out_row + c * p.out_col : b_hi * p.in_hi + b_lo * p.in_lo + r * p.in_row + c * p.in_col;
}
// the four fields (b_hi, b_lo, r, c) have power-of-two strides whose bit ranges tile [0, logn): the map permutes bits.  Holds for
// every size; the enumeration below confirms it element by element up to 2^20.
bool bit_ranges_tile(const PassParams& p, int logn, bool store)
{
  const uint64_t tiles = tiles_of(p, logn);
  const int hi_bits = ilog2(tiles) - (int)p.tiles_per_group_log;
  const uint64_t stride[4] = {store ? p.out_hi : p.in_hi, store ? p.out_lo : p.in_lo, store ? p.out_row : p.in_row, store ? p.out_col : p.in_col};
  const int bits[4] = {hi_bits, (int)p.tiles_per_group_log, p.log_r, p.log_c};
  uint64_t seen = 0;
  for (int k = 0; k < 4; k++) {
    if (bits[k] < 0) return false;
    if (!bits[k]) continue;
    if (!stride[k] || (stride[k] & (stride[k] - 1))) return false;
    const uint64_t m = ((1ull << bits[k]) - 1) * stride[k];
    if (seen & m) return false;
    seen |= m;
  }
  return seen == (1ull << logn) - 1;
}
bool enumerated_bijection(const PassParams& p, int logn, bool store)
{
  const uint64_t n = 1ull << logn, tiles = tiles_of(p, logn), R = 1ull << p.log_r, C = 1ull << p.log_c;
  std::vector<bool> hit(n, false);
  for (uint64_t b = 0; b < tiles; b++)
    for (uint64_t r = 0; r < R; r++)
      for (uint64_t c = 0; c < C; c++) {
        const uint64_t at = pos_of(p, b, r, c, store);
        if (at >= n || hit[at]) return false;
        hit[at] = true;
      }
  return tiles * R * C == n;
}

// the bounds of one radix-2^29 pass, level by level as ntt_pass29_kernel consumes b0, bs and shrink_last (k_mid, k_last): values are
// below B·r; a level's borrow-proof constant K must cover its subtrahends (K − 1 ≥ B); sums and the multiplied differences of a
// round that is not the last stay below 2B, the last round's unmultiplied differences below B + K.  fr29.h: K ≤ 1300 (sub), and a value
// stays below 2^264 ≈ 1354·r (mul, shrink).  Returns the end bound, 0 on a miss.
uint32_t walk_bounds(const Plan29& pl, int log_r, uint32_t b_in, std::string* why)
{
  if (pl.b0 < b_in) return *why = "b0 below the bound of what the pass loads", 0;
  uint32_t B = pl.b0;
  int log_m = log_r;
  for (; log_m > 3; log_m -= 3)
    for (int l = log_r - log_m; l < log_r - log_m + 3; l++) {
      const uint32_t K = (pl.b0 << l) + 1u; // k_mid
      if (K - 1 < B || K > 1300) return *why = "k_mid", 0;
      B *= 2;
    }
  if (pl.shrink_last) {
    if (B >= 1354) return *why = "shrink beyond its range", 0;
    B = (uint32_t)(((uint64_t)B * 244 + 999) / 1000) + 1; // fr29::shrink: below 0.244·a + 1
  }
  if (pl.bs < B) return *why = "bs below the bound at the last round", 0;
  B = pl.bs;
  for (int t = 0; t < log_m; t++) {
    const uint32_t K = (pl.bs + 1u) << t; // k_last
    if (K - 1 < B || K > 1300 || B + K >= 1354) return *why = "k_last", 0;
    B += K;
  }
  return B;
}

// ---- the plan run on the host: what a tile does, restated — an R-point DFT down the rows with ω = table[stage_stride], output row k
// times table[k·(b_lo·C + c)·tw_mul], stored at the store map; table[e] = ω_N^e, read at N − e by an inverse transform
struct Table {
  uint64_t gen;
  uint32_t mask;
  bool inverse;
  uint64_t at(uint32_t e) const { return powq(gen, inverse ? ((mask + 1 - e) & mask) : (e & mask)); }
};
void run_pass(const PassParams& p, int logn, const Table& T, const std::vector<uint64_t>& src, std::vector<uint64_t>& dst)
{
  const uint64_t tiles = tiles_of(p, logn), R = 1ull << p.log_r, C = 1ull << p.log_c;
  std::vector<uint64_t> wp(R), col(R), tw_row;
  wp[0] = 1;
  const uint64_t w = T.at(p.stage_stride);
  for (uint64_t j = 1; j < R; j++) wp[j] = mulq(wp[j - 1], w);
  const uint64_t ninv = powq((1ull << logn) % Q, Q - 2);
  for (uint64_t b = 0; b < tiles; b++) {
    const uint32_t b_lo = (uint32_t)(b & ((1ull << p.tiles_per_group_log) - 1));
    for (uint64_t c = 0; c < C; c++) {
      for (uint64_t r = 0; r < R; r++) col[r] = src[pos_of(p, b, r, c, false)];
      // ω_N^(step·k) by repeated multiplication: one table read per column
      const uint32_t step = (uint32_t)((b_lo << p.log_c) + c) * p.tw_mul;
      const uint64_t tstep = p.tw_mul ? T.at(step) : 1;
      uint64_t tk = 1;
      for (uint64_t k = 0; k < R; k++) {
        uint64_t y = 0;
        for (uint64_t r = 0; r < R; r++) y = (y + col[r] * wp[(r * k) & (R - 1)]) % Q;
        y = mulq(y, tk);
        if (p.scale) y = mulq(y, ninv);
        dst[pos_of(p, b, k, c, true)] = y;
        tk = mulq(tk, tstep);
      }
    }
  }
}
bool run_plan(const Plan& pl, int logn, int dom, bool inverse)
{
  const uint64_t n = 1ull << logn;
  const Table T = {powq(31, (Q - 1) >> dom), (uint32_t)((1ull << dom) - 1), inverse};
  std::vector<uint64_t> buf[3] = {std::vector<uint64_t>(n), std::vector<uint64_t>(pl.need_scratch ? n : 0), std::vector<uint64_t>(n)};
  uint64_t seed = 0x9e3779b97f4a7c15ull * (uint64_t)(logn + 1);
  for (uint64_t& v : buf[BUF_IN]) {
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    v = (seed >> 33) % Q;
  }
  for (int pi = 0; pi < pl.np; pi++) {
    const Pass& ps = pl.pass[pi];
    if (ps.src == ps.dst) { // a tile stores where it loaded (the middle pass of three): run it on a copy
      const std::vector<uint64_t> copy = buf[ps.src];
      run_pass(ps.p, logn, T, copy, buf[ps.dst]);
    } else run_pass(ps.p, logn, T, buf[ps.src], buf[ps.dst]);
  }
  // direct DFT, natural order in and out, at sampled outputs
  const uint64_t wn = T.at((uint32_t)((1ull << dom) >> logn) & T.mask), ninv = powq(n % Q, Q - 2);
  for (int smp = 0; smp < 12; smp++) {
    const uint64_t k = smp == 0 ? 0 : smp == 1 ? n - 1 : smp == 2 ? n / 2 : (0x2545f4914f6cdd1dull * (uint64_t)(smp + logn)) & (n - 1);
    const uint64_t wk = powq(wn, k);
    uint64_t acc = 0, x = 1;
    for (uint64_t j = 0; j < n; j++) {
      acc = (acc + buf[BUF_IN][j] * x) % Q;
      x = mulq(x, wk);
    }
    if (inverse) acc = mulq(acc, ninv);
    if (buf[BUF_OUT][k] != acc) return false;
  }
  return true;
}

struct Counts {
  uint64_t plans = 0, passes = 0, enumerated = 0, executed = 0, bound_walks = 0, errors = 0;
};

void check_plan(const Plan& pl, int logn, int dom, bool inverse, int batch, bool allow29, FuseKind fuse, Counts& n)
{
  auto bad = [&](const char* what, const std::string& d = "") { fail(logn, dom, inverse, batch, allow29, what, d); };
  n.plans++;
  if (pl.np < 1 || pl.np > 3) return bad("number of passes");
  int bits = 0;
  for (int pi = 0; pi < pl.np; pi++) bits += pl.pass[pi].p.log_r;
  if (bits != logn) bad("the passes' bits do not sum to log n");
  if (pl.need_scratch != (pl.np > 1)) bad("scratch");
  for (int pi = 0; pi < pl.np; pi++) {
    const Pass& ps = pl.pass[pi];
    const PassParams& p = ps.p;
    const bool last = pi == pl.np - 1;
    n.passes++;
    if (ps.src != (pi == 0 ? BUF_IN : BUF_SCRATCH) || ps.dst != (last ? BUF_OUT : BUF_SCRATCH)) bad("buffers");
    if (p.scale_tab || p.scale_stride) bad("a pointer in the plan");
    if (ps.lds > 160 * 1024 || (pl.use29 && 2 * (uint64_t)ps.lds > 160 * 1024)) bad("dynamic LDS");
    const uint64_t tiles = tiles_of(p, logn);
    if (ps.grid_x >= (1u << 31) || !ps.grid_x || (uint64_t)ps.grid_x * ps.grid_y != tiles * (ps.fused ? 1 : (uint64_t)batch)) bad("grid");
    if (p.xcd_batch && (!pl.use29 || ps.fused || ps.grid_y != 1 || p.xcd_batch != (uint32_t)batch || tiles % 8)) bad("one-dimensional grid where the kernel cannot read it");
    if (ps.fused != (last && fuse == FUSE_ABC) || ps.scale_tab != (last && fuse == FUSE_SCALE_TAB && inverse) || p.fuse_abc != (int)ps.fused) bad("fusion on the wrong pass");
    if (p.scale != (int)(last && inverse) || p.inverse != (int)inverse || p.batch_stride != 1ull << logn) bad("direction, scale or batch stride");
    if (pl.use29 && p.log_r + p.log_c != LOG_TILE) bad("a radix-2^29 pass without a full tile");
    for (const bool store : {false, true})
      if (!bit_ranges_tile(p, logn, store)) bad(store ? "store map" : "load map", "bit ranges");
    if (pl.use29) {
      std::string why;
      const uint32_t limit = !last || inverse ? 506u : 598u, end = walk_bounds(ps.pl29, p.log_r, pi == 0 ? 1u : 4u, &why);
      n.bound_walks++;
      if (!end || end > limit) bad("radix-2^29 bounds", why + " end " + std::to_string(end));
    }
  }
}

int sweep()
{
  Counts n;
  for (int logn = 0; logn <= 27; logn++) {
    int doms[3] = {logn, logn + 3 > Q_LOG ? Q_LOG : logn + 3, Q_LOG};
    for (int di = 0; di < 3; di++) {
      if (di && doms[di] == doms[di - 1]) continue;
      for (const bool inverse : {false, true})
        for (const bool allow29 : {true, false}) {
          for (int batch = 1; batch <= 3; batch++)
            for (const FuseKind fuse : {FUSE_NONE, FUSE_SCALE_TAB, FUSE_ABC}) {
              const Plan pl = ntt_plan(logn, doms[di], batch, inverse, allow29, true, fuse, false, false);
              const bool admitted = fuse != FUSE_ABC || (logn >= 12 && batch == 3 && !inverse); // ntt_fusable, and what the epilogue is for
              if (pl.err != ICICLE_SUCCESS) {
                n.errors++;
                if (admitted && logn >= 11 && logn <= 24) fail(logn, doms[di], inverse, batch, allow29, "plan error", pl.msg);
                static const char no_bounds[] = "ntt: internal error — no radix-2^29 bound plan for a ";
                if (fuse == FUSE_ABC ? pl.err != ICICLE_INVALID_ARGUMENT || strcmp(pl.msg, "ntt: fused epilogue needs a forward batch-of-3 transform with full tiles")
                                     : pl.err != ICICLE_UNKNOWN_ERROR || strncmp(pl.msg, no_bounds, sizeof no_bounds - 1))
                  fail(logn, doms[di], inverse, batch, allow29, "error code or text", pl.msg);
                continue;
              }
              if (fuse == FUSE_ABC && (batch != 3 || inverse)) fail(logn, doms[di], inverse, batch, allow29, "fused epilogue admitted");
              if (pl.use29 != (allow29 && logn >= 11 && logn <= 24)) fail(logn, doms[di], inverse, batch, allow29, "kernel family");
              check_plan(pl, logn, doms[di], inverse, batch, allow29, fuse, n);
            }
          // the maps and the arithmetic depend on neither batch nor fusion: once per size, domain, direction and family
          const Plan pl = ntt_plan(logn, doms[di], 1, inverse, allow29, true, FUSE_NONE, false, false);
          if (di == 0 && !inverse && logn <= 20)
            for (int pi = 0; pi < pl.np; pi++)
              for (const bool store : {false, true}) {
                n.enumerated++;
                if (!enumerated_bijection(pl.pass[pi].p, logn, store)) fail(logn, doms[di], inverse, 1, allow29, store ? "store map" : "load map", "enumeration");
              }
          if (logn <= 17) {
            n.executed++;
            if (!run_plan(pl, logn, doms[di], inverse)) fail(logn, doms[di], inverse, 1, allow29, "the executed plan is not the DFT in natural order");
          }
        }
    }
    // without the radix-2^29 twiddles the 8×32-bit plan runs whatever is allowed; rev_out and cols only bar the epilogue
    if (ntt_plan(logn, Q_LOG, 3, false, true, false, FUSE_NONE, false, false).use29) fail(logn, Q_LOG, false, 3, true, "radix-2^29 without its twiddles");
    if (ntt_plan(logn, Q_LOG, 3, false, true, true, FUSE_ABC, true, false).err == ICICLE_SUCCESS || ntt_plan(logn, Q_LOG, 3, false, true, true, FUSE_ABC, false, true).err == ICICLE_SUCCESS)
      fail(logn, Q_LOG, false, 3, true, "fused epilogue into a relaid output");
  }
  printf("plans %llu passes %llu enumerated_maps %llu executed %llu bound_walks %llu plan_errors %llu failures %d\n", (unsigned long long)n.plans, (unsigned long long)n.passes,
         (unsigned long long)n.enumerated, (unsigned long long)n.executed, (unsigned long long)n.bound_walks, (unsigned long long)n.errors, g_failures);
  return g_failures ? 1 : 0;
}

int table()
{
  int first_xcd = -1;
  for (int logn = 0; logn <= 27; logn++) {
    for (const bool inverse : {false, true}) {
      const Plan pl = ntt_plan(logn, 27, 1, inverse, true, true, FUSE_NONE, false, false);
      printf("%d %s %s", logn, inverse ? "inverse" : "forward", pl.use29 ? "29" : "8x32");
      for (int pi = 0; pi < pl.np; pi++) {
        const Pass& ps = pl.pass[pi];
        std::string why;
        printf(" %d:%llu", ps.p.log_r, (unsigned long long)tiles_of(ps.p, logn));
        if (pl.use29) printf(":%d:%u", ps.pl29.shrink_last, walk_bounds(ps.pl29, ps.p.log_r, pi == 0 ? 1u : 4u, &why));
      }
      printf("\n");
    }
    const Plan b3 = ntt_plan(logn, 27, 3, false, true, true, FUSE_NONE, false, false), b1 = ntt_plan(logn, 27, 1, false, true, true, FUSE_NONE, false, false);
    bool any = false;
    for (int pi = 0; pi < b3.np; pi++) any = any || b3.pass[pi].p.xcd_batch;
    for (int pi = 0; pi < b1.np; pi++)
      if (b1.pass[pi].p.xcd_batch) return 1; // never at batch 1
    if (any && first_xcd < 0) first_xcd = logn;
  }
  printf("first_xcd_batch %d\n", first_xcd);
  return 0;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
  if (argc == 2 && !strcmp(argv[1], "table")) return table();
  fprintf(stderr, "usage: %s sweep | table\n", argv[0]);
  return 2;
}
