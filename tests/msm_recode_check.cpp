// msm_recode_check.cpp — host check of csrc/msm_recode.h: the MSM's host plan (msm_geometry_plan) and the signed-digit recoding
// the sort kernels run per scalar (recode_fe, digit, bucket_id, entry_idx), over every geometry the plan can produce.
// Test infrastructure: a stand-alone program built by tests/test_msm_recode_host.py with g++, once plainly and once with
// -fsanitize=address,undefined.
//
//   msm_recode_check sweep FILE      FILE: one hexadecimal scalar below r per line (the fixed edge values of tests/msm_inputs.py;
//                                    the edges of each geometry's own windows are formed here).  Prints the number of geometries
//                                    and digits checked; the first failures, and exit status 1, when something does not hold.
//   msm_recode_check geom L,c_cfg,tab,bits,pf ...    prints "c W wide tab nbuckets IB Wb" of each, one line per argument
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../icicle-snark_amd/csrc/msm_recode.h"

using namespace isnark;
using bn254::fe;
using bn254::Fr;

namespace {

// ---- integers of 320 bits, little-endian 32-bit limbs: enough for t = s' + H (288 bits) and sums of shifted digits
struct Big {
  uint32_t l[10];
  Big() { memset(l, 0, sizeof l); }
};
Big big_of(const uint32_t* w, int n)
{
  Big b;
  for (int i = 0; i < n; i++) b.l[i] = w[i];
  return b;
}
int big_cmp(const Big& a, const Big& b)
{
  for (int i = 9; i >= 0; i--)
    if (a.l[i] != b.l[i]) return a.l[i] < b.l[i] ? -1 : 1;
  return 0;
}
Big big_add(const Big& a, const Big& b)
{
  Big r;
  uint64_t c = 0;
  for (int i = 0; i < 10; i++) {
    c += (uint64_t)a.l[i] + b.l[i];
    r.l[i] = (uint32_t)c;
    c >>= 32;
  }
  return r;
}
Big big_sub(const Big& a, const Big& b) // a ≥ b
{
  Big r;
  int64_t c = 0;
  for (int i = 0; i < 10; i++) {
    c += (int64_t)a.l[i] - b.l[i];
    r.l[i] = (uint32_t)c;
    c >>= 32;
  }
  return r;
}
Big big_shl(uint64_t v, int bit) // v · 2^bit, v < 2^32
{
  Big r;
  const int limb = bit >> 5, off = bit & 31;
  const uint64_t x = v << off;
  if (limb < 10) r.l[limb] = (uint32_t)x;
  if (limb + 1 < 10) r.l[limb + 1] = (uint32_t)(x >> 32);
  return r;
}
bool big_zero_from(const Big& a, int bit) // a >> bit == 0
{
  for (int b = bit; b < 320; b++)
    if (a.l[b >> 5] >> (b & 31) & 1) return false;
  return true;
}
Big modulus() { return big_of(bn254::FrP::MOD, 8); }
Big half() // (r − 1) / 2
{
  Big h = modulus();
  h.l[0] -= 1;
  for (int i = 0; i < 10; i++) h.l[i] = (h.l[i] >> 1) | (i < 9 ? h.l[i + 1] << 31 : 0);
  return h;
}
Big pow2_mod_r(int k) // doubling from 1, a conditional subtraction each step
{
  Big x, r = modulus();
  x.l[0] = 1;
  for (int i = 0; i < k; i++) {
    x = big_add(x, x);
    if (big_cmp(x, r) >= 0) x = big_sub(x, r);
  }
  return x;
}
fe fe_of(const Big& b)
{
  fe v;
  for (int i = 0; i < 8; i++) v.l[i] = b.l[i];
  return v;
}
std::string hex_of(const Big& b)
{
  char buf[96];
  std::string s;
  for (int i = 9; i >= 0; i--) {
    snprintf(buf, sizeof buf, "%08x", b.l[i]);
    s += buf;
  }
  return s;
}

struct Window {
  int bit, cw;
};
std::vector<Window> windows_of(const MsmGeom& g)
{
  std::vector<Window> w;
  for (int k = 0; k < g.W; k++) w.push_back(k < g.wide ? Window{k * g.c, g.c} : Window{g.wide * g.c + (k - g.wide) * (g.c - 1), g.c - 1});
  return w;
}

int g_failures = 0;
void fail(const MsmGeom& g, uint32_t L, int bits, const char* what, const std::string& detail)
{
  if (g_failures++ < 10)
    fprintf(stderr, "FAIL %s: L=%u bits=%d c=%d W=%d wide=%d tab=%d IB=%d pf=%d nbms=%d  %s\n", what, L, bits, g.c, g.W, g.wide, g.tab, g.IB, g.pf, g.nbms, detail.c_str());
}

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint64_t next64() // splitmix64
{
  uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
Big random_below(int bits) // uniform over [0, min(2^bits, r))
{
  const Big r = modulus();
  for (;;) {
    Big x;
    for (int i = 0; i < 8; i += 2) {
      const uint64_t v = next64();
      x.l[i] = (uint32_t)v;
      x.l[i + 1] = (uint32_t)(v >> 32);
    }
    for (int b = bits; b < 256; b++) x.l[b >> 5] &= ~(1u << (b & 31));
    if (big_cmp(x, r) < 0) return x;
  }
}

// one scalar through recode_fe / digit / bucket_id against the integers
uint64_t check_scalar(const MsmGeom& g, uint32_t L, int bits, const std::vector<Window>& win, uint32_t nbuckets, const Big& s)
{
  const Big r = modulus(), h = half();
  const bool want_neg = big_cmp(s, h) > 0;
  const Big sp = want_neg ? big_sub(r, s) : s;
  uint32_t t[9], neg = 9, tm[9], negm = 9;
  recode_fe(fe_of(s), g, 0, t, neg);
  recode_fe(Fr::to_mont(fe_of(s)), g, 1, tm, negm);
  if (neg != (want_neg ? 1u : 0u)) fail(g, L, bits, "sign", hex_of(s));
  if (negm != neg || memcmp(t, tm, sizeof t)) fail(g, L, bits, "Montgomery-form scalar recodes differently", hex_of(s));
  const int top = win.back().bit + win.back().cw;
  if (!big_zero_from(big_of(t, 9), top)) fail(g, L, bits, "bits above the top window", hex_of(s));
  Big pos, negsum;
  for (int w = 0; w < g.W; w++) {
    const uint32_t d = digit(t, w, g);
    const uint32_t mag = d & 0x7fffffffu;
    if (mag > (1u << (win[w].cw - 1))) fail(g, L, bits, "digit beyond its window", hex_of(s));
    if (!mag) continue;
    if (d >> 31) negsum = big_add(negsum, big_shl(mag, win[w].bit));
    else pos = big_add(pos, big_shl(mag, win[w].bit));
    if (bucket_id(g, w, mag - 1) >= nbuckets) fail(g, L, bits, "bucket beyond the bucket array", hex_of(s));
  }
  if (big_cmp(pos, negsum) < 0 || big_cmp(big_sub(pos, negsum), sp) != 0) fail(g, L, bits, "digits do not sum to s'", hex_of(s));
  return (uint64_t)g.W;
}

int sweep(const char* path)
{
  std::vector<Big> fixed;
  FILE* f = fopen(path, "r");
  if (!f) {
    fprintf(stderr, "cannot read %s\n", path);
    return 2;
  }
  char line[256];
  while (fgets(line, sizeof line, f)) {
    Big b;
    int n = 0;
    for (char* p = line; *p; p++) n += (*p >= '0' && *p <= '9') || (*p >= 'a' && *p <= 'f');
    if (!n || n > 64) continue;
    int k = 0;
    for (char* p = line + strlen(line); p-- > line;) {
      const int v = *p >= '0' && *p <= '9' ? *p - '0' : *p >= 'a' && *p <= 'f' ? *p - 'a' + 10 : -1;
      if (v < 0) continue;
      b.l[k >> 3] |= (uint32_t)v << (4 * (k & 7));
      k++;
    }
    if (big_cmp(b, modulus()) < 0) fixed.push_back(b);
  }
  fclose(f);
  if (fixed.size() < 20) {
    fprintf(stderr, "%s holds %zu values\n", path, fixed.size());
    return 2;
  }
  std::vector<uint32_t> Ls = {1, 2, 255, 256, 257};
  for (int k = 0; k <= 24; k++) {
    Ls.push_back(1u << k);
    Ls.push_back((1u << k) + 1);
  }
  const int tabs[] = {0, 1, 13, 14, 15, 16, 17, 18, 19, 20}, bitss[] = {0, 1, 13, 64, 128, 253, 254}, pfs[] = {1, 2, 3, 8};
  std::set<std::tuple<int, int, int, int, int, int, int, int>> done;
  uint64_t combos = 0, geoms = 0, scalars = 0, digits = 0, narrowed_all = 0;
  for (uint32_t L : Ls)
    for (int c_cfg = 0; c_cfg <= 24; c_cfg++)
      for (int tab : tabs)
        for (int bits : bitss)
          for (int pf : pfs) {
            const MsmGeom g = msm_geometry_plan(L, c_cfg, tab, bits, pf);
            const int eff = bits <= 0 || bits > 254 ? 254 : bits;
            combos++;
            // ---- the plan itself
            if (g.c < 4 || g.c > 20 || g.W < 1 || g.W > 64 || g.wide < 0 || g.wide > g.W || (g.wide < g.W && g.c < 3)) {
              fail(g, L, bits, "geometry out of range", "");
              continue;
            }
            const std::vector<Window> win = windows_of(g);
            const int top = win.back().bit + win.back().cw;
            if (top < eff) fail(g, L, bits, "the windows do not cover the scalar", "");
            if (top > 288) fail(g, L, bits, "the windows pass t's nine limbs", "");
            Big H;
            for (const Window& w : win) H = big_add(H, big_shl(1, w.bit + w.cw - 1));
            if (big_cmp(H, big_of(g.H, 9)) != 0) fail(g, L, bits, "H is not one bit per window", hex_of(big_of(g.H, 9)));
            const uint32_t nbuckets = g.NBb * (uint32_t)g.Wb;
            if (g.NB != 1u << (g.c - 1) || g.nbms != (g.W + g.pf - 1) / g.pf || nbuckets != (g.tab ? g.NB : (uint32_t)g.nbms * g.NB)) fail(g, L, bits, "bucket layout", "");
            if (g.tab && (eff != 254 || pf > 1 || c_cfg > 0 || !tab || g.pf != 1 || g.IB != ilog2_ceil(L ? L : 1))) fail(g, L, bits, "table mode where it does not belong", "");
            // the sort entry: point index (and window, in table mode) below the sign bit, each field recoverable
            for (uint32_t i : {0u, L - 1})
              for (int w : {0, g.W - 1}) {
                const uint32_t e = entry_idx(g, w, i);
                bool ok = e < (1u << 31);
                if (g.tab) ok = ok && (e & ((1u << g.IB) - 1)) == i && (e >> g.IB) == (uint32_t)w && tab_low_bits(g.c, g.IB, g.W) >= 0;
                else ok = ok && e == (g.pf > 1 ? i * (uint32_t)g.pf + (uint32_t)(w / g.nbms) : i) && (g.pf == 1 || e < (uint64_t)L * g.pf);
                if (!ok) fail(g, L, bits, "sort entry", std::to_string(e));
              }
            // ---- the recoding, once per distinct geometry and scalar width
            if (!done.insert(std::make_tuple(g.c, g.W, g.wide, g.tab, g.tab ? g.IB : 0, g.pf, g.nbms, eff)).second) continue;
            geoms++;
            if (g.wide == 0) narrowed_all++;
            std::vector<Big> vals = fixed;
            for (const Window& w : win)
              for (int kind = 0; kind < 3; kind++) {
                Big v = pow2_mod_r(kind == 0 ? w.bit : w.bit + w.cw - 1);
                if (kind == 2) {
                  Big one;
                  one.l[0] = 1;
                  v = big_cmp(v, one) >= 0 ? big_sub(v, one) : big_sub(modulus(), one);
                }
                vals.push_back(v);
                Big zero;
                vals.push_back(big_cmp(v, zero) ? big_sub(modulus(), v) : v);
              }
            for (int k = 0; k < 4096; k++) vals.push_back(random_below(eff));
            for (const Big& s : vals) {
              if (eff < 254 && !big_zero_from(s, eff)) continue; // the caller's promise: every scalar is below 2^bits
              digits += check_scalar(g, L, bits, win, nbuckets, s);
              scalars++;
            }
          }
  printf("combinations %llu geometries %llu scalars %llu digits %llu all_windows_narrowed %llu failures %d\n", (unsigned long long)combos, (unsigned long long)geoms,
         (unsigned long long)scalars, (unsigned long long)digits, (unsigned long long)narrowed_all, g_failures);
  return g_failures ? 1 : 0;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc >= 3 && !strcmp(argv[1], "sweep")) return sweep(argv[2]);
  if (argc >= 3 && !strcmp(argv[1], "geom")) {
    for (int k = 2; k < argc; k++) {
      unsigned L;
      int c_cfg, tab, bits, pf;
      if (sscanf(argv[k], "%u,%d,%d,%d,%d", &L, &c_cfg, &tab, &bits, &pf) != 5) return 2;
      const MsmGeom g = msm_geometry_plan(L, c_cfg, tab, bits, pf);
      printf("%d %d %d %d %u %d %d\n", g.c, g.W, g.wide, g.tab, g.NBb * (uint32_t)g.Wb, g.IB, g.Wb);
    }
    return 0;
  }
  fprintf(stderr, "usage: %s sweep FILE | geom L,c_cfg,tab,bits,pf ...\n", argv[0]);
  return 2;
}
