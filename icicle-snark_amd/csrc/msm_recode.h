// msm_recode.h — the arithmetic of the MSM's signed-digit recoding and its host plan, apart from the kernels that use it
// (msm_sort.hip), so that a host build can run it over every geometry: tests/msm_recode_check.cpp.
//
//  recode_fe   s ↦ t = s' + H and the sign: scalars above (r − 1)/2 are negated first (s' = r − s, sign flipped), and
//              H = Σ_w 2^(bit_w + cw − 1) makes the digits d_w = ((t >> bit_w) & (2^cw − 1)) − 2^(cw − 1) independent per window
//  digit       d_w of a recoded scalar: windows w < wide are c bits wide at bit c·w, the others c − 1 bits at
//              c·wide + (c − 1)(w − wide) (MsmGeom.wide, msm_plan.h)
//  bucket_id / entry_idx   where a digit lands and how its sort entry names the point, per layout
//  msm_geometry_plan       the host plan: digit width, windows, layout and H for a length-L MSM (msm_geometry, msm_plan.h)
#pragma once
#include <string.h>

#include "msm_plan.h"

namespace isnark {

// scalar → t = s' + H (9 limbs), neg = (s was replaced by r − s)
FF_HD void recode_fe(bn254::fe s, const MsmGeom& g, int mont, uint32_t t[9], uint32_t& neg)
{
  using bn254::Fr;
  if (mont) s = Fr::from_mont(s);
  // s > (r − 1)/2 is replaced by r − s: the value recoded is then ≤ (r − 1)/2 < 0.756·2^253, which leaves the top window —
  // exactly the scalar's last bits in table mode — room for its half-range offset and a carry
  constexpr uint32_t HALF[8] = {0xf8000000u, 0xa1f0fac9u, 0x3cdcb848u, 0x9419f424u, 0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u};
  neg = 0;
  bool decided = false;
#pragma unroll
  for (int k = 7; k >= 0; k--) {
    if (!decided && s.l[k] != HALF[k]) {
      neg = s.l[k] > HALF[k] ? 1u : 0u;
      decided = true;
    }
  }
  if (neg) s = Fr::neg(s);
  uint64_t c = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    c += (uint64_t)s.l[k] + g.H[k];
    t[k] = (uint32_t)c;
    c >>= 32;
  }
  t[8] = (uint32_t)c + g.H[8];
}
// signed digit of window w: 0 for a zero digit, else |d| with the sign in bit 31
FF_HD uint32_t digit(const uint32_t t[9], int w, const MsmGeom& g)
{
  const int cw = w < g.wide ? g.c : g.c - 1;
  const int bit = w < g.wide ? w * g.c : g.wide * g.c + (w - g.wide) * (g.c - 1);
  const int limb = bit >> 5, off = bit & 31;
  uint64_t v = t[limb];
  if (limb < 8) v |= (uint64_t)t[limb + 1] << 32;
  const uint32_t raw = (uint32_t)(v >> off) & ((1u << cw) - 1);
  const int32_t d = (int32_t)raw - (int32_t)(1u << (cw - 1));
  if (d == 0) return 0;
  return d < 0 ? ((uint32_t)(-d) | 0x80000000u) : (uint32_t)d;
}

// bucket of digit magnitude bk+1 of window w, and the entry that names the point
// (classic layout with precomputed bases: window w uses multiple j = w / nbms of the base and the bucket set w mod nbms)
FF_HD uint32_t bucket_id(const MsmGeom& g, int w, uint32_t bk)
{
  if (g.tab) return bk;
  const int wm = g.pf > 1 ? w % g.nbms : w;
  return (uint32_t)wm * g.NB + bk;
}
FF_HD uint32_t entry_idx(const MsmGeom& g, int w, uint32_t i)
{
  if (g.tab) return i | ((uint32_t)w << g.IB);
  return g.pf > 1 ? i * (uint32_t)g.pf + (uint32_t)(w / g.nbms) : i;
}

inline int ilog2_ceil(uint64_t x)
{
  int l = 0;
  while ((1ull << l) < x) l++;
  return l;
}

// Table mode: low bucket bits carried in the 32-bit entries of the two-level sort (partitions = buckets >> low).  8192
// partitions (64 KiB of LDS cursors in the partition pass) as a rule; 16384 (128 KiB, one workgroup per CU) when only
// that lets the entry — point index | window | low bucket bits | sign — fit: 3.2 M constraints keep c = 20 / 13 digits
// instead of c = 19 / 14.  −1: does not fit.
inline int tab_low_bits(int c, int ib, int W)
{
  for (int pb = 13; pb <= 14; pb++) {
    int low = (c - 1) - pb;
    if (low < 0) low = 0;
    if (low > 7) continue;
    if (ib + ilog2_ceil((uint64_t)W) + low <= 31) return low;
  }
  return -1;
}

inline MsmGeom msm_geometry_plan(uint32_t L, int c_cfg, int tab, int bits, int pf)
{
  if (bits <= 0 || bits > 254) bits = 254;
  if (pf < 1) pf = 1;
  if (bits != 254 || pf > 1) tab = 0; // the table mode belongs to the prover's cached keys: full-width scalars, own tables
  // window size: as the reference, ≈ log2(L) − 4 (cuda_msm.cuh:45-48), capped so that bucket magnitudes fit
  // 15 bits + sign
  MsmGeom g;
  memset(&g, 0, sizeof g);
  int c = c_cfg > 0 ? c_cfg : ilog2_ceil(L ? L : 1) - 4;
  if (c < 4) c = 4;
  if (c > 16) c = 16;
  if (tab) {
    // one bucket set: as many buckets as the classic layout has over all its windows (≈ 2^(c+3)) → digits up to 4 bits
    // wider; the widest digit whose entry (point index | window | low bucket bits | sign) still fits 32 bits is taken
    const int ib = ilog2_ceil(L ? L : 1);
    int ct = 0;
    if (c_cfg <= 0) {
      for (int t = c + 4 > 20 ? 20 : c + 4; t > c; t--) {
        if (tab_low_bits(t, ib, 254 / t + 1) >= 0) {
          ct = t;
          break;
        }
      }
      // same number of digits with a narrower digit: fewer buckets, and the top digit keeps enough bits to spread over
      // many buckets (c = 18 leaves it 2 bits — three buckets then hold a quarter of all entries each; c = 17 leaves 16)
      while (ct > c + 1 && 254 / (ct - 1) + 1 == 254 / ct + 1) ct--;
      // tab > 1: table mode with THIS digit width (a base subset that keeps the geometry of the full set, prover.cpp: sparse B)
      if (tab > 1 && tab <= 20 && tab_low_bits(tab, ib, 254 / tab + 1) >= 0) ct = tab;
    }
    if (ct) c = ct;
    else tab = 0;
    g.IB = ib;
  }
  g.tab = tab ? 1 : 0;
  g.c = c;
  g.W = bits / c + 1; // the top window holds the remaining bits + the carry of the signed recoding
  // … for which it has no room when c − 1 bits remain for it: 2^(c−1) − 1 plus the carry is beyond the largest digit, and a short
  // scalar is never negated out of the way as a full-width one is (recode_fe) — one more window takes the carry
  // (tests/msm_recode_check.cpp: bitsize 64 with c = 5 or 13 lost every scalar whose top bits are all ones)
  if (bits != 254 && g.W > 1 && bits % c == c - 1) g.W++;
  g.NB = 1u << (c - 1);
  g.pf = g.tab ? 1 : pf;
  g.nbms = (g.W + g.pf - 1) / g.pf;
  if (g.tab) {
    g.NBb = g.NB > 32768u ? 32768u : g.NB;
    g.Wb = (int)(g.NB / g.NBb);
  } else {
    g.NBb = g.NB;
    g.Wb = g.nbms;
  }
  g.wide = g.W;
  {
    // Table mode: always (one shared bucket set: nothing is lost).  Classic layout (one bucket set per window): a narrower
    // window leaves half of its buckets empty, so only when the top digit would be 1–3 bits short — then its entries sit in
    // 1/2 … 1/8 of a window's buckets, too few per bucket for the large-bucket path and several times the average
    // (c = 16: a 14-bit top digit); a top digit 4 or more bits short is handled by the large-bucket kernels.
    const int spare = g.W * c - 254; // ≥ 0: bits the W windows cover beyond the 254 of a scalar
    // (only for full-width scalars — the argument rests on the recoded value being ≤ (r − 1)/2 — and equal windows are what
    //  the shift c·nbms of precomputed bases assumes)
    if (bits == 254 && g.pf == 1 && c >= 5 && (g.tab || spare <= 3)) g.wide = g.W - (spare < g.W ? spare : g.W); // (a 3-bit top window would have no room for offset + carry)
  }
  uint32_t H[10] = {0};
  for (int w = 0; w < g.W; w++) {
    const int bit = (w < g.wide ? w * c : g.wide * c + (w - g.wide) * (c - 1)) + (w < g.wide ? c : c - 1) - 1;
    H[bit >> 5] |= 1u << (bit & 31);
  }
  memcpy(g.H, H, sizeof g.H);
  return g;
}

} // namespace isnark
