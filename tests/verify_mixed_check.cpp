// verify_mixed_check.cpp — the mixed-key verifier's equation evaluated on the host, under F29_CHECK.
// Test infrastructure: a stand-alone program that tests/test_verify_mixed_host.py compiles with g++ -DF29_CHECK (every bound of
// ff29.h / ec29.h / pairing29.h asserted) and once more with -fsanitize=address,undefined.  The grouping, the per-key sums and the
// layout of the segmented sum are the product's own (prover/verify_host.h: group_by_key, MixedSums, mixed_segments); the lanes, the
// Miller loops and the final exponentiation are pairing29.h's; the segment sums are plain double-and-add over the layout's arrays.
//
//   verify_mixed_check <input file>
// input (little endian):  u32 K, u32 m, seed[32];  per key: u32 n_pub, α₁ (64 B), β₂, γ₂, δ₂ (128 B each), IC ((n_pub + 1)·64 B);
//                         per item: i32 key, u64 index, A (64 B), B (128 B), C (64 B), n_pub signals of its key (32 B each)
// output:                 "global g" and one "key k v" per key — 1 the equation holds and every pi_b is in G2, 0 otherwise, for the
//                         whole batch and for each key's own equation — then "bounds ok" or the first violated bound.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../icicle-snark_amd/csrc/prover/verify_host.h"

using namespace bn254;
using namespace isnark::vb;

static fe to_std(const fe9& x) { return f29::pack(f29::canon(f29::mul(x, f29::one_std()))); }

struct Reader {
  std::vector<uint8_t> buf;
  size_t at = 0;
  bool ok = true;
  void take(void* out, size_t n)
  {
    if (at + n > buf.size()) {
      ok = false;
      memset(out, 0, n);
      return;
    }
    memcpy(out, buf.data() + at, n);
    at += n;
  }
  template <class T>
  T get()
  {
    T v;
    take(&v, sizeof v);
    return v;
  }
};

// Σ scalars[k]·points[k] over [lo, hi), the low `bits` bits of every scalar, (0, 0) points skipped: standard-form affine, (0, 0) = O
static void segment_sum(const std::vector<fe>& points, const std::vector<fe>& scalars, uint64_t lo, uint64_t hi, int bits, fe out[2])
{
  G1L::X acc = G1L::x_zero();
  for (uint64_t k = lo; k < hi; k++) {
    if (p29::g1_std_is_zero(&points[2 * k])) continue;
    acc = G1L::x_add(acc, p29::g1_mul_bits({f29::from_std(points[2 * k]), f29::from_std(points[2 * k + 1])}, scalars[k].l, bits));
  }
  out[0] = out[1] = Fq::zero();
  if (G1L::x_is_zero(acc)) return;
  fe9 x, y;
  p29::g1_to_affine(acc, x, y);
  out[0] = to_std(x);
  out[1] = to_std(y);
}

int main(int argc, char** argv)
{
  if (argc != 2) return 2;
  Reader in;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint8_t chunk[65536];
  for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) in.buf.insert(in.buf.end(), chunk, chunk + n);
  fclose(f);

  const uint32_t K = in.get<uint32_t>(), m = in.get<uint32_t>();
  uint8_t seed[32];
  in.take(seed, 32);
  std::vector<VbKey> keys(K);
  std::vector<size_t> n_public(K);
  for (uint32_t k = 0; k < K && in.ok; k++) {
    VbKey& key = keys[k];
    key.n_public = n_public[k] = in.get<uint32_t>();
    in.take(key.alpha, sizeof key.alpha);
    in.take(key.beta, sizeof key.beta);
    in.take(key.gamma, sizeof key.gamma);
    in.take(key.delta, sizeof key.delta);
    key.ic.resize(2 * (key.n_public + 1));
    in.take(key.ic.data(), key.ic.size() * sizeof(fe));
  }
  std::vector<int32_t> key_of(m);
  std::vector<uint64_t> index(m);
  std::vector<VbItem> items(m);
  std::vector<std::vector<fe>> signals(m);
  std::vector<int> live;
  for (uint32_t i = 0; i < m && in.ok; i++) {
    key_of[i] = in.get<int32_t>();
    index[i] = in.get<uint64_t>();
    if (key_of[i] < 0 || (uint32_t)key_of[i] >= K) return 2;
    in.take(&items[i], sizeof(VbItem));
    signals[i].resize(n_public[key_of[i]] + 1);
    in.take(signals[i].data(), n_public[key_of[i]] * sizeof(fe));
    live.push_back((int)i);
  }
  if (!in.ok || in.at != in.buf.size()) return 2;

  // the product's host part: grouping, per-key sums (two partial sets added, as the pool's ranges are), the layout
  const KeyGroups groups = group_by_key(key_of.data(), live, K);
  const MixedSegments seg = mixed_segments(groups, n_public);
  MixedSums sums(n_public), second(n_public);
  std::vector<uint32_t> z(4 * (size_t)m + 4);
  for (uint32_t i = 0; i < m; i++) (i < m / 2 ? sums : second).add_item((size_t)key_of[i], seed, index[i], signals[i].data(), &z[4 * (size_t)i]);
  sums.add(second);

  // the lanes
  std::vector<p29::F12> lane(m);
  std::vector<uint8_t> ok(m);
  for (uint32_t i = 0; i < m; i++) ok[i] = p29::combined_lane(items[i].a, items[i].b, &z[4 * (size_t)i], lane[i]) ? 1 : 0;

  // the segmented sum's operands as the layout places them, and its 3K results
  std::vector<fe> points(2 * seg.total + 2, Fq::zero()), scalars(seg.total + 1, Fr::zero());
  for (size_t q = 0; q < groups.pos.size(); q++) {
    const uint32_t p = groups.pos[q];
    points[2 * q] = items[p].c[0];
    points[2 * q + 1] = items[p].c[1];
    for (int w = 0; w < 4; w++) scalars[q].l[w] = z[4 * (size_t)p + w];
  }
  for (uint32_t k = 0; k < K; k++) {
    const uint64_t at = seg.offsets[K + k];
    for (size_t j = 0; j <= n_public[k]; j++) {
      points[2 * (at + j)] = keys[k].ic[2 * j];
      points[2 * (at + j) + 1] = keys[k].ic[2 * j + 1];
      scalars[at + j] = sums.per_key[k].u[j];
    }
    points[2 * (seg.alpha_base + k)] = keys[k].alpha[0];
    points[2 * (seg.alpha_base + k) + 1] = keys[k].alpha[1];
    scalars[seg.alpha_base + k] = sums.per_key[k].u[0];
  }
  if (seg.offsets.size() != 3 * (size_t)K + 1 || seg.offsets[3 * K] != seg.total) return 3;

  // per key: its lanes' values and its three pairs (S_C, δ₂), (S_pub, γ₂), (u₀·α₁, β₂); the whole batch: all of them
  p29::F12 all = p29::f12_one();
  bool all_ok = true;
  std::vector<int> verdict(K);
  for (uint32_t k = 0; k < K; k++) {
    p29::F12 v = p29::f12_one();
    bool flags = true;
    for (uint32_t q = groups.off[k]; q < groups.off[k + 1]; q++) {
      if (key_of[live[groups.pos[q]]] != (int32_t)k) return 3;
      v = p29::f12_mul(v, lane[groups.pos[q]]);
      flags = flags && ok[groups.pos[q]];
    }
    const fe2* g2[3] = {keys[k].delta, keys[k].gamma, keys[k].beta};
    for (int part = 0; part < 3; part++) {
      const size_t s = (size_t)part * K + k;
      if (seg.bits[s] != (part == 0 ? 128 : 254)) return 3;
      fe sum[2];
      segment_sum(points, scalars, seg.offsets[s], seg.offsets[s + 1], seg.bits[s], sum);
      if (p29::g1_std_is_zero(sum) || p29::g2_std_is_zero(g2[part])) continue;
      v = p29::f12_mul(v, p29::miller_single(f29::from_std(sum[0]), f29::from_std(sum[1]), Fq2_29::load_std(g2[part][0]), Fq2_29::load_std(g2[part][1])));
    }
    verdict[k] = flags && p29::combined_finish(v, p29::f12_one()) ? 1 : 0;
    all = p29::f12_mul(all, v);
    all_ok = all_ok && flags;
  }
  printf("global %d\n", all_ok && p29::combined_finish(all, p29::f12_one()) ? 1 : 0);
  for (uint32_t k = 0; k < K; k++) printf("key %u %d\n", k, verdict[k]);
  if (f29::g_check_failure) {
    printf("bound: %s\n", f29::g_check_failure);
    return 4;
  }
  printf("bounds ok\n");
  return 0;
}
