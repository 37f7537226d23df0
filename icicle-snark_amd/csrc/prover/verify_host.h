// verify_host.h — the host-only pieces of the Groth16 verifiers: what the parser leaves (VbKey, VbItem), the per-key
// preparation every device stage and the combined tail read (PreparedKey), the combined verifier's host sums (CombinedSums), the
// mixed-key verifier's grouping, per-key sums and segment layout (KeyGroups, MixedSums, MixedSegments), and the host point helpers
// of the key tools (identity-aware affine forms, the generators, one pairing equation).
// No HIP types: the product's .hip files and the F29_CHECK host builds (tests/pairing29_check.cpp,
// tests/pairing29_combined_check.cpp, tests/verify_mixed_check.cpp) compile the same code, so a bound broken here fires in the
// checked build.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../../include/icicle_snark_hip.h"
#include "../pairing29.h"
#include "sha256.h"

namespace isnark {
namespace vb {

struct VbKey {                   // standard form, canonical; (0, 0) = identity
  bn254::fe alpha[2];
  bn254::fe2 beta[2], gamma[2], delta[2];
  std::vector<bn254::fe> ic;     // (n_public + 1) affine points, x then y
  size_t n_public = 0;
};
struct VbItem {                  // one proof's points, standard form, canonical, on their curves
  bn254::fe a[2];
  bn254::fe2 b[2];
  bn254::fe c[2];
};

// The input checks of all three verifier entry points (pairing.cpp).  0, or the code for the text (−2 format, −3 null) with the
// message in groth16_verify_last_error() of the calling thread.  parse_item runs the order-r test of pi_b only when
// `host_subgroup_test` is set: the batch stages leave it to their kernels.
int parse_vk(const char* vk_json, VbKey* out);
int parse_item(const char* proof_json, const char* public_json, size_t n_public, VbItem* item, bn254::fe* pub, bool host_subgroup_test);
int fail(int code, const char* msg);

// What one verification key contributes to every proof, made once per call.
//   vk      as verify_batch_kernel reads it: γ₂ / δ₂'s lines (use_gamma / use_delta = 0 for an identity point, whose pairings are 1)
//           and the target conj(e(α₁, β₂)).  The target costs a pairing and only the per-item stage compares with it, so it is
//           left out until need_target().
//   ic1     the IC points in lazy form behind one identity slot, ic1_zero their identity flags: the combined tail's Straus sum
//           Σⱼ uⱼ·ICⱼ reads n_public + 2 entries from slot 0 (p29::combined_tail_miller), the per-item stage n_public + 1 from slot 1.
struct PreparedKey {
  std::vector<bn254::p29::VerifyKey29> vk; // one entry (≈ 40 KB: not on the stack)
  std::vector<bn254::G1L::A> ic1;
  std::vector<uint8_t> ic1_zero;
  const VbKey* key = nullptr;
  bool have_target = false;

  void prepare(const VbKey& k)
  {
    using namespace bn254;
    key = &k;
    have_target = false;
    vk.resize(1);
    p29::make_verify_lines(k.gamma, k.delta, (int)k.n_public, &vk[0]);
    ic1.resize(k.n_public + 2);
    ic1_zero.resize(k.n_public + 2);
    ic1[0] = {f29::one_m(), f29::one_m()};
    ic1_zero[0] = 1;
    for (size_t j = 0; j <= k.n_public; j++) {
      ic1_zero[j + 1] = p29::g1_std_is_zero(&k.ic[2 * j]);
      ic1[j + 1] = {f29::from_std(k.ic[2 * j]), f29::from_std(k.ic[2 * j + 1])};
    }
  }
  void need_target()
  {
    using namespace bn254;
    if (have_target) return;
    p29::make_verify_target(key->alpha, key->beta, &vk[0]);
    have_target = true;
  }
  const bn254::p29::Line* gamma_lines() const { return vk[0].use_gamma ? vk[0].gamma : nullptr; }
  const bn254::p29::Line* delta_lines() const { return vk[0].use_delta ? vk[0].delta : nullptr; }
  const bn254::G1L::A* ic() const { return ic1.data() + 1; } // n_public + 1 entries, as p29::verify_proof / public_input take them
  const uint8_t* ic_zero() const { return ic1_zero.data() + 1; }
};

// The combined verifier's host arithmetic over a set of items: u₀ = Σ z, u_{j+1} = Σ z·sⱼ mod r (standard form)
struct CombinedSums {
  std::vector<bn254::fe> u;
  explicit CombinedSums(size_t n_public) : u(n_public + 1, bn254::Fr::zero()) {}
  // the item at `index` of the caller's arrays, signals s[0 … n_public) in standard form: its coefficient z (sha256.h's rule) goes
  // to z4 as four 32-bit words, little endian, and into the sums
  void add_item(const uint8_t seed[32], uint64_t index, const bn254::fe* s, uint32_t z4[4])
  {
    using namespace bn254;
    uint8_t c[16];
    combined_coefficient(seed, index, c);
    fe zf = Fr::zero();
    for (int w = 0; w < 4; w++) zf.l[w] = z4[w] = (uint32_t)c[4 * w] | (uint32_t)c[4 * w + 1] << 8 | (uint32_t)c[4 * w + 2] << 16 | (uint32_t)c[4 * w + 3] << 24;
    u[0] = Fr::add(u[0], zf);
    const fe zm = Fr::to_mont(zf); // (z·R)·s·R⁻¹ = z·s
    for (size_t j = 0; j + 1 < u.size(); j++) u[j + 1] = Fr::add(u[j + 1], Fr::mul(zm, s[j]));
  }
  void add(const CombinedSums& o)
  {
    for (size_t j = 0; j < u.size(); j++) u[j] = bn254::Fr::add(u[j], o.u[j]);
  }
};

// ---- the mixed-key verifier's host part (verify_mixed.hip): live items grouped by key, one CombinedSums per key, and the layout of
// the one segmented sum over 3·K segments.
// pos[off[k] … off[k+1]) = the positions in `live` of key k's items, ascending; key_of[live[·]] is in range (the parse refused the rest)
struct KeyGroups {
  std::vector<uint32_t> off, pos;
  size_t n_keys() const { return off.size() - 1; }
  size_t count(size_t k) const { return off[k + 1] - off[k]; }
};
inline KeyGroups group_by_key(const int32_t* key_of, const std::vector<int>& live, size_t n_keys)
{
  KeyGroups g;
  g.off.assign(n_keys + 1, 0);
  g.pos.resize(live.size());
  for (int i : live) g.off[(size_t)key_of[i] + 1]++;
  for (size_t k = 0; k < n_keys; k++) g.off[k + 1] += g.off[k];
  std::vector<uint32_t> cursor(g.off.begin(), g.off.end() - 1);
  for (size_t p = 0; p < live.size(); p++) g.pos[cursor[(size_t)key_of[live[p]]]++] = (uint32_t)p;
  return g;
}
// u₀,k = Σ_{i∈k} zᵢ, u_{j+1,k} = Σ_{i∈k} zᵢ·sᵢⱼ: the one-key sums, once per key
struct MixedSums {
  std::vector<CombinedSums> per_key;
  explicit MixedSums(const std::vector<size_t>& n_public)
  {
    per_key.reserve(n_public.size());
    for (size_t np : n_public) per_key.emplace_back(np);
  }
  void add_item(size_t key, const uint8_t seed[32], uint64_t index, const bn254::fe* s, uint32_t z4[4]) { per_key[key].add_item(seed, index, s, z4); }
  void add(const MixedSums& o)
  {
    for (size_t k = 0; k < per_key.size(); k++) per_key[k].add(o.per_key[k]);
  }
};
// The segmented sum's operands, region by region: [the live items' C, key-major as KeyGroups orders them | every key's IC | every
// key's α₁], with the scalars [zᵢ | u₀,k … u_{np,k} | u₀,k] beside them.  Segment k < K is S_C,k (128 bits), K + k is S_pub,k and
// 2K + k is u₀,k·α₁,k (254 bits): the pair partners are δ₂,k, γ₂,k and β₂,k in that order.
struct MixedSegments {
  std::vector<uint64_t> offsets; // 3K + 1
  std::vector<uint8_t> bits;     // 3K
  uint64_t ic_base = 0, alpha_base = 0, total = 0;
};
inline MixedSegments mixed_segments(const KeyGroups& g, const std::vector<size_t>& n_public)
{
  const size_t K = g.n_keys();
  MixedSegments m;
  m.offsets.resize(3 * K + 1);
  m.bits.resize(3 * K);
  uint64_t at = 0;
  size_t s = 0;
  const auto segment = [&](uint64_t len, uint8_t b) {
    m.offsets[s] = at;
    m.bits[s++] = b;
    at += len;
  };
  for (size_t k = 0; k < K; k++) segment(g.count(k), 128);
  m.ic_base = at;
  for (size_t k = 0; k < K; k++) segment(n_public[k] + 1, 254);
  m.alpha_base = at;
  for (size_t k = 0; k < K; k++) segment(1, 254);
  m.offsets[s] = m.total = at;
  return m;
}

// ---- host point helpers: the C ABI's standard-form points, an affine (0, 0) or a projective z = 0 the identity
inline bool words_zero(const void* p, size_t bytes)
{
  const uint8_t* b = (const uint8_t*)p;
  for (size_t i = 0; i < bytes; i++)
    if (b[i]) return false;
  return true;
}
inline bn254_affine_t affine_or_zero(const bn254_projective_t& p)
{
  bn254_affine_t a;
  memset(&a, 0, sizeof a);
  if (!words_zero(&p.z, sizeof p.z)) bn254_to_affine(&p, &a);
  return a;
}
inline bn254_g2_affine_t affine_or_zero(const bn254_g2_projective_t& p)
{
  bn254_g2_affine_t a;
  memset(&a, 0, sizeof a);
  if (!words_zero(&p.z, sizeof p.z)) bn254_g2_to_affine(&p, &a);
  return a;
}
template <class P>
bool same_point(const P& l, const P& r)
{
  const auto a = affine_or_zero(l), b = affine_or_zero(r);
  return memcmp(&a, &b, sizeof a) == 0;
}
inline bn254_affine_t g1_generator_affine()
{
  bn254_projective_t p;
  bn254_affine_t a;
  bn254_generator(&p);
  bn254_to_affine(&p, &a);
  return a;
}
inline bn254_g2_affine_t g2_generator_affine()
{
  bn254_g2_projective_t p;
  bn254_g2_affine_t a;
  bn254_g2_generator(&p);
  bn254_g2_to_affine(&p, &a);
  return a;
}
// the same two in Montgomery form, as a zkey stores its points
inline bn254::G1::A g1_generator_mont()
{
  const bn254_affine_t s = g1_generator_affine();
  bn254::G1::A g;
  memcpy(&g, &s, sizeof g);
  return bn254::G1::aff_to_mont(g);
}
inline bn254::G2::A g2_generator_mont()
{
  const bn254_g2_affine_t s = g2_generator_affine();
  bn254::G2::A g;
  memcpy(&g, &s, sizeof g);
  return bn254::G2::aff_to_mont(g);
}
// e(a1, a2) = e(b1, b2) by the host pairing.  A side with an identity operand is 1, and when either side is 1 the equation holds
// exactly when both are.
inline bool pairing_eq(const bn254_affine_t& a1, const bn254_g2_affine_t& a2, const bn254_affine_t& b1, const bn254_g2_affine_t& b2)
{
  const bool one_a = words_zero(&a1, sizeof a1) || words_zero(&a2, sizeof a2), one_b = words_zero(&b1, sizeof b1) || words_zero(&b2, sizeof b2);
  if (one_a || one_b) return one_a && one_b;
  alignas(16) bn254_fq12_t l, r; // (bn254_pairing stores 16-byte-aligned field elements; the C type alone asks for 4)
  (void)bn254_pairing(&a1, &a2, &l);
  (void)bn254_pairing(&b1, &b2, &r);
  return memcmp(&l, &r, sizeof l) == 0;
}

} // namespace vb
} // namespace isnark
