// pairing29_combined_check.cpp — host-side checked build of what the combined batch verifier adds to csrc/pairing29.h.
// Test infrastructure: compiled with g++ -DF29_CHECK by tests/test_pairing29_combined.py while every bound of ff29.h / ec29.h /
// pairing29.h is asserted.  The key preparation and the sums are the product's own (prover/verify_host.h: PreparedKey, CombinedSums).
// p29c_last_failure() names the first violated bound ("" when none fired).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../icicle-snark_amd/csrc/prover/verify_host.h"

using namespace bn254;

extern "C" const char* p29c_last_failure() { return f29::g_check_failure ? f29::g_check_failure : ""; }
extern "C" void p29c_reset() { f29::g_check_failure = nullptr; }

static fe to_std(const fe9& x) { return f29::pack(f29::canon(f29::mul(x, f29::one_std()))); }

// both subgroup tests of a twist point (standard form, on the twist, not the identity): bit 0 = g2_in_subgroup, bit 1 = the fast one
extern "C" int p29c_g2_subgroup_both(const fe2* q)
{
  const p29::F2 x = Fq2_29::load_std(q[0]), y = Fq2_29::load_std(q[1]);
  return (p29::g2_in_subgroup(x, y) ? 1 : 0) | (p29::g2_in_subgroup_fast(x, y) ? 2 : 0);
}

// [z](−A) as the lane computes it (g1_mul_bits over 128 bits, g1_to_affine): A standard form, not the identity; z four words.
// Returns 0 for the identity, else 1 and the affine point (standard form) in out[0], out[1].
extern "C" int p29c_lane_mul(const fe* a, const uint32_t* z, fe* out)
{
  const G1L::A na = {f29::from_std(a[0]), p29::fq_neg(f29::from_std(a[1]))};
  const G1L::X r = p29::g1_mul_bits(na, z, 128);
  if (G1L::x_is_zero(r)) return 0;
  fe9 x, y;
  p29::g1_to_affine(r, x, y);
  out[0] = to_std(x);
  out[1] = to_std(y);
  return 1;
}

// out = final_exp(Π_i miller(P_i, Q_i)), identity inputs contributing 1 (12 standard-form coefficients)
extern "C" void p29c_pairing_product(const fe* p, const fe2* q, int n, fe* out)
{
  p29::F12 f = p29::f12_one();
  for (int i = 0; i < n; i++) {
    const fe* P = p + 2 * i;
    const fe2* Q = q + 2 * i;
    if (p29::g1_std_is_zero(P) || p29::g2_std_is_zero(Q)) continue;
    f = p29::f12_mul(f, p29::miller_single(f29::from_std(P[0]), f29::from_std(P[1]), Fq2_29::load_std(Q[0]), Fq2_29::load_std(Q[1])));
  }
  p29::f12_store_std(p29::final_exp(f), out);
}

extern "C" void p29c_coefficients(const uint8_t* seed, uint64_t first, uint64_t count, uint8_t* out16)
{
  for (uint64_t k = 0; k < count; k++) isnark::combined_coefficient(seed, first + k, out16 + 16 * k);
}
extern "C" void p29c_coefficient_from_digest(const uint8_t* digest, uint8_t* out16) { isnark::combined_coefficient_from_digest(digest, out16); }
extern "C" void p29c_sha256(const uint8_t* msg, uint64_t len, uint8_t* out) { isnark::sha256(msg, (size_t)len, out); }

// The whole combined decision over m proofs of one key, as groth16_verify_batch_combined takes it, restated on the host:
// lanes (combined_lane), their product, u₀ = Σ z, u_{j+1} = Σ z·s_j mod r, S_C = Σ z·C, combined_accept.  Key and proofs as
// p29_verify_batch of pairing29_check.cpp takes them, but the signals item-major: pub[k·n_pub + j]; index[k] = the item's index
// for its coefficient.  Returns 1 accepted, 0 the equation failed, −1 a pi_b outside the subgroup.
extern "C" int p29c_combined(const fe* alpha, const fe2* beta, const fe2* gamma, const fe2* delta, const fe* ic, int n_pub, int m, const fe* pub,
                             const fe* a, const fe2* b, const fe* c, const uint8_t* seed, const uint64_t* index)
{
  isnark::vb::VbKey key;
  memcpy(key.alpha, alpha, sizeof key.alpha);
  memcpy(key.beta, beta, sizeof key.beta);
  memcpy(key.gamma, gamma, sizeof key.gamma);
  memcpy(key.delta, delta, sizeof key.delta);
  key.ic.assign(ic, ic + 2 * (n_pub + 1));
  key.n_public = (size_t)n_pub;
  isnark::vb::PreparedKey pk;
  pk.prepare(key);
  isnark::vb::CombinedSums sums((size_t)n_pub);
  p29::F12 prod = p29::f12_one();
  G1L::X sc = G1L::x_zero();
  for (int k = 0; k < m; k++) {
    uint32_t z[4];
    sums.add_item(seed, index[k], pub + (size_t)k * n_pub, z);
    p29::F12 f;
    if (!p29::combined_lane(a + 2 * k, b + 2 * k, z, f)) return -1;
    prod = p29::f12_mul(prod, f);
    const fe* C = c + 2 * k;
    if (!p29::g1_std_is_zero(C)) sc = G1L::x_add(sc, p29::g1_mul_bits({f29::from_std(C[0]), f29::from_std(C[1])}, z, 128));
  }
  fe scs[2] = {Fq::zero(), Fq::zero()};
  if (!G1L::x_is_zero(sc)) {
    fe9 x, y;
    p29::g1_to_affine(sc, x, y);
    scs[0] = to_std(x);
    scs[1] = to_std(y);
  }
  return p29::combined_accept(prod, key.alpha, key.beta, pk.gamma_lines(), pk.delta_lines(), pk.ic1.data(), pk.ic1_zero.data(), n_pub, sums.u.data(), scs)
           ? 1
           : 0;
}
