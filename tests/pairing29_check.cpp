// pairing29_check.cpp — host-side checked build of the radix-2^29 pairing (csrc/pairing29.h).
// Test infrastructure: compiled with g++ -DF29_CHECK by tests/test_pairing29.py, which compares the results with the host
// pairing / verifier of the library (prover/pairing.cpp) and with a discrete-log model of the verification equation
// (tests/groth16_dlog_model.py) while every bound of ff29.h / ec29.h / pairing29.h is asserted.
// The per-key preparation is the product's own (prover/verify_host.h: PreparedKey), so its bounds are asserted here too.
// p29_last_failure() names the first violated bound ("" when none fired).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../icicle-snark_amd/csrc/prover/verify_host.h"

using namespace bn254;

extern "C" const char* p29_last_failure() { return f29::g_check_failure ? f29::g_check_failure : ""; }
extern "C" void p29_reset() { f29::g_check_failure = nullptr; }

// out[i] = e(P_i, Q_i): standard-form affine in ((0, 0) = identity ↦ 1), 12 standard-form coefficients out
extern "C" void p29_pairing(const fe* p, const fe2* q, int n, fe* out)
{
  for (int i = 0; i < n; i++) {
    const fe* P = p + 2 * i;
    const fe2* Q = q + 2 * i;
    const p29::F12 e = (p29::g1_std_is_zero(P) || p29::g2_std_is_zero(Q))
                         ? p29::f12_one()
                         : p29::pairing(f29::from_std(P[0]), f29::from_std(P[1]), Fq2_29::load_std(Q[0]), Fq2_29::load_std(Q[1]));
    p29::f12_store_std(e, out + 12 * i);
  }
}

// the arguments as the parser would leave them; a null point stands for the identity (no lines are made for it)
static isnark::vb::VbKey make_key(const fe* alpha, const fe2* beta, const fe2* gamma, const fe2* delta, const fe* ic, int n_pub)
{
  isnark::vb::VbKey key{};
  if (alpha) memcpy(key.alpha, alpha, sizeof key.alpha);
  if (beta) memcpy(key.beta, beta, sizeof key.beta);
  if (gamma) memcpy(key.gamma, gamma, sizeof key.gamma);
  if (delta) memcpy(key.delta, delta, sizeof key.delta);
  key.ic.assign(ic, ic + 2 * (n_pub + 1));
  key.n_public = (size_t)n_pub;
  return key;
}

// m proofs of one key through verify_proof, with the key prepared once (PreparedKey, target included) and the signals laid out as
// verify_batch_kernel reads them: signal j of proof k at pub[j·m + k].  vk = α (2 fe), β, γ, δ (2 fe2 each); ic = n_pub + 1
// affine points (standard form); a, b, c the proofs' points (m each).  verdicts[k] = 1 / 0 / −2.
extern "C" void p29_verify_batch(const fe* alpha, const fe2* beta, const fe2* gamma, const fe2* delta, const fe* ic, int n_pub, int m,
                                 const fe* pub, const fe* a, const fe2* b, const fe* c, int* verdicts)
{
  const isnark::vb::VbKey key = make_key(alpha, beta, gamma, delta, ic, n_pub);
  isnark::vb::PreparedKey pk;
  pk.prepare(key);
  pk.need_target();
  for (int k = 0; k < m; k++)
    verdicts[k] = p29::verify_proof(pk.vk[0], pk.ic(), pk.ic_zero(), a + 2 * k, b + 2 * k, c + 2 * k, pub + k, (size_t)m);
}

// cpub_k = IC₀ + Σ_j pub[j·m + k]·IC_{j+1} through public_input, for k < m: found[k] = 0 for cpub = O, else 1 and xy[2k], xy[2k + 1]
// the affine point (standard form, canonical)
extern "C" void p29_public_input(const fe* ic, int n_pub, int m, const fe* pub, int* found, fe* xy)
{
  const isnark::vb::VbKey key = make_key(nullptr, nullptr, nullptr, nullptr, ic, n_pub);
  isnark::vb::PreparedKey pk;
  pk.prepare(key);
  for (int k = 0; k < m; k++) {
    fe9 x, y;
    found[k] = p29::public_input(pk.ic(), pk.ic_zero(), n_pub, pub + k, (size_t)m, x, y);
    if (found[k]) {
      xy[2 * k] = f29::pack(f29::canon(f29::mul(x, f29::one_std())));
      xy[2 * k + 1] = f29::pack(f29::canon(f29::mul(y, f29::one_std())));
    }
  }
}

// one proof (stride 1): pub = n_pub scalars.  Returns 1 / 0 / −2.
extern "C" int p29_verify(const fe* alpha, const fe2* beta, const fe2* gamma, const fe2* delta, const fe* ic, int n_pub, const fe* pub,
                          const fe* a, const fe2* b, const fe* c)
{
  int v = 0;
  p29_verify_batch(alpha, beta, gamma, delta, ic, n_pub, 1, pub, a, b, c, &v);
  return v;
}

// [r]·Q = O on the twist (Q standard form, on the twist, not the identity)
extern "C" int p29_g2_in_subgroup(const fe2* q) { return p29::g2_in_subgroup(Fq2_29::load_std(q[0]), Fq2_29::load_std(q[1])); }
