// pairing29_check.cpp — host-side checked build of the radix-2^29 pairing (csrc/pairing29.h).
// Test infrastructure: compiled with g++ -DF29_CHECK by tests/test_pairing29.py, which compares the results with the host
// pairing / verifier of the library (prover/pairing.cpp) and with a discrete-log model of the verification equation
// (tests/groth16_dlog_model.py) while every bound of ff29.h / ec29.h / pairing29.h is asserted.
// p29_last_failure() names the first violated bound ("" when none fired).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../icicle-snark_amd/csrc/pairing29.h"

using namespace bn254;

extern "C" const char* p29_last_failure() { return f29::g_check_failure ? f29::g_check_failure : ""; }
extern "C" void p29_reset() { f29::g_check_failure = nullptr; }

// out[i] = e(P_i, Q_i): standard-form affine in ((0, 0) = identity ↦ 1), 12 standard-form coefficients out
extern "C" void p29_pairing(const fe* p, const fe2* q, int n, fe* out)
{
  for (int i = 0; i < n; i++) {
    const fe* P = p + 2 * i;
    const fe2* Q = q + 2 * i;
    const bool pz = p29::std_is_zero(P[0]) && p29::std_is_zero(P[1]);
    const bool qz = p29::std_is_zero(Q[0].c0) && p29::std_is_zero(Q[0].c1) && p29::std_is_zero(Q[1].c0) && p29::std_is_zero(Q[1].c1);
    const p29::F12 e = (pz || qz) ? p29::f12_one()
                                  : p29::pairing(f29::from_std(P[0]), f29::from_std(P[1]), Fq2_29::load_std(Q[0]), Fq2_29::load_std(Q[1]));
    p29::f12_store_std(e, out + 12 * i);
  }
}

// IC points (standard form, (0, 0) = identity) → the lazy affine form and identity flags that public_input takes
static void load_ic(const fe* ic, int n_pub, std::vector<G1L::A>& icl, std::vector<uint8_t>& icz)
{
  icl.resize(n_pub + 1);
  icz.resize(n_pub + 1);
  for (int j = 0; j <= n_pub; j++) {
    icz[j] = p29::std_is_zero(ic[2 * j]) && p29::std_is_zero(ic[2 * j + 1]);
    icl[j] = {f29::from_std(ic[2 * j]), f29::from_std(ic[2 * j + 1])};
  }
}

// m proofs of one key through verify_proof, with the key's lines precomputed once (make_verify_key) and the signals laid out as
// verify_batch_kernel reads them: signal j of proof k at pub[j·m + k].  vk = α (2 fe), β, γ, δ (2 fe2 each); ic = n_pub + 1
// affine points (standard form); a, b, c the proofs' points (m each).  verdicts[k] = 1 / 0 / −2.
extern "C" void p29_verify_batch(const fe* alpha, const fe2* beta, const fe2* gamma, const fe2* delta, const fe* ic, int n_pub, int m,
                                 const fe* pub, const fe* a, const fe2* b, const fe* c, int* verdicts)
{
  static p29::VerifyKey29 vk; // large: not on the stack
  p29::make_verify_key(alpha, beta, gamma, delta, n_pub, &vk);
  std::vector<G1L::A> icl;
  std::vector<uint8_t> icz;
  load_ic(ic, n_pub, icl, icz);
  for (int k = 0; k < m; k++)
    verdicts[k] = p29::verify_proof(vk, icl.data(), icz.data(), a + 2 * k, b + 2 * k, c + 2 * k, pub + k, (size_t)m);
}

// cpub_k = IC₀ + Σ_j pub[j·m + k]·IC_{j+1} through public_input, for k < m: found[k] = 0 for cpub = O, else 1 and xy[2k], xy[2k + 1]
// the affine point (standard form, canonical)
extern "C" void p29_public_input(const fe* ic, int n_pub, int m, const fe* pub, int* found, fe* xy)
{
  std::vector<G1L::A> icl;
  std::vector<uint8_t> icz;
  load_ic(ic, n_pub, icl, icz);
  for (int k = 0; k < m; k++) {
    fe9 x, y;
    found[k] = p29::public_input(icl.data(), icz.data(), n_pub, pub + k, (size_t)m, x, y);
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
