"""groth16_setup_toxic_check, the host half of groth16_setup: which toxic waste (τ, α, β, γ, δ) the setup refuses before any device
work.  Every case is CONSTRUCTED; the synthesiser says why the domain cases must be refused (it divides by zero there).  No GPU."""
import pytest

P = 9                      # the domain of the largest test circuit: n = 512
N = 1 << P


def test_the_synthesisers_toxic_waste_passes(K, S):
    T = S.toxic_waste()
    assert all(0 < x < S.R_MOD for x in T) and pow(T[0], 2 * N, S.R_MOD) != 1
    for p in (0, 1, 3, P, 20, 27):
        assert K.setup_toxic_check(T, p) == 0
    assert K.setup_toxic_check(T[:3] + (1, 1), P) == 0               # γ = δ = 1: zkey-new's key


@pytest.mark.parametrize("which", range(5))
def test_a_zero_scalar(K, S, which):
    T = list(S.toxic_waste())
    T[which] = 0
    assert K.setup_toxic_check(T, P) == K.TOXIC_ZERO == 2


@pytest.mark.parametrize("which", range(5))
def test_a_scalar_that_is_r(K, S, which):
    T = list(S.toxic_waste())
    T[which] = S.R_MOD
    assert K.setup_toxic_check(T, P) == K.TOXIC_RANGE == 1
    T[which] = (1 << 256) - 1
    assert K.setup_toxic_check(T, P) == K.TOXIC_RANGE
    T[which] = S.R_MOD - 1                                            # the largest scalar there is (τ = −1 is in every domain ≥ 2)
    assert K.setup_toxic_check(T, P) == (K.TOXIC_DOMAIN if which == 0 else 0)


def test_the_first_fault_is_reported(K, S):
    T = list(S.toxic_waste())
    T[1], T[3] = 0, S.R_MOD                                           # α = 0 comes before γ = r
    assert K.setup_toxic_check(T, P) == K.TOXIC_ZERO
    T[1], T[3] = S.R_MOD, 0
    assert K.setup_toxic_check(T, P) == K.TOXIC_RANGE
    T = list(S.toxic_waste())
    T[0], T[4] = 1, 0                                                 # a range or zero fault comes before the domain's
    assert K.setup_toxic_check(T, P) == K.TOXIC_ZERO


def test_tau_in_the_domain_or_its_coset(K, S):
    w, g = S.omega(P), S.omega(P + 1)
    base = S.toxic_waste()
    in_domain, in_coset = pow(w, 3, S.R_MOD), g * pow(w, 3, S.R_MOD) % S.R_MOD
    # the synthesiser divides by zero exactly there: L_j(τ) has the denominator τ − ω^j, section 9's row τ/g − ω^j
    with pytest.raises((ZeroDivisionError, ValueError)):
        S.lagrange_at(N, P, in_domain)
    with pytest.raises((ZeroDivisionError, ValueError)):
        S.lagrange_at(N, P, in_coset * pow(g, -1, S.R_MOD) % S.R_MOD)
    S.lagrange_at(N, P, in_coset)                                     # (the coset is harmless to row 0 alone)
    for tau in (in_domain, in_coset, 1, S.R_MOD - 1, g):
        assert K.setup_toxic_check((tau,) + base[1:], P) == K.TOXIC_DOMAIN == 3, hex(tau)
    # the same τ is no fault for a domain it is not in: ω_512³ has order 512, outside the domain of 128 and its coset
    assert pow(in_domain, 2 * 128, S.R_MOD) != 1
    assert K.setup_toxic_check((in_domain,) + base[1:], 7) == 0
    assert K.setup_toxic_check((in_domain,) + base[1:], 8) == K.TOXIC_DOMAIN      # 2n = 512
    # a root of a larger domain is fine here
    assert K.setup_toxic_check((S.omega(P + 2),) + base[1:], P) == 0


def test_arguments(K, S):
    with pytest.raises(K.ProverError, match=r"\(-3\)"):
        K.setup_toxic_check(S.toxic_waste(), 28)
    assert K.lib().groth16_setup_toxic_check(None, 3) == -3
