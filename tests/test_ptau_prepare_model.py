"""tests/ptau_prepare_model.py against the synthesiser and against the algebra it restates.  No GPU: the model is what the GPU
tests take their expected bytes from, so it is tested on its own first."""
import struct

import pytest

import ptau_prepare_model as PM

R = PM.R
POWERS = [0, 1, 2, 3, 5]


@pytest.fixture(scope="module")
def fbm(O):
    gen = {g: O.ec_to_affine(g, O.ec_generator(g)) for g in ("g1", "g2")}
    return lambda g, sc: O.fixed_base_mul(g, gen[g], sc)


def test_omega_is_the_synthesisers(S):
    assert all(PM.omega(k) == S.omega(k) for k in range(0, 29, 3)) and (PM.R, PM.Q) == (S.R_MOD, S.Q_MOD)


@pytest.mark.parametrize("power", POWERS)
def test_blocks_are_the_lagrange_values(S, power):
    """generic τ: block p ≤ power of every section is k·L_j(τ) of the size-2^p domain, as synth.write_ptau has it"""
    tau, alpha, beta = S.toxic_waste()[:3]
    got = PM.prepared_scalars(power, tau, alpha, beta)
    lag = []
    for p in range(power + 1):
        lag += S.lagrange_at(1 << p, p, tau) if p else [1]
    N = 1 << power
    assert got[12][:2 * N - 1] == lag and got[13] == lag
    assert got[14] == [alpha * x % R for x in lag] and got[15] == [beta * x % R for x in lag]
    assert len(got[12]) == 4 * N - 1


@pytest.mark.parametrize("power", POWERS)
def test_the_last_block_is_the_truncated_basis(S, power):
    """block power + 1 of section 12 is L'_j(τ) − τ^(2N−1)·ω'^(−j(2N−1))/(2N): the transform of the vector without τ^(2N−1)"""
    tau = S.toxic_waste()[0]
    N = 1 << power
    got = PM.prepared_scalars(power, tau, 1, 1)[12][2 * N - 1:]
    full = S.lagrange_at(2 * N, power + 1, tau)
    wi = pow(PM.omega(power + 1), -1, R)
    top, inv2n = pow(tau, 2 * N - 1, R), pow(2 * N, -1, R)
    assert got == [(full[j] - top * pow(wi, j * (2 * N - 1), R) * inv2n) % R for j in range(2 * N)]
    assert got != full
    # Σ_j p(ω'^j)·Ltrunc_j = p(τ) for every polynomial of degree ≤ 2N − 2: what makes a key over this block valid
    w = PM.omega(power + 1)
    pr = S._Prng(7 + power)
    for deg in sorted({0, N - 1, 2 * N - 2} - {-1}):
        coef = [pr.fr() for _ in range(deg + 1)]
        ev = lambda x: sum(c * pow(x, i, R) for i, c in enumerate(coef)) % R
        assert sum(ev(pow(w, j, R)) * got[j] for j in range(2 * N)) % R == ev(tau)
    # and one degree higher it does not hold
    coef = [0] * (2 * N - 1) + [1]
    ev = lambda x: pow(x, 2 * N - 1, R)
    assert sum(ev(pow(w, j, R)) * got[j] for j in range(2 * N)) % R != ev(tau)


def test_tau_inside_a_domain():
    """where synth.lagrange_at divides by zero: τ = ω₃ makes block 3 the unit vector e₁, τ = 1 makes every block e₀"""
    w3 = PM.omega(3)
    sc = PM.prepared_scalars(3, w3, 5, 7)
    assert sc[12][7:15] == [0, 1, 0, 0, 0, 0, 0, 0] and sc[14][7:15] == [0, 5, 0, 0, 0, 0, 0, 0]
    one = PM.prepared_scalars(3, 1, 5, 7)
    for p in range(4):
        assert one[13][(1 << p) - 1:(2 << p) - 1] == [1] + [0] * ((1 << p) - 1)
    # block power + 1 with its last input missing: every output is non-zero (1 − ω'^j/16 ≠ 0 … the sum of 15 of 16 roots' powers)
    assert all(one[12][15:])


@pytest.mark.parametrize("power", [0, 2, 3])
def test_the_unprepared_writer_is_the_synthesisers(S, O, fbm, power):
    to_mont = lambda a: O.fq_convert_montgomery(a, True)
    tau, alpha, beta = S.toxic_waste()[:3]
    full = S.write_ptau(power, fbm, points_to_mont=to_mont)
    mine = PM.write_unprepared(power, tau, alpha, beta, fbm, to_mont)
    assert mine == PM.without(full, {12, 13, 14, 15}) and struct.unpack_from("<I", mine, 8)[0] == 7
    want = PM.expected_prepared(mine, power, tau, alpha, beta, fbm, to_mont)
    assert len(want) == PM.prepared_size(power, len(mine)) == len(full)
    N = 1 << power
    cut = PM.sections(full)[0][12][0] + (2 * N - 1) * 64                   # section 12's last block
    assert want[:cut] == full[:cut] and want[cut + 2 * N * 64:] == full[cut + 2 * N * 64:]
    assert want[cut:cut + 2 * N * 64] != full[cut:cut + 2 * N * 64]
