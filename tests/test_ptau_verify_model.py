"""The model of groth16_ptau_verify (tests/ptau_verify_model.py) against itself, in Python integers: the randomised Lagrange equation
Σ λ_e·b_e = Σ d_i·s_i holds for the exact transforms — τ inside a domain and section 12's zero-extended last block included — the
cross-block cancellation that equal multipliers allow and the μ_p stop, and the exact truth names the bits the specification's
table lists.  No library, no GPU."""
import pytest

import ptau_prepare_model as PM
import ptau_verify_model as VM

R = PM.R
SEEDS = [bytes(range(32)), bytes([0xA5]) * 32]
TAUS = {"random": 0x1D0F5A3C9E7B2468ACE013579BDF02468ACE13579BDF02468ACE13579BDF0246 % R, "one": 1, "minus_one": R - 1, "omega3": PM.omega(3)}
ALPHA, BETA = 0x2B7E151628AED2A6ABF7158809CF4F3C % R, 0x3243F6A8885A308D313198A2E0370734 % R


def _mu(seed):
    return lambda p: VM.mu_of(seed, p)


@pytest.mark.parametrize("power", [0, 1, 3])
@pytest.mark.parametrize("name", list(TAUS))
def test_the_equation_holds_for_the_exact_transform(power, name):
    logs = VM.sound_logs(power, TAUS[name], ALPHA, BETA, prepared=True)
    assert len(logs[2]) == (2 << power) - 1 and len(logs[12]) == (4 << power) - 1    # the truncated top block is there
    for seed in SEEDS:
        x, _ = VM.x_of(seed, power)
        assert x and pow(x, 2 << power, R) != 1
        for sid in (12, 13, 14, 15):
            left, right = VM.lagrange_sides(power, sid, logs[PM.SOURCE[sid]], logs[sid], x, _mu(seed))
            assert left == right, (power, name, sid)
    assert VM.truth(power, logs) == (True, 0, 0, None)
    if name != "random" and power == 3:
        assert any(v == 0 for v in logs[13])                                          # τ inside a domain: identities in 12 … 15


def test_the_equation_sees_one_wrong_element():
    power, seed = 3, SEEDS[0]
    logs = VM.sound_logs(power, TAUS["random"], ALPHA, BETA, prepared=True)
    x, _ = VM.x_of(seed, power)
    for sid in (12, 13, 14, 15):
        for e in (0, 1, 2, len(logs[sid]) - 1):
            blk = list(logs[sid])
            blk[e] = (blk[e] + 1) % R
            left, right = VM.lagrange_sides(power, sid, logs[PM.SOURCE[sid]], blk, x, _mu(seed))
            assert left != right
    # the untruncated last block of section 12 (a writer that knows τ) is another file
    full = list(logs[12])
    N2 = 2 << power
    tau = TAUS["random"]
    full[N2 - 1:] = [(pow(tau, N2, R) - 1) * pow(N2 * (tau * pow(pow(PM.omega(power + 1), j, R), -1, R) - 1), -1, R) % R for j in range(N2)]
    assert full[:N2 - 1] == logs[12][:N2 - 1] and all(a != b for a, b in zip(full[N2 - 1:], logs[12][N2 - 1:]))
    left, right = VM.lagrange_sides(power, 12, logs[2], full, x, _mu(seed))
    assert left != right


@pytest.mark.parametrize("sid,p,j", [(13, 1, 1), (12, 2, 3), (14, 0, 0)])
def test_cross_block_cancellation_needs_the_multipliers(sid, p, j):
    """errors in two neighbouring blocks that cancel for EVERY x when all multipliers are equal; the μ_p tell them apart"""
    power = 3
    logs = VM.sound_logs(power, TAUS["random"], ALPHA, BETA, prepared=True)
    blk = list(logs[sid])
    errors = VM.cancelling_errors(p, j, 0x123456789ABCDEF)
    assert len(errors) == 1 + (2 << p) and max(errors) < len(blk)
    assert sum(1 for v in errors.values() if v) == 2 + (1 << p)       # g vanishes at the other n − 1 roots of X^n − 1: the even k but 2j
    for e, err in errors.items():
        blk[e] = (blk[e] + err) % R
    bad = dict(logs)
    bad[sid] = blk
    assert VM.truth(power, bad) == (False, VM.LAGRANGE_12 + sid - 12, VM.bit(VM.LAGRANGE_12 + sid - 12), None)
    for seed in SEEDS:
        x, _ = VM.x_of(seed, power)
        left, right = VM.lagrange_sides(power, sid, logs[PM.SOURCE[sid]], blk, x, lambda p_: 1)
        assert left == right                                                          # μ ≡ 1: accepted, whatever x
        left, right = VM.lagrange_sides(power, sid, logs[PM.SOURCE[sid]], blk, x, _mu(seed))
        assert left != right                                                          # the μ_p: refused


def test_the_truth_names_the_listed_bits():
    """the specification's table of faults in sections 2 to 6, on logarithms"""
    power, c = 3, 0x1234567
    N = 1 << power
    tau = TAUS["random"]
    sound = VM.sound_logs(power, tau, ALPHA, BETA, prepared=False)

    def bits(change):
        logs = {k: list(v) for k, v in sound.items()}
        change(logs)
        ok, kind, mask, fault = VM.truth(power, logs)
        assert ok == (mask == 0) and fault is None and (kind == 0) == (mask == 0) and (mask == 0 or mask & VM.bit(kind) and not mask & (VM.bit(kind) - 1))
        return mask

    def times(s, k):
        def f(logs):
            logs[s][k] = logs[s][k] * c % R
        return f

    def swap(logs):
        logs[2][3], logs[2][9] = logs[2][9], logs[2][3]

    def whole(s):
        def f(logs):
            logs[s] = [v * c % R for v in logs[s]]
        return f

    def other_tau(logs):
        logs[4] = [ALPHA * pow(tau + 1, i, R) % R for i in range(N)]

    B = VM.bit
    for k in (2, N, 2 * N - 2):
        assert bits(times(2, k)) == B(VM.TAU_G1)
    assert bits(times(2, 1)) == B(VM.TAU_G1) | B(VM.TAU_PAIR)
    assert bits(swap) == B(VM.TAU_G1)
    assert bits(times(3, 5)) == B(VM.TAU_G2)
    assert bits(other_tau) == B(VM.ALPHA_TAU)
    assert bits(whole(5)) == B(VM.BETA_PAIR)
    assert bits(times(6, 0)) == B(VM.BETA_PAIR)
    assert bits(whole(2)) == B(VM.GENERATORS) | B(VM.TAU_PAIR)
    assert bits(lambda logs: None) == 0
    # an identity is a verdict of its own, section 6 first, the lowest element
    logs = {k: list(v) for k, v in sound.items()}
    logs[2][4] = logs[2][7] = 0
    assert VM.truth(power, logs) == (False, VM.IDENTITY, 0, (2, 4))
    logs[6][0] = 0
    assert VM.truth(power, logs) == (False, VM.IDENTITY, 0, (6, 0))
    # power 0: nothing to sum
    assert VM.truth(0, VM.sound_logs(0, tau, ALPHA, BETA, prepared=True)) == (True, 0, 0, None)


def test_x_lies_in_no_domain():
    for power in (0, 3, 27):
        for seed in SEEDS:
            x, c = VM.x_of(seed, power)
            assert 0 < x < R and pow(x, 2 << power, R) != 1 and c == 0                # a retry has probability 2^(power+1)/r
    assert VM.coefficient(SEEDS[0], 0) < 1 << 128 and VM.mu_of(SEEDS[0], 5) == VM.coefficient(SEEDS[0], (1 << 32) + 5)
