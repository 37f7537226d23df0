"""The full-range input helpers of the GPU tests (tests/fr_inputs.py, tests/field_inputs.py) do what they say — CPU only."""
import hashlib

import numpy as np

from field_inputs import Q_MOD, edge_field, rand_field

from fr_inputs import R_MOD, below_r, edge_fr, edge_fr_arr, ints_to_arr, rand_fr_full


def _ints(a):
    return [int.from_bytes(r.tobytes(), "little") for r in np.ascontiguousarray(a).view(np.uint8).reshape(-1, 32)]


def test_rand_fr_full_covers_the_field_above_2p253(O):
    assert R_MOD == O.R_MOD
    a = rand_fr_full(np.random.default_rng(1), 20000)
    assert a.shape == (20000, 4) and a.dtype == np.uint64
    v = _ints(a)
    assert all(0 <= x < R_MOD for x in v)
    above = sum(x >= 1 << 253 for x in v)
    # (r − 2^253) / r = 0.339: 6780 expected, standard deviation 67
    assert 6400 < above < 7150, above
    assert max(v) > R_MOD - (R_MOD >> 8) and min(v) < R_MOD >> 8
    # the same seed gives the same values; the limb-wise comparison with r agrees with Python's
    assert np.array_equal(a, rand_fr_full(np.random.default_rng(1), 20000))
    probe = ints_to_arr([0, R_MOD - 1, R_MOD, R_MOD + 1, (1 << 254) - 1, R_MOD - (1 << 64), R_MOD + (1 << 64), R_MOD - (1 << 192), R_MOD + (1 << 192)])
    assert below_r(probe).tolist() == [True, True, False, False, False, True, False, True, False]
    assert len(rand_fr_full(np.random.default_rng(2), 0)) == 0


def test_edge_list_is_present_and_in_range():
    e = edge_fr()
    r = R_MOD
    half = (r - 1) // 2
    for v in (0, 1, 2, r - 1, r - 2, half - 1, half, half + 1, (1 << 253) - 1, 1 << 253, (1 << 253) + 1, (1 << 32) - 1,
              (1 << 64) - 1, (1 << 64) + 1, (1 << 128) - 1, (1 << 128) + 1, (1 << 192) - 1, (1 << 192) + 1, (1 << 29) - 1, (1 << 232) + 1):
        assert v in e, hex(v)
    assert len(set(e)) == len(e) and all(0 <= v < r for v in e)
    assert sum(v >= 1 << 253 for v in e) >= 8
    assert _ints(edge_fr_arr()) == e


def test_edge_fr_is_the_list_it_has_always_been():
    """edge_fr now delegates to field_inputs: the existing GPU tests must see exactly the values they saw before"""
    e = edge_fr()
    assert len(e) == 48 and e[:5] == [0, 1, 2, R_MOD - 1, R_MOD - 2] and e[-1] == R_MOD >> 64 << 64
    assert hashlib.sha256(b"".join(v.to_bytes(32, "little") for v in e)).hexdigest() == "b077c07481ee7df1f61b6de8851318c538bee2426f522db25d47cc9225a914d4"
    assert edge_field(R_MOD)[:48] == e


def test_edge_field_generalises_to_fq_and_reaches_the_gap_above_r(O):
    assert Q_MOD == O.Q_MOD and Q_MOD > R_MOD
    for p in (R_MOD, Q_MOD):
        e = edge_field(p)
        half = (p - 1) // 2
        for v in (0, 1, 2, p - 1, p - 2, half - 1, half, half + 1, (1 << 253) - 1, 1 << 253, (1 << 253) + 1, (1 << 64) - 1, (1 << 32) + 1,
                  (1 << 29) - 1, (1 << 232) + 1, p - (1 << 64), p - (1 << 128) + 1, p >> 64 << 64, pow(2, 256, p), pow(2, 261, p), p - (1 << 32)):
            assert v in e, hex(v)
        assert len(set(e)) == len(e) and all(0 <= v < p for v in e)
    eq = edge_field(Q_MOD)
    assert sum(R_MOD <= v < Q_MOD for v in eq) >= 12 and R_MOD in eq and R_MOD + 1 in eq
    assert not any(v >= R_MOD for v in edge_field(R_MOD))


def test_rand_field_is_uniform_below_p():
    for p in (R_MOD, Q_MOD):
        v = rand_field(np.random.default_rng(3), 20000, p)
        assert len(v) == 20000 and all(0 <= x < p for x in v)
        above = sum(x >= 1 << 253 for x in v)
        assert 6400 < above < 7150, above                       # (p − 2^253) / p = 0.339, as for rand_fr_full
        assert v == rand_field(np.random.default_rng(3), 20000, p)
    assert rand_field(np.random.default_rng(3), 0, R_MOD) == []


def test_five_generates_the_multiplicative_group():
    """the coset tests use 5 as `the field's multiplicative generator`: 5^((r−1)/q) ≠ 1 for every prime q dividing r − 1"""
    primes = [2, 3, 13, 29, 983, 11003, 237073, 405928799, 1670836401704629, 13818364434197438864469338081]
    rest = R_MOD - 1
    for q in primes:
        assert all(pow(a, q - 1, q) == 1 for a in (2, 3, 5, 7) if a % q) and rest % q == 0
        while rest % q == 0:
            rest //= q
    assert rest == 1
    assert all(pow(5, (R_MOD - 1) // q, R_MOD) != 1 for q in primes)
