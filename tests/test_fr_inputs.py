"""The full-range input helpers of the GPU tests (tests/fr_inputs.py) do what they say — CPU only."""
import numpy as np

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
