"""bn254_ntt at every size and on every path of its host plan (needs an MI355X), bit-exact against the CPU oracle.

csrc/ntt_plan.h: ntt_plan (walked on the host by tests/test_ntt_plan_host.py) switches on log2(n): one pass of the 8×32-bit kernel up to 2^9 (and two at 2^10), the lazy radix-2^29 passes from 2^11
to 2^24 (plan29: a pass plan of its own per size; bounds29: a value-bound plan per pass, with `shrink_last` where a sum would pass
its limit; the `xcd_batch` launch once tiles % 8 == 0), and the 8×32-bit three-pass plan again from 2^25 on, which plan29 does not
take.  Every log n from 0 to 24 runs here in a 2^24 domain (strides 2^24 … 1), six sizes again in a domain of their own size, one
transform at 2^25, cosets with arbitrary generators, the orderings at a three-pass size, inputs that drive the lazy field to its
bounds, and everything up to 2^20 once more on the 8×32-bit kernels behind ICICLE_SNARK_NTT29=0.  Inputs cover the whole field
(tests/fr_inputs.py): uniform in [0, r) with the edge values planted at the ends, the middle and the tile border 2047 | 2048."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fr_inputs import R_MOD, edge_fr_arr, ints_to_arr, rand_fr_full

pytestmark = pytest.mark.gpu

BIG = 24                                   # the module's domain: the largest size the radix-2^29 plan takes
NN, NR, RN, RR, NM, MN = range(6)          # Ordering (include/icicle_snark_hip.h)
# coset generators: any field element is allowed (NTTConfig.coset_gen), not only roots of unity
COSET_G = {
    "rand": 0x2B5C93A7E1D04F6688A1F3C2957E0B4D6C1A9F8E7D3B2C5A4F6E8D7C9B0A1F23,   # above 2^253, below r
    "gen": 5,                                                                     # the multiplicative generator of Fr
}
UP_TO_20 = list(range(0, 21))
ABOVE_20 = [21, 22, 23, 24]
OWN_DOMAIN = [11, 12, 14, 16, 17, 20]
COSET_LOGS = [0, 1, 9, 10, 11, 14, 16, 17, 19]

_domain = {"log": None}


def _use_domain(K, log):
    """bn254_ntt_init_domain silently keeps an existing domain: release first whenever the size changes"""
    if _domain["log"] != log:
        K.release_domain()
        K.initialize_domain(K.get_root_of_unity(1 << log))
        _domain["log"] = log


@pytest.fixture(scope="module", autouse=True)
def _domain_released_before_and_after(gpu):
    gpu.release_domain()
    _domain["log"] = None
    yield
    gpu.release_domain()
    _domain["log"] = None


def batch_of(logn):
    """3 rows up to 2^20, 2 rows at 2^21 and 2^22 (a 3-pass plan with batch > 1 in both launch shapes), 1 row above"""
    return 3 if logn <= 20 else 2 if logn <= 22 else 1


def _inputs(logn, batch, seed):
    """(batch·n, 4): uniform over the whole field; every row carries edge values first, last, at n/2 and on both sides of the
    tile border (2047, 2048), a different stretch of the edge list per row and size; the whole list once across the border"""
    n = 1 << logn
    x = rand_fr_full(np.random.default_rng(seed), batch * n).reshape(batch, n, 4)
    E = edge_fr_arr()
    if n >= 4096:
        x[0, 2048 - len(E) // 2: 2048 - len(E) // 2 + len(E)] = E
    elif n >= 4 * len(E):
        x[0, n // 4: n // 4 + len(E)] = E
    for b in range(batch):
        for i, p in enumerate((0, n - 1, n // 2, 2047, 2048)):
            if p < n:
                x[b, p] = E[(i + 5 * b + 15 * logn) % len(E)]
    return np.ascontiguousarray(x.reshape(-1, 4))


def _check_against_oracle(K, O, logn, domain_log, batch, seed):
    """forward and inverse: host in/out; in place on the device, asynchronous on a stream, with both round trips"""
    x = _inputs(logn, batch, seed)
    want_f = O.fr_ntt(x, False, batch=batch, domain_log=domain_log)
    want_i = O.fr_ntt(x, True, batch=batch, domain_log=domain_log)
    assert np.array_equal(K.ntt(x, False, batch_size=batch), want_f), "forward, host"
    assert np.array_equal(K.ntt(x, True, batch_size=batch), want_i), "inverse, host"
    st = K.IcicleStream()
    d = K.DeviceVec.from_host(x, st)
    K.ntt(d, False, batch_size=batch, stream=st, is_async=True)
    assert np.array_equal(d.to_host(x.shape, stream=st), want_f), "forward, in place on the device"
    K.ntt(d, True, batch_size=batch, stream=st, is_async=True)
    assert np.array_equal(d.to_host(x.shape, stream=st), x), "forward then inverse"
    K.ntt(d, True, batch_size=batch, stream=st, is_async=True)
    assert np.array_equal(d.to_host(x.shape, stream=st), want_i), "inverse, in place on the device"
    K.ntt(d, False, batch_size=batch, stream=st, is_async=True)
    assert np.array_equal(d.to_host(x.shape, stream=st), x), "inverse then forward"
    st.destroy()
    d.free()


@pytest.mark.parametrize("logn", UP_TO_20, ids=lambda v: f"log{v:02d}")
def test_ntt_every_log_in_the_2p24_domain(gpu, O, logn):
    """logs 0 … 20, batch 3, domain 2^24 (stride 2^24 … 2^4).  Radix-2^29 pass plans: 11 [6,5] (one tile), 12 [6,6], 13 [8,5],
    14 [8,6] (first xcd_batch launch), 15 [8,7] (shrink_last in the inverse's last pass), 16 [8,8] (shrink_last both ways),
    17 [6,6,5] (first 3-pass), 18 [6,6,6], 19 [8,6,5], 20 [8,6,6]"""
    _use_domain(gpu, BIG)
    _check_against_oracle(gpu, O, logn, BIG, batch_of(logn), seed=1000 + logn)


@pytest.mark.parametrize("logn", ABOVE_20, ids=lambda v: f"log{v:02d}")
def test_ntt_every_log_in_the_2p24_domain_above_2p20(gpu, O, logn):
    """21 [8,8,5] (shrink in the middle pass), 22 [8,8,6] — batch 2 —, 23 [8,8,7], 24 [8,8,8] (shrink in two passes, stride 1) —
    batch 1"""
    _use_domain(gpu, BIG)
    _check_against_oracle(gpu, O, logn, BIG, batch_of(logn), seed=1000 + logn)


@pytest.mark.parametrize("logn", OWN_DOMAIN, ids=lambda v: f"log{v:02d}")
def test_ntt_in_a_domain_of_its_own_size(gpu, O, logn):
    """domain == n: twiddle stride 1 on 2-pass (11, 12, 14, 16) and 3-pass (17, 20) plans"""
    _use_domain(gpu, logn)
    _check_against_oracle(gpu, O, logn, logn, 3, seed=2000 + logn)


@pytest.mark.parametrize("logn", list(range(11, 25)), ids=lambda v: f"log{v:02d}")
def test_ntt_radix29_bound_plan_holds_for_the_worst_inputs(gpu, logn):
    """The radix-2^29 passes do not reduce after additions; bounds29 plans how far the values may grow.  Three rows drive every
    sub-transform to its bound: all r − 1 (the all-sums path: element 0 becomes n·(r − 1)), 0 / r − 1 alternating, and
    r − 1 / 1 alternating (the difference paths).  Their transforms are known in closed form — only elements 0 and n/2 are not
    zero — so every radix-2^29 size up to 2^24 is checked without the oracle's time:
        row 0: X[0] = −n                      row 1: X[0] = −n/2, X[n/2] = n/2               row 2: X[0] = 0, X[n/2] = −n
    and the inverse transform is the same times 1/n (ω^(n/2) = ω^(−n/2) = −1)."""
    K = gpu
    _use_domain(K, BIG)
    n = 1 << logn
    rm1 = ints_to_arr([R_MOD - 1])[0]
    x = np.tile(rm1, (3, n, 1))
    x[1, 0::2] = 0
    x[2, 1::2] = ints_to_arr([1])[0]
    x = np.ascontiguousarray(x.reshape(-1, 4))
    nonzero = {(0, 0): -n, (1, 0): -(n // 2), (1, n // 2): n // 2, (2, n // 2): -n}
    for inverse in (False, True):
        got = K.ntt(x, inverse, batch_size=3)
        scale = pow(n, -1, R_MOD) if inverse else 1
        want = {b * n + k: v * scale % R_MOD for (b, k), v in nonzero.items()}
        where = np.flatnonzero(got.any(axis=1))
        assert where.tolist() == sorted(want), (logn, inverse, where[:8])
        assert np.array_equal(got[where], ints_to_arr([want[i] for i in where.tolist()])), (logn, inverse)


# ---------------------------------------------------------------------------------------------------------------- cosets
_gpow_cache = {}


def _gpows(g, n):
    if (g, n) not in _gpow_cache:
        p = [1] * n
        for j in range(1, n):
            p[j] = p[j - 1] * g % R_MOD
        _gpow_cache.clear()              # one table at a time (2^19 Python integers)
        _gpow_cache[(g, n)] = p
    return _gpow_cache[(g, n)]


def _shift(O, a, n, g):
    """a[b·n + j] · g^j in Python integers"""
    p = _gpows(g, n)
    return O.ints_to_arr([v * p[j % n] % R_MOD for j, v in enumerate(O.arr_to_ints(a))])


def _coset_model(O, x, n, batch, g, inverse):
    """forward: the transform of x_j·g^j (evaluation on g·H); inverse: the inverse transform, then ·g^(−j)"""
    if not inverse:
        return O.fr_ntt(_shift(O, x, n, g), False, batch=batch, domain_log=BIG)
    return _shift(O, O.fr_ntt(x, True, batch=batch, domain_log=BIG), n, pow(g, -1, R_MOD))


@pytest.mark.parametrize("gname", sorted(COSET_G))
@pytest.mark.parametrize("batch", [1, 3], ids=lambda v: f"batch{v}")
@pytest.mark.parametrize("logn", COSET_LOGS, ids=lambda v: f"log{v:02d}")
def test_ntt_coset_arbitrary_generator(gpu, O, logn, batch, gname):
    """coset_mul_kernel and the buffers around it (the pre-multiplied copy in scratch that the first pass then reads, the
    post-multiplication of the last pass's output): n = 1 and 2, the 8×32-bit sizes 2^9 and 2^10, radix-2^29 2-pass (11, 14, 16)
    and 3-pass (17, 19) plans; one row and three; host arrays and in place on the device."""
    K = gpu
    _use_domain(K, BIG)
    n = 1 << logn
    g = COSET_G[gname]
    cg = ints_to_arr([g])[0]
    x = _inputs(logn, batch, seed=3000 + logn)
    want_f = _coset_model(O, x, n, batch, g, False)
    want_i = _coset_model(O, x, n, batch, g, True)
    got_f = K.ntt(x, False, batch_size=batch, coset_gen=cg)
    assert np.array_equal(got_f, want_f), "forward, host"
    assert np.array_equal(K.ntt(x, True, batch_size=batch, coset_gen=cg), want_i), "inverse, host"
    assert np.array_equal(K.ntt(got_f, True, batch_size=batch, coset_gen=cg), x), "round trip, host"
    st = K.IcicleStream()
    d = K.DeviceVec.from_host(x, st)
    K.ntt(d, False, batch_size=batch, coset_gen=cg, stream=st, is_async=True)
    assert np.array_equal(d.to_host(x.shape, stream=st), want_f), "forward, in place on the device"
    K.ntt(d, True, batch_size=batch, coset_gen=cg, stream=st, is_async=True)
    assert np.array_equal(d.to_host(x.shape, stream=st), x), "round trip, in place on the device"
    K.ntt(d, True, batch_size=batch, coset_gen=cg, stream=st, is_async=True)
    assert np.array_equal(d.to_host(x.shape, stream=st), want_i), "inverse, in place on the device"
    st.destroy()
    d.free()


def _bitrev_index(logn):
    i = np.arange(1 << logn, dtype=np.int64)
    r = np.zeros_like(i)
    for k in range(logn):
        r |= ((i >> k) & 1) << (logn - 1 - k)
    return r


def _caller_layout(a, n, batch, reversed_order, columns):
    """rows in natural order (batch·n, 4) → what the caller holds: bit-reversed index and / or element i of row b at b + i·batch"""
    a = a.reshape(batch, n, 4)
    if reversed_order:
        a = a[:, _bitrev_index(n.bit_length() - 1)]
    if columns:
        a = a.transpose(1, 0, 2)
    return np.ascontiguousarray(a).reshape(-1, 4)


@pytest.mark.parametrize("columns", [False, True], ids=["rows", "columns"])
@pytest.mark.parametrize("ordering", [NR, RN], ids=["kNR", "kRN"])
@pytest.mark.parametrize("logn", [11, 14], ids=lambda v: f"log{v:02d}")
def test_ntt_coset_with_orderings_and_columns_batch(gpu, O, logn, ordering, columns):
    """the coset powers follow the NATURAL index j whatever the caller's layout (icicle/include/icicle/ntt.h:52-64): the re-layout
    pass runs before the pre-multiplication and after the post-multiplication"""
    K = gpu
    _use_domain(K, BIG)
    n, batch = 1 << logn, 3
    g = COSET_G["rand"]
    cg = ints_to_arr([g])[0]
    x = _inputs(logn, batch, seed=4000 + logn)
    given = _caller_layout(x, n, batch, ordering == RN, columns)
    for inverse in (False, True):
        want = _caller_layout(_coset_model(O, x, n, batch, g, inverse), n, batch, ordering == NR, columns)
        got = K.ntt(given, inverse, batch_size=batch, coset_gen=cg, ordering=ordering, columns_batch=columns)
        assert np.array_equal(got, want), ("host", inverse)
        d = K.DeviceVec.from_host(given)
        K.ntt(d, inverse, batch_size=batch, coset_gen=cg, ordering=ordering, columns_batch=columns)
        assert np.array_equal(d.to_host(given.shape), want), ("in place on the device", inverse)
        d.free()


@pytest.mark.parametrize("columns", [False, True], ids=["rows", "columns"])
def test_ntt_orderings_at_a_three_pass_size(gpu, O, columns):
    """kNR / kRN / kRR / kNM / kMN and columns_batch at 2^17 (radix-2^29 [6,6,5]) in the 2^24 domain, three rows"""
    K = gpu
    _use_domain(K, BIG)
    logn, batch = 17, 3
    n = 1 << logn
    x = _inputs(logn, batch, seed=5000)
    for inverse in (False, True):
        want = O.fr_ntt(x, inverse, batch=batch, domain_log=BIG)
        for ordering, rev_in, rev_out in ((NN, 0, 0), (NR, 0, 1), (RN, 1, 0), (RR, 1, 1), (NM, 0, 1), (MN, 1, 0)):
            given = _caller_layout(x, n, batch, rev_in, columns)
            expect = _caller_layout(want, n, batch, rev_out, columns)
            got = K.ntt(given, inverse, batch_size=batch, ordering=ordering, columns_batch=columns)
            assert np.array_equal(got, expect), ("host", inverse, ordering)
            d = K.DeviceVec.from_host(given)
            K.ntt(d, inverse, batch_size=batch, ordering=ordering, columns_batch=columns)
            assert np.array_equal(d.to_host(given.shape), expect), ("in place on the device", inverse, ordering)
            d.free()


# ------------------------------------------------------------------------------------- sizes the radix-2^29 plan does not take
def test_ntt_2p25_on_the_8x32_three_pass_kernels(gpu, O):
    """plan29 has no plan for 2^25 (three passes of at most 8 bits): the transform runs on the 8×32-bit kernels with passes of
    9, 8 and 8 bits, in a 2^25 domain.  Checked through the even / odd split of the reference's own identity test
    (ntt/tests.rs:99-166): out[k] = E[k mod n] + ω_2n^k · O[k mod n], where E and O are this library's 2^24 transforms of the
    even and odd elements — a size pinned to the oracle above — evaluated in Python integers at k = 0, n − 1, n, 2n − 1, around
    the tile borders and at 2^14 random places; then the full round trip."""
    K = gpu
    n = 1 << BIG
    x = _inputs(BIG + 1, 1, seed=6000)
    _use_domain(K, BIG)
    ev = K.ntt(np.ascontiguousarray(x[0::2]), False)
    od = K.ntt(np.ascontiguousarray(x[1::2]), False)
    _use_domain(K, BIG + 1)
    got = K.ntt(x, False)
    w = O.fr_omega(BIG + 1)
    rng = np.random.default_rng(6001)
    ks = [0, 1, n - 1, n, n + 1, 2 * n - 1, 2047, 2048, n + 2047, n + 2048, n // 2, n + n // 2]
    ks += rng.integers(0, 2 * n, size=1 << 14).tolist()
    ks = np.array(ks, dtype=np.int64)
    e_s, o_s, g_s = O.arr_to_ints(ev[ks % n]), O.arr_to_ints(od[ks % n]), O.arr_to_ints(got[ks])
    for k, e, o, v in zip(ks.tolist(), e_s, o_s, g_s):
        assert v == (e + pow(w, k, R_MOD) * o) % R_MOD, k
    del ev, od
    assert np.array_equal(K.ntt(got, True), x), "round trip"


# ----------------------------------------------------------------------------------------------- the 8×32-bit kernels at every size
NOT_IN_THE_CHILD = ("above_2p20", "radix29", "2p25", "behind_the_switch")


def _cases(fn):
    total = 1
    for m in getattr(fn, "pytestmark", []):
        if m.name == "parametrize":
            total *= len(m.args[1])
    return total


def test_every_case_up_to_2p20_on_the_8x32_kernels_behind_the_switch():
    """ICICLE_SNARK_NTT29=0 — and a domain whose Montgomery-261 twiddle table could not be allocated — sends every size through
    the 8×32-bit pass kernels (2-pass up to 2^18, 3-pass above), which otherwise see only sizes below 2^11 and above 2^24.  The
    switch is read once per process: every oracle comparison of this module with log n ≤ 20 runs again in one child process."""
    mod = sys.modules[__name__]
    names = [name for name in dir(mod) if name.startswith("test_") and not any(tag in name for tag in NOT_IN_THE_CHILD)]
    expected = sum(_cases(getattr(mod, name)) for name in names)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", " and ".join(f"not {tag}" for tag in NOT_IN_THE_CHILD)],
                         capture_output=True, text=True, env=dict(os.environ, ICICLE_SNARK_NTT29="0"), timeout=1500)
    assert out.returncode == 0 and f"{expected} passed" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
