"""bn254_msm / bn254_g2_msm at every window geometry of their host plan (needs an MI355X), bit-exact against the CPU oracle.

msm_geometry (csrc/msm_recode.h) and msm_sort_shape (csrc/msm_sort_plan.h) switch on the length L: automatic c = ⌈log2 L⌉ − 4 in the
classic layout, with the top windows narrowed by one bit at c = 5, 8, 15, 16; behind device-resident bases of 2^15 points and more
the table mode with c = 15 (two-level sort: 17 windows), 16, 17, 19 (twelve of fourteen windows narrowed) and 20, whose table
msm_table_refresh_kernel rebuilds from (c, W, wide) when the bases change behind the library's back.  DESIGN.md §6 has the table.
Every length here is the smallest of its bracket; the scalars cover the whole field and carry, at the tile borders of the digit
sorts, the values at which a recoding goes wrong FOR THE GEOMETRY THAT RUNS (tests/msm_inputs.py): one digit alone in each
window, each window's negative extreme with its carry, all-ones below, r − v of each, the negation threshold (r − 1)/2, 2^253.
After every call the geometry the library reports (icicle_snark_msm_profile) is held against the table of this file: a sweep
that ran another path than it names fails.

Each test prints the seconds it spent in the oracle and in the library's calls (pytest -rP shows them)."""
import ctypes as C
import time

import numpy as np
import pytest

import msm_inputs as MI
from fr_inputs import ints_to_arr
from test_gpu_ops import DIMS, _bases

pytestmark = pytest.mark.gpu

# L: ((c, W, nbuckets) of the first call over fresh device-resident bases — classic layout —, of the calls on the table)
TABLE_SWEEP = {
    32768: ((11, 24, 24576), (15, 17, 16384)),      # the only length with c = 15: W > 16 keeps it off the LDS-staged sort
    32769: ((12, 22, 45056), (16, 16, 32768)),
    65537: ((13, 20, 81920), (17, 15, 65536)),      # two pseudo-windows of 32768 buckets in the reduction
    262145: ((15, 17, 278528), (19, 14, 262144)),   # wide = 2: twelve of fourteen windows narrowed
    524289: ((16, 16, 524288), (20, 13, 524288)),
}
# L: (c, W) of the classic layout with host-resident bases; nbuckets = W · 2^(c − 1)
CLASSIC_SWEEP = {257: (5, 51), 1025: (7, 37), 2049: (8, 32), 4097: (9, 29), 131073: (14, 19)}
REFRESH_AT = [("g1", 32768), ("g1", 262145), ("g1", 524289), ("g2", 262145)]
MONTGOMERY_AT = {("g1", 32768), ("g2", 262145), ("g1", 65537), ("g2", 32769)}   # refresh test: the first two; table sweep: the others

_host_bases = {}


@pytest.fixture(scope="module", autouse=True)
def _oracle_threads(O):
    O.calibrate_threads()


def bases_of(O, grp, L):
    """test_gpu_ops._bases: 100 distinct points repeated (P + P occurs), two identities; built once per (group, L), never written"""
    if (grp, L) not in _host_bases:
        b = _bases(O, grp, np.random.default_rng(L + (7 if grp == "g2" else 0)), L)
        b[1] = 0
        b[L - 1] = 0
        b.setflags(write=False)
        _host_bases[grp, L] = b
    return _host_bases[grp, L]


class Clock:
    """seconds in the oracle and in the library, per test"""

    def __init__(self, O, K):
        self.O, self.K, self.oracle_s, self.gpu_s = O, K, 0.0, 0.0

    def want(self, grp, sc, bases):
        t0 = time.perf_counter()
        out = self.O.ec_to_affine(grp, self.O.msm(grp, sc, bases))
        self.oracle_s += time.perf_counter() - t0
        return out

    def msm(self, grp, *args, sync=None, **kw):
        t0 = time.perf_counter()
        out = self.K.msm(grp, *args, **kw)
        if sync is not None:
            sync.synchronize()
        self.gpu_s += time.perf_counter() - t0
        return out

    def report(self, what):
        print(f"[msm plans] {what}: oracle {self.oracle_s:.2f} s, library calls {self.gpu_s:.3f} s")


def assert_profile(K, grp, L, c, W, nbuckets):
    g = K.msm_profile(0)[1]
    assert (g["L"], g["c"], g["W"], g["nbuckets"], g["is_g2"]) == (L, c, W, nbuckets, grp == "g2"), g


def affine(K, grp, res):
    return K.ec(grp, "to_affine", res)


def _vector(kind, L, geoms, seed, rot=0):
    rng = np.random.default_rng(seed)
    return MI.edge_vector(rng, L, geoms, rot) if kind == "edge" else MI.skewed_vector(rng, L)


@pytest.mark.parametrize("kind", ["edge", "skewed"])
@pytest.mark.parametrize("L", sorted(TABLE_SWEEP))
@pytest.mark.parametrize("grp", ["g1", "g2"])
def test_table_sweep(gpu, O, grp, L, kind):
    """classic → table build → table hit over device-resident bases, automatic c.  The edge vector carries the window edges of the
    table geometry and, behind them, those of the first call's classic geometry; the skewed one puts 3/10 of its entries into
    bucket 0 (several 1024-entry work items of the large-bucket kernels) and 1/10 at r − 1."""
    K = gpu
    clk = Clock(O, K)
    classic, table = TABLE_SWEEP[L]
    assert (classic[:2], table[:2]) == (MI.TABLE_FIRST_CALL_GEOMS[L][:2], MI.TABLE_GEOMS[L][:2])
    bases = bases_of(O, grp, L)
    sc = _vector(kind, L, [MI.TABLE_GEOMS[L], MI.TABLE_FIRST_CALL_GEOMS[L]], seed=L + (1 if kind == "edge" else 2))
    want = clk.want(grp, sc, bases)
    d_b, d_s = K.DeviceVec.from_host(bases), K.DeviceVec.from_host(sc)   # (the upload retires whatever table the address had)
    for call, geom in enumerate((classic, table, table)):
        got = clk.msm(grp, d_s, d_b)
        assert_profile(K, grp, L, *geom)
        assert np.array_equal(affine(K, grp, got), want), (call, geom)
    if kind == "edge" and (grp, L) in MONTGOMERY_AT:
        K.scalar_convert_montgomery(d_s, True)
        got = clk.msm(grp, d_s, d_b, scalars_mont=True)
        assert_profile(K, grp, L, *table)
        assert np.array_equal(affine(K, grp, got), want), "Montgomery-form scalars"
    d_b.free(); d_s.free()
    clk.report(f"table sweep {grp} {L} {kind}")


@pytest.mark.parametrize("grp,L", REFRESH_AT)
def test_table_refresh_at_every_width(gpu, O, grp, L):
    """msm_table_refresh_kernel(c, W, wide) at c = 15, 19 and 20 (G1) and 19 (G2): three bases — index 0, index 1023 (the last
    scalar of the sort's first tile) and index L − 1 — are overwritten by a raw hipMemcpy the library cannot see, and the next two
    calls, on fresh edge scalars, give the oracle's sum over the NEW bases (first the refreshed table, then a plain hit)."""
    K = gpu
    clk = Clock(O, K)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipDeviceSynchronize.argtypes = []
    classic, table = TABLE_SWEEP[L]
    geoms = [MI.TABLE_GEOMS[L], MI.TABLE_FIRST_CALL_GEOMS[L]]
    bases = bases_of(O, grp, L).copy()
    d_b = K.DeviceVec.from_host(bases)
    d_s = K.DeviceVec.from_host(_vector("edge", L, geoms, seed=3 * L))
    first = clk.msm(grp, d_s, d_b)
    assert_profile(K, grp, L, *classic)
    built = clk.msm(grp, d_s, d_b)
    assert_profile(K, grp, L, *table)
    assert np.array_equal(first, built) or np.array_equal(affine(K, grp, first), affine(K, grp, built))   # (the sweep holds both against the oracle)
    d_s.free()
    psize = bases[0].nbytes
    fresh = _bases(O, grp, np.random.default_rng(5 * L), 3)
    assert hip.hipDeviceSynchronize() == 0
    for k, i in enumerate((0, 1023, L - 1)):
        bases[i] = fresh[k]
        a = np.ascontiguousarray(bases[i])
        assert hip.hipMemcpy(C.c_void_p(d_b.ptr + i * psize), a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0   # hipMemcpyHostToDevice
    sc = _vector("edge", L, geoms, seed=7 * L, rot=41)
    sc[[0, 1023, L - 1]] = ints_to_arr([MI.HALF, MI.HALF + 1, (1 << 253) + 1])       # dense digits: every row of the rewritten bases is used
    want = clk.want(grp, sc, bases)
    d_s = K.DeviceVec.from_host(sc)
    for call in ("refresh", "hit"):
        got = clk.msm(grp, d_s, d_b)
        assert_profile(K, grp, L, *table)
        assert np.array_equal(affine(K, grp, got), want), call
    if (grp, L) in MONTGOMERY_AT:
        K.scalar_convert_montgomery(d_s, True)
        got = clk.msm(grp, d_s, d_b, scalars_mont=True)
        assert_profile(K, grp, L, *table)
        assert np.array_equal(affine(K, grp, got), want), "Montgomery-form scalars"
    d_b.free(); d_s.free()
    clk.report(f"table refresh {grp} {L}")


@pytest.mark.parametrize("kind", ["edge", "skewed"])
@pytest.mark.parametrize("L", sorted(CLASSIC_SWEEP))
@pytest.mark.parametrize("grp", ["g1", "g2"])
def test_classic_sweep(gpu, O, grp, L, kind):
    """host-resident bases — no table is ever built — at automatic c = 5, 7, 8, 9, 14 with buckets that fill: once host in / host
    out, once with scalars and result on the device, asynchronous on a stream.  Where the edge list is longer than the vector
    (257 scalars) the two runs carry its two halves."""
    K = gpu
    clk = Clock(O, K)
    c, W = CLASSIC_SWEEP[L]
    assert (c, W) == MI.CLASSIC_GEOMS[L][:2]
    nb = W << (c - 1)
    bases = bases_of(O, grp, L)
    sc = _vector(kind, L, MI.CLASSIC_GEOMS[L], seed=L + 11)
    want = clk.want(grp, sc, bases)
    got = clk.msm(grp, sc, bases)                                           # host in, host out
    assert_profile(K, grp, L, c, W, nb)
    assert np.array_equal(affine(K, grp, got), want), "host"
    if kind == "edge":
        sc = _vector(kind, L, MI.CLASSIC_GEOMS[L], seed=L + 12, rot=L)
        want = clk.want(grp, sc, bases)
    st = K.IcicleStream()
    d_s = K.DeviceVec.from_host(sc, st)
    d_r = K.DeviceVec(32 * DIMS[grp][1], st)
    clk.msm(grp, d_s, bases, out=d_r, stream=st, is_async=True, sync=st)
    assert_profile(K, grp, L, c, W, nb)
    assert np.array_equal(affine(K, grp, d_r.to_host((DIMS[grp][1], 4), stream=st)), want), "device, asynchronous"
    st.destroy(); d_s.free(); d_r.free()
    clk.report(f"classic sweep {grp} {L} {kind}")


@pytest.mark.parametrize("grp", ["g1", "g2"])
def test_short_scalars_whose_top_window_holds_all_but_one_bit(gpu, O, grp):
    """MSMConfig.bitsize with bits mod c = c − 1: the top window would hold c − 1 bits of the scalar and has no room for the carry
    of the signed recoding — a short scalar is not negated out of the way as a full-width one is — so the plan adds a window
    (csrc/msm_recode.h; found by tests/msm_recode_check.cpp: every scalar with its top c − 1 bits set and a carry from below was
    lost).  (bits, c) = (64, 5), (64, 13), (13, 7) and the automatic c = 5 of 300 points at bitsize 64, with 2^bits − 1, the values
    whose top window is all ones over every lower window's two extremes, and precomputed bases."""
    K = gpu
    n = 300
    bases = bases_of(O, grp, n)
    rng = np.random.default_rng(64)
    for bits, c, W in ((64, 5, 14), (64, 13, 6), (13, 7, 3), (64, 0, 14), (63, 5, 13)):
        ce = c or 5
        vals = [int(v) % (1 << bits) for v in rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * 2 + rng.integers(0, 2, size=n, dtype=np.uint64)]
        top = ((1 << bits) - 1) >> (bits - bits % ce) << (bits - bits % ce) if bits % ce else 0      # the top window's bits, all ones
        edge = [(1 << bits) - 1, top, top | 1 << (bits - bits % ce - 1), top | ((1 << (bits - bits % ce - 1)) - 1), top | 1 << (ce - 1), 1, 0]
        vals[5:5 + len(edge)] = edge
        vals[n - 1] = (1 << bits) - 1
        sc = ints_to_arr(vals)
        want = O.ec_to_affine(grp, O.msm(grp, sc, bases))
        got = K.msm(grp, sc, bases, bitsize=bits, c=c)
        assert_profile(K, grp, n, ce, W, W << (ce - 1))
        assert np.array_equal(affine(K, grp, got), want), (bits, c)
        if (bits, c) == (64, 5):
            pre = K.msm_precompute_bases(grp, np.array(bases), 3, c=c, bitsize=bits)
            got = K.msm(grp, sc, pre, size=n, precompute_factor=3, bitsize=bits, c=c)
            assert np.array_equal(affine(K, grp, got), want), "precomputed bases"
