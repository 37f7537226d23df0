"""icicle_snark_msm_segmented (csrc/prover/msm_segmented.hip) against the CPU oracle's MSM, segment by segment and bit for bit.

The shapes are the smallest that reach every branch of the two kernels: segment lengths around the wave (63 | 64 | 65) and the
workgroup (255 | 256 | 257 — the first length at which a lane holds two entries), empty segments (two side by side, one at the end),
segments just past one and two default cuts (a lane with four entries; the second launch with two and three pieces), and `cut`
small enough that every segment is cut.  Scalars: the edge set of tests/msm_inputs.py.  Points: the identity, one point repeated
(P + P inside a lane and in the LDS tree), P beside −P with equal scalars, a segment whose sum is the identity.
A scalar of 2^128 or more in a 128-bit segment is the caller's error (include/icicle_snark_hip.h) and is not tested."""
import numpy as np
import pytest

from fr_inputs import R_MOD, ints_to_arr, rand_fr_full
from msm_inputs import recode_limits

pytestmark = pytest.mark.gpu

DEFAULT_CUT = 1024          # DEFAULT_SEGMENT_CUT of csrc/prover/msm_segmented.hip
LENGTHS = [0, 1, 2, 63, 0, 0, 64, 65, 255, 256, 257, 2, 2, 0]
BITS = [254, 128, 254, 128, 128, 254, 254, 128, 254, 128, 254, 254, 128, 254]
EDGE_128 = [0, 1, (1 << 128) - 1, 1 << 127, (1 << 127) - 1, (1 << 64) - 1, 1 << 64, 1 << 32, (1 << 29) - 1]
EDGE_254 = EDGE_128 + [R_MOD - 1, R_MOD - 2, 1 << 253, (1 << 253) - 1, (1 << 253) + 1] + recode_limits()


def _neg(O, p):
    """−P of a standard-form affine point (2, 4)"""
    y = O.arr_to_ints(p[1:2])[0]
    out = p.copy()
    out[1] = O.ints_to_arr([(O.Q_MOD - y) % O.Q_MOD])[0]
    return out


def _scalars(rng, n, bits, edges):
    """n scalars below 2^bits (and r) with the edge values planted from the front, as many as fit"""
    sc = rand_fr_full(rng, n)
    if bits == 128:
        sc[:, 2:] = 0
    k = min(n, len(edges))
    if k:
        at = rng.permutation(n)[:k]
        sc[at] = ints_to_arr(edges[:k])
    return sc


def _points(O, rng, n):
    G = O.ec_to_affine("g1", O.ec_generator("g1"))
    return O.fixed_base_mul("g1", G, rand_fr_full(rng, n)).reshape(n, 2, 4)


def _plant(O, pts, sc, lo, n, stride):
    """inside [lo, lo + n): an identity point, P twice `stride` apart with scalar 1 and with one full scalar (P + P: the doubling
    branch, in one lane when stride is the workgroup's width), P and −P `stride` apart with equal scalars (cancellation)"""
    if n < 3:
        return
    pts[lo + n // 2] = 0
    if n <= stride + 3:
        return
    pts[lo + stride] = pts[lo]
    sc[lo] = sc[lo + stride] = ints_to_arr([1])[0]
    pts[lo + 1 + stride] = pts[lo + 1]
    sc[lo + 1 + stride] = sc[lo + 1]
    pts[lo + 2 + stride] = _neg(O, pts[lo + 2])
    sc[lo + 2 + stride] = sc[lo + 2]


def _reference(O, pts, sc, offsets):
    """the oracle's MSM per segment as canonical affine, (0, 0) for the identity; identity points contribute nothing"""
    out = np.zeros((len(offsets) - 1, 2, 4), dtype=np.uint64)
    for s in range(len(offsets) - 1):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        keep = [k for k in range(lo, hi) if pts[k].any()]
        if not keep:
            continue
        acc = O.msm("g1", sc[keep], pts[keep], naive=len(keep) <= 300)
        if acc[2].any():
            out[s] = O.ec_to_affine("g1", acc)
    return out


@pytest.fixture(scope="module")
def small(O):
    rng = np.random.default_rng(20240611)
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.uint64)
    n = int(offsets[-1])
    pts = _points(O, rng, n)
    sc = np.zeros((n, 4), dtype=np.uint64)
    for s, (ln, b) in enumerate(zip(LENGTHS, BITS)):
        lo = int(offsets[s])
        sc[lo:lo + ln] = _scalars(rng, ln, b, EDGE_128 if b == 128 else EDGE_254)
        _plant(O, pts, sc, lo, ln, 1 if ln < 257 else 256)
    # the two 2-entry segments: P + P in the LDS tree, and P + (−P): a segment whose sum is the identity
    a, b = int(offsets[11]), int(offsets[12])
    pts[a + 1], sc[a + 1] = pts[a], sc[a]
    pts[b + 1], sc[b + 1] = _neg(O, pts[b]), sc[b]
    want = _reference(O, pts, sc, offsets)
    assert not want[12].any() and want[11].any() and not want[0].any()
    return pts, sc, offsets, np.array(BITS, dtype=np.uint8), want


def test_every_length_in_one_call(gpu, small):
    pts, sc, offsets, bits, want = small
    got = gpu.msm_segmented(pts, sc, offsets, bits)
    for s in range(len(bits)):
        assert np.array_equal(got[s], want[s]), (s, LENGTHS[s], int(bits[s]))


@pytest.mark.parametrize("cut", [1, 4, 64, 0])
def test_output_bytes_do_not_depend_on_cut(gpu, small, cut):
    pts, sc, offsets, bits, want = small
    got = gpu.msm_segmented(pts, sc, offsets, bits, cut=cut)
    assert got.tobytes() == want.tobytes()


def test_segments_past_the_default_cut(gpu, O):
    """DEFAULT_CUT + 1 entries (two pieces, 128 bits) and 2·DEFAULT_CUT + 1 (three pieces, 254 bits) beside an uncut and an empty
    segment; in the full pieces a lane holds four entries, 256 apart: P + P and P − P are planted at that stride"""
    rng = np.random.default_rng(77)
    lengths = [DEFAULT_CUT + 1, 3, 2 * DEFAULT_CUT + 1, 0]
    bits = np.array([128, 254, 254, 128], dtype=np.uint8)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    n = int(offsets[-1])
    pts = _points(O, rng, n)
    sc = np.zeros((n, 4), dtype=np.uint64)
    for s, ln in enumerate(lengths):
        lo = int(offsets[s])
        sc[lo:lo + ln] = _scalars(rng, ln, int(bits[s]), EDGE_128 if bits[s] == 128 else EDGE_254)
        _plant(O, pts, sc, lo, ln, 256)
    want = _reference(O, pts, sc, offsets)
    got = gpu.msm_segmented(pts, sc, offsets, bits)
    assert got.tobytes() == want.tobytes()
    assert gpu.msm_segmented(pts, sc, offsets, bits, cut=DEFAULT_CUT).tobytes() == want.tobytes()


def test_bad_plans_are_refused_on_the_host(gpu, small):
    pts, sc, offsets, bits, _ = small
    down = offsets.copy()
    down[3] = down[2] - 1
    with pytest.raises(gpu.IcicleError):
        gpu.msm_segmented(pts, sc, down, bits)
    odd = bits.copy()
    odd[1] = 64
    with pytest.raises(gpu.IcicleError):
        gpu.msm_segmented(pts, sc, offsets, odd)
    assert gpu.msm_segmented(pts[:0], sc[:0], np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint8)).shape == (0, 2, 4)
