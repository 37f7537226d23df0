"""Checked host build of csrc/prover/ptau_contribute29.h — one lane of groth16_ptau_contribute: the scalar c·τ′^i that the lane
computes from the two small tables, and the signed-digit walk over it — compiled here with g++ -DF29_CHECK (every lazy bound a
recorded failure) and compared with Python integers: the scalar against c·τ′^i mod r, the scaled point of j·G against
(s·j mod r)·G from the oracle, in the file's own bytes (affine, Montgomery form, the identity all zero).  Every case is
CONSTRUCTED.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
import groth16_dlog_model as M
import ptau_contribute_model as CM
import ptau_prepare_model as PM
import zkey_contribute_model as ZM

Q, R = M.Q, M.R
MONT = 1 << 256
OMEGA3 = PM.omega(3)                                                        # the powers cycle with period 8
TAUS = ZM.EDGE_SCALARS + [OMEGA3]
CS = [1, R - 1, ZM.FULL]                                                    # section 2 and 3's c, −1, a full-width α′ or β′
POWERS = [0, 1, 3, 7, 28]


def _indices(power):
    """0, 1, both sides of the table boundary, the last index of section 2 — those that exist"""
    k, last = CM.table_bits(power), (2 << power) - 2
    return sorted({i for i in (0, 1, (1 << k) - 1, 1 << k, (1 << k) + 1, last) if i <= last})


@pytest.fixture(scope="module")
def chk():
    out = os.path.join(ROOT, "build", "ptau_contribute29_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "ptau_contribute29_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-DF29_CHECK", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc"), "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.pc29_last_failure.restype = C.c_char_p
    lib.pc29_table_bits.restype = C.c_uint32
    lib.pc29_reset()
    yield lib
    assert lib.pc29_last_failure().decode() == "", "F29_CHECK bound fired"


def _words(v, n=32):
    return int(v).to_bytes(n, "little")


class Tables:
    """lo and hi of (τ′, c, power) from the checked build"""

    def __init__(self, chk, tau, c, power):
        self.chk, self.k = chk, chk.pc29_table_bits(power)
        assert self.k == CM.table_bits(power)
        n_lo, n_hi = 1 << self.k, 1 << (power + 1 - self.k)
        self.lo, self.hi = C.create_string_buffer(32 * n_lo), C.create_string_buffer(32 * n_hi)
        chk.pc29_tables(C.c_char_p(_words(tau)), C.c_char_p(_words(c)), C.c_uint32(self.k), C.c_uint32(n_hi), self.lo, self.hi)

    def scalar(self, i):
        out = C.create_string_buffer(32)
        self.chk.pc29_scalar(self.lo, self.hi, C.c_uint32(self.k), C.c_uint64(i), out)
        return int.from_bytes(out.raw, "little")


def test_the_cases_are_what_they_claim():
    """conditions on the inputs, not measurements"""
    assert all(0 < t < R for t in TAUS) and len(set(TAUS)) == len(TAUS) and 1 in TAUS and R - 1 in TAUS
    assert pow(OMEGA3, 8, R) == 1 and pow(OMEGA3, 4, R) == R - 1
    assert [CM.table_bits(p) for p in POWERS] == [1, 1, 2, 4, 15]
    assert _indices(0) == [0] and _indices(1) == [0, 1, 2] and _indices(3) == [0, 1, 3, 4, 5, 14]
    assert _indices(7) == [0, 1, 15, 16, 17, 254] and _indices(28)[-1] == (1 << 29) - 2
    # every index of a section has its two entries: i ≫ k below the hi table's 2^(power+1−k), i mod 2^k below lo's 2^k
    for p in POWERS:
        k = CM.table_bits(p)
        assert 0 <= p + 1 - k and ((2 << p) - 2) >> k < 1 << (p + 1 - k)


@pytest.mark.parametrize("power", [0, 1, 3, 7])
def test_the_lanes_scalar_is_c_times_the_power(chk, power):
    for tau in TAUS:
        for c in CS:
            t = Tables(chk, tau, c, power)
            for i in _indices(power):
                assert t.scalar(i) == c * pow(tau, i, R) % R, (power, hex(tau), hex(c), i)
    assert chk.pc29_last_failure().decode() == ""


def test_the_lanes_scalar_at_the_largest_power(chk):
    """power 28: tables of 2^15 and 2^14 entries for 2^29 − 1 indices"""
    for tau, c in ((ZM.FULL, R - 1), (OMEGA3, 1), (R - 2, ZM.FULL)):
        t = Tables(chk, tau, c, 28)
        for i in _indices(28):
            assert t.scalar(i) == c * pow(tau, i, R) % R, (hex(tau), hex(c), i)


class Lane:
    def __init__(self, chk, O):
        self.chk, self.pts = chk, M.Points(O)

    def file_point(self, group, k):
        k %= R
        p = self.pts.memo[group].get(k) if k else (0,) * (2 if group == "g1" else 4)
        return b"".join(_words(c * MONT % Q) for c in p)

    def check(self, group, power, cases):
        """cases: (j, τ′, c, i): the lane of element i holding j·G"""
        self.pts.need(group, [x for j, tau, c, i in cases for x in (j, j * c * pow(tau, i, R))])
        self.pts.resolve()
        size = 64 if group == "g1" else 128
        f = self.chk.pc29_lane_g1 if group == "g1" else self.chk.pc29_lane_g2
        tables = {}
        for j, tau, c, i in cases:
            t = tables.setdefault((tau, c), Tables(self.chk, tau, c, power))
            out = C.create_string_buffer(size)
            f(C.c_char_p(self.file_point(group, j)), t.lo, t.hi, C.c_uint32(t.k), C.c_uint64(i), out)
            what = (group, j, hex(tau), hex(c), i)
            assert self.chk.pc29_last_failure().decode() == "", what
            assert out.raw == self.file_point(group, j * c * pow(tau, i, R)), what


@pytest.fixture(scope="module")
def lane(chk, O):
    return Lane(chk, O)


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_the_scaled_point_is_the_oracles_multiple(lane, group):
    """power 3 (k = 2): every boundary index, every edge τ′; s = 1 at i = 0 with c = 1, s = r − 1, s of the longest form"""
    cases = [(j, tau, c, i) for j in (1, 12345) for tau in TAUS for c in (1, R - 1) for i in _indices(3)]
    assert any(c * pow(tau, i, R) % R == 1 for _, tau, c, i in cases) and any(c * pow(tau, i, R) % R == R - 1 for _, tau, c, i in cases)
    assert any(len(ZM.naf(c * pow(tau, i, R) % R)) == 255 for _, tau, c, i in cases)
    lane.check(group, 3, cases)
    # the identity in: the identity out, all zero
    lane.check(group, 3, [(0, ZM.FULL, R - 1, 5), (0, 1, 1, 0)])
    # c·τ′^i = r − 1 gives −P: the same x, the other y
    lane.pts.need(group, [5, R - 5])
    lane.pts.resolve()
    half = 32 if group == "g1" else 64
    p, n = lane.file_point(group, 5), lane.file_point(group, R - 5)
    assert p[:half] == n[:half] and p[half:] != n[half:]
    lane.check(group, 3, [(5, R - 1, 1, 1)])
