"""Checked host build of csrc/prover/ptau_truncate29.h — one lane of groth16_ptau_truncate's fix-up: the scalar ω′^j/2n′ that the lane
computes from the two small tables, its 51 signed digits of width 5, the table of Q's signed-window multiples, the walk over it and
B − T — compiled here with g++ -DF29_CHECK (every lazy bound a recorded failure) and compared with Python integers: the scalar
against ω′^j/2n′ mod r, the digits against their sum, points against (k mod r)·G from the oracle in the file's own bytes (affine,
Montgomery form, the identity all zero).  Every case is CONSTRUCTED.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
import ptau_contribute_model as CM
import ptau_prepare_model as PM
import ptau_truncate_model as TM

R = PM.R
WIDTH, WINDOWS, ROW = 5, 51, 16
OMEGA8 = PM.omega(3)
# 1, −1, the two halves, the cube root of one, a root of order 8, every window all ones (2^253 − 1 < r < 2^254), every window 16 (no
# carry anywhere) and every window 17 (a carry everywhere)
SCALARS = [1, 2, R - 1, (R - 1) // 2, (R + 1) // 2, TM.CUBE_ROOT, OMEGA8, (1 << 253) - 1,
           sum(16 << (5 * w) for w in range(50)), sum(17 << (5 * w) for w in range(50))]
# a partial sum that MEETS a row: with s = 24·2^250 − r the windows below 50 sum to 12·2^250 − r ≡ 12·2^250, the row the top digit 12
# then adds — x_madd's doubling branch; s = r (never a lane's scalar: the walk alone) sums to −12·2^250 below the top digit 12 — its
# cancelling branch, and the identity
MEETS_ROW, CANCELS = (24 << 250) - R, R
POWERS = [0, 1, 3, 7, 26]


@pytest.fixture(scope="module")
def chk():
    out = os.path.join(ROOT, "build", "ptau_truncate29_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "ptau_truncate29_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-DF29_CHECK", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc"), "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.pt29_last_failure.restype = C.c_char_p
    lib.pt29_table_bits.restype = C.c_uint32
    lib.pt29_digits.restype = C.c_uint32
    lib.pt29_reset()
    yield lib
    assert lib.pt29_last_failure().decode() == "", "F29_CHECK bound fired"


def _words(v, n=32):
    return int(v).to_bytes(n, "little")


def _digits(chk, s):
    out = (C.c_int32 * WINDOWS)()
    carry = chk.pt29_digits(C.c_char_p(_words(s)), out)
    return list(out), carry


def test_the_cases_are_what_they_claim(chk):
    """conditions on the inputs and on the geometry, not measurements"""
    geo = (C.c_int32 * 5)()
    chk.pt29_geometry(geo)
    assert list(geo) == [WIDTH, WINDOWS, ROW, WINDOWS * ROW, WINDOWS * ROW * 64] and WINDOWS * WIDTH == 255 and R < 1 << 254
    assert 3 * geo[4] <= 160 * 1024 < 2 * (43 * 32 * 64)                  # three workgroups' tables a CU at width 5; not two at width 6
    assert all(0 < s < R for s in SCALARS) and len(set(SCALARS)) == len(SCALARS)
    assert (1 + TM.CUBE_ROOT + TM.CUBE_ROOT ** 2) % R == 0 and pow(OMEGA8, 4, R) == R - 1
    assert 0 < MEETS_ROW < R and MEETS_ROW >> 250 == 11 and (MEETS_ROW % (1 << 250)) - (1 << 250) == (12 << 250) - R
    assert [CM.table_bits(p) for p in POWERS] == [1, 1, 2, 4, 14]


def _indices(p):
    k, last = CM.table_bits(p), (2 << p) - 1
    return sorted({j for j in (0, 1, (1 << k) - 1, 1 << k, (1 << k) + 1, last) if j <= last})


@pytest.mark.parametrize("p", POWERS)
def test_the_lanes_scalar_is_the_root_to_the_j_over_2n(chk, p):
    k, w, ninv = chk.pt29_table_bits(p), PM.omega(p + 1), pow(2 << p, -1, R)
    assert k == CM.table_bits(p) and pow(w, 2 << p, R) == 1 and (p == 0 or pow(w, 1 << p, R) == R - 1)
    n_lo, n_hi = 1 << k, 1 << (p + 1 - k)
    assert ((2 << p) - 1) >> k < n_hi                                        # every lane has its two entries
    lo, hi = C.create_string_buffer(32 * n_lo), C.create_string_buffer(32 * n_hi)
    chk.pt29_tables(C.c_char_p(_words(w)), C.c_char_p(_words(ninv)), C.c_uint32(k), C.c_uint32(n_hi), lo, hi)
    for j in _indices(p):
        out = C.create_string_buffer(32)
        chk.pt29_scalar(lo, hi, C.c_uint32(k), C.c_uint64(j), out)
        s = int.from_bytes(out.raw, "little")
        assert s == pow(w, j, R) * ninv % R, (p, j)
        # the scalar of input 2n′ − 1 in the inverse transform's row j
        assert s == pow(w, -j * ((2 << p) - 1), R) * ninv % R
    assert chk.pt29_last_failure().decode() == ""


def test_the_digits_sum_back(chk):
    for s in SCALARS + [MEETS_ROW, CANCELS, (1 << 254) - 1, 0]:
        d, carry = _digits(chk, s)
        assert carry == 0 and all(-15 <= x <= 16 for x in d), hex(s)
        assert sum(x << (5 * w) for w, x in enumerate(d)) == s, hex(s)
    assert _digits(chk, SCALARS[-1])[0][:3] == [-15, -14, -14] and set(_digits(chk, SCALARS[-2])[0][:50]) == {16}
    assert _digits(chk, (1 << 253) - 1)[0] == [-1] + [0] * 49 + [8]


class Q:
    """Q = k·G: its table from the checked build"""

    def __init__(self, chk, pb, k):
        self.chk, self.pb, self.k = chk, pb, k
        self.table = C.create_string_buffer(64 * WINDOWS * ROW)
        chk.pt29_fill_table(C.c_char_p(pb.g1(k)), self.table)

    def entry(self, i):
        out = C.create_string_buffer(64)
        self.chk.pt29_entry(self.table, C.c_uint32(i), out)
        return out.raw

    def walk(self, s):
        out = C.create_string_buffer(64)
        self.chk.pt29_walk(C.c_char_p(_words(s)), self.table, out)
        return out.raw


@pytest.fixture(scope="module")
def world(chk, O):
    pb = CM.PointBytes(O)
    return pb, {k: Q(chk, pb, k) for k in (1, 12345)}


def test_the_table_holds_the_signed_window_multiples(chk, world):
    pb, qs = world
    for k, q in qs.items():
        cases = [(w, d) for w in (0, 1, 25, 50) for d in (1, 2, 3, 16)]
        pb.prefetch(g1=[d * 32 ** w * k for w, d in cases])
        for w, d in cases:
            assert q.entry(ROW * w + d - 1) == pb.g1(d * 32 ** w * k), (k, w, d)
    assert chk.pt29_last_failure().decode() == ""


def test_the_walk_is_the_oracles_multiple(chk, world):
    pb, qs = world
    for k, q in qs.items():
        pb.prefetch(g1=[s * k for s in SCALARS + [MEETS_ROW]])
        for s in SCALARS + [MEETS_ROW]:
            assert q.walk(s) == pb.g1(s * k), (k, hex(s))
        assert q.walk(CANCELS) == bytes(64) and q.walk(0) == bytes(64)
    assert chk.pt29_last_failure().decode() == ""


def test_the_lane_subtracts(chk, world):
    """B − s·Q with s from two table entries (hi = c, lo = t: s = c·t): B general, the identity, T itself (the identity out, all
    zero), −T (the doubling branch)"""
    pb, qs = world
    mont = lambda v: _words(v * (1 << 256) % R)
    for k, q in qs.items():
        for c, t in ((1, 1), (pow(4, -1, R), OMEGA8), (R - 1, TM.CUBE_ROOT), (SCALARS[-1], 1)):
            s = c * t % R
            bs = [777, 0, s * k, -s * k]
            pb.prefetch(g1=bs + [b - s * k for b in bs])
            for b in bs:
                out = C.create_string_buffer(64)
                chk.pt29_lane(C.c_char_p(pb.g1(b)), C.c_char_p(mont(c)), C.c_char_p(mont(t)), q.table, out)
                assert out.raw == pb.g1(b - s * k), (k, hex(s), b)
            assert pb.g1(s * k - s * k) == bytes(64)
    assert chk.pt29_last_failure().decode() == ""
