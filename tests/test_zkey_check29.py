"""Checked host build of csrc/prover/zkey_check29.h — classify_g1 / classify_g2, the per-point tests groth16_zkey_check runs on
the GPU — compiled here with g++ -DF29_CHECK (every lazy bound a recorded failure) and compared with Python integer arithmetic on
the file's Montgomery form.  Every faulty input below is CONSTRUCTED (a named edit of a sound point, or a point built to lie where
it lies), none is random; the integer model decides what each must classify as, and the cases whose class is known by
construction assert that class as well.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import groth16_dlog_model as M
import test_pairing29_combined as T   # the twist in Python integers: _tw_add, _tw_mul, _twist_points_outside

Q, R_ORDER = M.Q, M.R
MONT = 1 << 256
MONT_INV = pow(MONT, -1, Q)
SOUND, NONCANONICAL, OFF_CURVE, OFF_SUBGROUP = 0, 1, 2, 3
D82 = pow(82, -1, Q)
B_TWIST = M._f2mul((3, 0), (9 * D82 % Q, -D82 % Q))  # 3/ξ


@pytest.fixture(scope="module")
def chk():
    out = os.path.join(ROOT, "build", "zkey_check29_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "zkey_check29_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-DF29_CHECK", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc"), "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.zk29_last_failure.restype = C.c_char_p
    lib.zk29_products.restype = C.c_ulong
    lib.zk29_reset()
    yield lib
    assert lib.zk29_last_failure().decode() == "", "F29_CHECK bound fired"


def to_file(x):
    """standard-form coordinate → the 256-bit residue the .zkey holds"""
    return x * MONT % Q


def model_g1(v):
    """the class of the raw words (vx, vy), by integers"""
    if any(c >= Q for c in v):
        return NONCANONICAL
    if not any(v):
        return SOUND
    x, y = (c * MONT_INV % Q for c in v)
    return SOUND if y * y % Q == (x * x * x + 3) % Q else OFF_CURVE


def model_g2(v):
    if any(c >= Q for c in v):
        return NONCANONICAL
    if not any(v):
        return SOUND
    x0, x1, y0, y1 = (c * MONT_INV % Q for c in v)
    x, y = (x0, x1), (y0, y1)
    rhs = M._f2mul(M._f2mul(x, x), x)
    if M._f2mul(y, y) != ((rhs[0] + B_TWIST[0]) % Q, (rhs[1] + B_TWIST[1]) % Q):
        return OFF_CURVE
    return SOUND if T._tw_mul(R_ORDER, (x, y)) is None else OFF_SUBGROUP


def classify(chk, group, v):
    """→ (class, lazy products run)"""
    buf = np.frombuffer(b"".join(int(c).to_bytes(32, "little") for c in v), dtype=np.uint64).copy()
    before = chk.zk29_products()
    kind = (chk.zk29_classify_g1 if group == "g1" else chk.zk29_classify_g2)(buf.ctypes.data_as(C.c_void_p))
    assert chk.zk29_last_failure().decode() == "", (group, v)
    return kind, chk.zk29_products() - before


def agrees(chk, group, v, want=None):
    model = (model_g1 if group == "g1" else model_g2)(v)
    if want is not None:
        assert model == want, (group, v, model, want)
    kind, products = classify(chk, group, v)
    assert kind == model, (group, [hex(c) for c in v], kind, model)
    return products


KS = [1, 2, 3, R_ORDER - 1, 12345, T.X_BN, 0x1234567890abcdef1234567890abcdef]


@pytest.fixture(scope="module")
def sound(O):
    """oracle-made subgroup points in file form: {'g1': [(vx, vy)…], 'g2': [(vx0, vx1, vy0, vy1)…]}"""
    pts = M.Points(O)
    pts.need("g1", KS)
    pts.need("g2", KS)
    pts.resolve()
    return {"g1": [tuple(to_file(c) for c in pts.g1(k)) for k in KS], "g2": [tuple(to_file(c) for c in pts.g2(k)) for k in KS]}


def test_sound_points_and_the_identity(chk, sound):
    for g, w in (("g1", 2), ("g2", 4)):
        for v in sound[g]:
            assert agrees(chk, g, v, SOUND) > 0
        assert agrees(chk, g, (0,) * w, SOUND) == 0          # the identity is decided by comparisons alone


def test_constructed_edits_of_a_sound_point(chk, sound):
    for g, w in (("g1", 2), ("g2", 4)):
        for v in sound[g][:3]:
            for pos in range(w):                              # constructed: one coordinate changed by one, up and down
                for d in (1, -1):
                    e = list(v)
                    e[pos] = (e[pos] + d) % Q
                    agrees(chk, g, e, OFF_CURVE)
            neg = list(v)                                     # constructed: (x, −y), on the curve and in the group again
            for pos in range(w // 2, w):
                neg[pos] = (Q - neg[pos]) % Q
            agrees(chk, g, neg, SOUND)
            zero_x = [0] * (w // 2) + list(v[w // 2:])        # constructed: x = 0 with the point's own y ≠ 0
            agrees(chk, g, zero_x)
        agrees(chk, g, [0] * (w // 2) + [to_file(1)] + [0] * (w // 2 - 1), OFF_CURVE)  # constructed: x = 0, y = 1: 1 ≠ b


def test_coordinates_around_q_in_each_position(chk, sound):
    for g, w in (("g1", 2), ("g2", 4)):
        v = sound[g][0]
        for pos in range(w):
            e = list(v)
            e[pos] = Q - 1                                    # constructed: the largest canonical residue
            assert agrees(chk, g, e) > 0
            for bad in (Q, Q + 1, (1 << 256) - 1):            # constructed: not residues at all
                e[pos] = bad
                assert agrees(chk, g, e, NONCANONICAL) == 0, "a lazy operation ran on a non-canonical coordinate"
        # non-canonical wins over everything else in the same point: an off-curve partner, an all-zero partner
        e = [Q] + [0] * (w - 1)
        assert agrees(chk, g, e, NONCANONICAL) == 0
        e = list(v)
        e[0], e[w - 1] = (e[0] + 1) % Q, Q
        assert agrees(chk, g, e, NONCANONICAL) == 0


def test_twist_points_outside_the_subgroup(chk, O, sound):
    outside = T._twist_points_outside(20)                     # constructed: x = 1, 2, … with a square right side
    std = lambda P: (P[0][0], P[0][1], P[1][0], P[1][1])
    file_form = lambda P: tuple(to_file(c) for c in std(P))
    for P in outside:
        agrees(chk, "g2", file_form(P), OFF_SUBGROUP)
    pts = M.Points(O)
    pts.need("g2", KS)
    pts.resolve()
    g2 = lambda k: ((pts.g2(k)[0], pts.g2(k)[1]), (pts.g2(k)[2], pts.g2(k)[3]))
    for i, P in enumerate(outside[:5]):
        rP = T._tw_mul(R_ORDER, P)                            # constructed: a pure-cofactor point
        agrees(chk, "g2", file_form(rP), OFF_SUBGROUP)
        k = KS[i % len(KS)]
        agrees(chk, "g2", file_form(T._tw_add(P, g2(k))), OFF_SUBGROUP)   # constructed: mixed sums T + k·G₂, r·T + k·G₂
        agrees(chk, "g2", file_form(T._tw_add(rP, g2(k))), OFF_SUBGROUP)
