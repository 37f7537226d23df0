"""Checked host build of csrc/prover/point_pack29.h — the packed point form of groth16_ptau_pack / groth16_ptau_unpack: the sign
of a coordinate, a square root in Fq and in Fq2, both encodings and their inverse with its refusals — compiled here with
g++ -DF29_CHECK (every lazy bound a recorded failure) and compared with tests/point_pack_model.py's Python integers, byte for byte
in both directions.  Every case is CONSTRUCTED.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
import groth16_dlog_model as M
import point_pack_model as PK
import test_pairing29_combined as T   # the twist in Python integers: _tw_add, _tw_mul, _twist_points_outside
import zkey_contribute_model as ZM

Q, R = PK.Q, PK.R
SOUND, NONCANONICAL, OFF_CURVE, OFF_SUBGROUP = PK.SOUND, PK.NONCANONICAL, PK.OFF_CURVE, PK.OFF_SUBGROUP
FULL_Q = [0x2a4f1c3b5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f701 % Q, Q - 2, (1 << 253) + 12345]   # full-width residues


@pytest.fixture(scope="module")
def chk():
    out = os.path.join(ROOT, "build", "point_pack29_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "point_pack29_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-DF29_CHECK", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc"), "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.pk29_last_failure.restype = C.c_char_p
    lib.pk29_products.restype = C.c_ulong
    lib.pk29_reset()
    yield lib
    assert lib.pk29_last_failure().decode() == "", "F29_CHECK bound fired"


def _words(vs):
    return b"".join(int(v).to_bytes(32, "little") for v in vs)


def _call(chk, name, data, out_bytes):
    out = C.create_string_buffer(out_bytes)
    rc = getattr(chk, name)(C.c_char_p(data), out)
    assert chk.pk29_last_failure().decode() == "", (name, data.hex())
    return rc, out.raw


def in_subgroup(P):
    return T._tw_mul(R, P) is None


# ---- signs
def test_sign_in_fq_at_the_values_where_the_comparison_can_be_off_by_one(chk):
    for y, want in ((0, 0), (1, 0), ((Q - 1) // 2, 0), ((Q + 1) // 2, 1), (Q - 1, 1)):
        assert PK.sign_fq(y) == want
        assert chk.pk29_sign_g1(C.c_char_p(_words([PK.to_file(5), PK.to_file(y)]))) == want, hex(y)
    assert chk.pk29_last_failure().decode() == ""


def test_sign_in_fq2(chk):
    lo, hi = 7, Q - 7
    cases = [((lo, 0), 0), ((hi, 0), 1),                                     # c1 = 0: c0 decides
             ((hi, lo), 0), ((lo, hi), 1), ((0, lo), 0), ((0, hi), 1),       # c1 ≠ 0: c1 decides, whatever c0
             ((hi, (Q - 1) // 2), 0), ((lo, (Q + 1) // 2), 1)]
    for y, want in cases:
        assert PK.sign_fq2(y) == want
        assert chk.pk29_sign_g2(C.c_char_p(_words([PK.to_file(3), PK.to_file(4), PK.to_file(y[0]), PK.to_file(y[1])]))) == want, y
    assert chk.pk29_last_failure().decode() == ""


# ---- roots
def _sqrt_fq(chk, a):
    rc, out = _call(chk, "pk29_sqrt_fq", _words([PK.to_file(a)]), 32)
    return rc, PK.from_file(int.from_bytes(out, "little"))


def test_sqrt_fq(chk):
    squares = [z % Q * (z % Q) % Q for z in ZM.EDGE_SCALARS] + [0, 1] + [z * z % Q for z in FULL_Q]
    for a in squares:
        rc, root = _sqrt_fq(chk, a)
        assert rc == 1 and root * root % Q == a, hex(a)
        assert root in (PK.sqrt_fq(a), -PK.sqrt_fq(a) % Q)
    for a in (3, Q - 1):                                                     # non-residues
        assert pow(a, (Q - 1) // 2, Q) == Q - 1 and PK.sqrt_fq(a) is None
        assert _sqrt_fq(chk, a)[0] == 0, hex(a)


def _sqrt_fq2(chk, a):
    rc, out = _call(chk, "pk29_sqrt_fq2", _words([PK.to_file(a[0]), PK.to_file(a[1])]), 64)
    return rc, tuple(PK.from_file(int.from_bytes(out[i:i + 32], "little")) for i in (0, 32))


def test_sqrt_fq2(chk):
    c = 0x1234567890abcdef
    zs = [(c, 0), (0, c), (1, 1), (FULL_Q[0], FULL_Q[1]), (FULL_Q[2], FULL_Q[0]), (Q - 1, Q - 1), (Q - 1, 1)]
    squares = [PK.f2mul(z, z) for z in zs]
    residue, non_residue = 4, 3
    assert pow(residue, (Q - 1) // 2, Q) == 1 and pow(non_residue, (Q - 1) // 2, Q) == Q - 1
    squares += [(residue, 0), (c * c % Q, 0), (non_residue, 0), (Q - 1, 0), (0, 0)]   # a1 = 0: a real root, a purely imaginary one, 0
    for a in squares:
        rc, root = _sqrt_fq2(chk, a)
        assert rc == 1 and PK.f2mul(root, root) == a, a
        m = PK.sqrt_fq2(a)
        assert root in (m, (-m[0] % Q, -m[1] % Q))
    for a0 in (non_residue, Q - 1):
        rc, root = _sqrt_fq2(chk, (a0, 0))
        assert root[0] == 0 and root[1] != 0, "the root of a non-residue of Fq is purely imaginary"
    # constructed non-squares: a non-square times a square.  g = 1 + 2u has the non-residue norm 5… checked, not assumed
    non_squares = [g for g in ((1, 2), (2, 1), (9, 1), (1, 3), (3, 5)) if pow(g[0] * g[0] + g[1] * g[1], (Q - 1) // 2, Q) == Q - 1]
    assert len(non_squares) >= 2
    for g in non_squares:
        for z in zs[:4]:
            a = PK.f2mul(g, PK.f2mul(z, z))
            assert PK.sqrt_fq2(a) is None
            assert _sqrt_fq2(chk, a)[0] == 0, (g, z)


# ---- points
@pytest.fixture(scope="module")
def pts(O):
    p = M.Points(O)
    ks = [j for j in range(1, 17)] + [R - j for j in range(1, 17)] + [12345, T.X_BN]
    p.need("g1", ks)
    p.need("g2", ks)
    p.resolve()
    return p


def _file_g1(pts, k):
    return _words([PK.to_file(c) for c in pts.g1(k)])


def _file_g2(pts, k):
    return _words([PK.to_file(c) for c in pts.g2(k)])


def test_g1_round_trip(chk, pts):
    signs = set()
    for k in list(range(1, 17)) + [R - j for j in range(1, 17)]:
        point = _file_g1(pts, k)
        word = PK.pack_g1(point)
        signs.add(word[31] >> 7)
        assert _call(chk, "pk29_pack_g1", point, 32) == (0, word), k
        assert PK.unpack_g1(word) == (SOUND, point)
        assert _call(chk, "pk29_unpack_g1", word, 64) == (0, point), k
    assert signs == {0, 1}
    identity = bytes(31) + b"\x40"
    assert PK.pack_g1(bytes(64)) == identity
    assert _call(chk, "pk29_pack_g1", bytes(64), 32) == (0, identity)
    before = chk.pk29_products()
    assert _call(chk, "pk29_unpack_g1", identity, 64) == (0, bytes(64))
    assert chk.pk29_products() == before                                     # the identity is decided by comparisons alone


def _refused_g1(chk, word, want=None):
    kind, _ = PK.unpack_g1(word)
    if want is not None:
        assert kind == want, (word.hex(), kind, want)
    assert kind != SOUND
    before = chk.pk29_products()
    rc, out = _call(chk, "pk29_unpack_g1", word, 64)
    assert rc == kind and out == bytes(64), (word.hex(), rc, kind)           # nothing written
    return chk.pk29_products() - before


def test_g1_refusals(chk, pts):
    for x in (Q, Q + 1, (1 << 254) - 1):                                     # x >= q: no lazy operation sees it
        assert _refused_g1(chk, _words([x]), NONCANONICAL) == 0
        assert _refused_g1(chk, _words([x | PK.SIGN_BIT]), NONCANONICAL) == 0
    # x = q − 1, the largest canonical word: whatever the model says it is
    for sign in (0, PK.SIGN_BIT):
        word = _words([(Q - 1) | sign])
        kind, point = PK.unpack_g1(word)
        rc, out = _call(chk, "pk29_unpack_g1", word, 64)
        assert rc == kind and out == (point or bytes(64))
    # the identity flag with another bit set
    for extra in (1, 1 << 100, 1 << 253, PK.SIGN_BIT, PK.to_file(pts.g1(1)[0])):
        assert _refused_g1(chk, _words([PK.IDENTITY_BIT | extra]), NONCANONICAL) == 0
    # standard-form x in {0, 4, 10}: x³ + 3 is a non-residue.  An all-zero word without the flag is OFF_CURVE, not the identity
    for x in (0, 4, 10):
        assert pow(PK.g1_rhs(x), (Q - 1) // 2, Q) == Q - 1
        assert _refused_g1(chk, _words([PK.to_file(x)]), OFF_CURVE) > 0
    assert _refused_g1(chk, bytes(32), OFF_CURVE) > 0
    # and pack refuses what the lane test refuses
    bad = bytearray(_file_g1(pts, 3))
    bad[32] ^= 1
    assert _call(chk, "pk29_pack_g1", bytes(bad), 32) == (OFF_CURVE, bytes(32))
    assert _call(chk, "pk29_pack_g1", _words([Q, 0]), 32) == (NONCANONICAL, bytes(32))


def test_g2_round_trip(chk, pts):
    signs = set()
    for k in list(range(1, 17)) + [R - j for j in range(1, 17)] + [12345, T.X_BN]:
        point = _file_g2(pts, k)
        word = PK.pack_g2(point)
        signs.add(word[63] >> 7)
        assert _call(chk, "pk29_pack_g2", point, 64) == (0, word), k
        assert PK.unpack_g2(word, lambda P: True) == (SOUND, point)          # (the oracle's multiples are in the subgroup)
        assert _call(chk, "pk29_unpack_g2", word, 128) == (0, point), k
    assert signs == {0, 1}
    identity = bytes(63) + b"\x40"
    assert PK.pack_g2(bytes(128)) == identity
    assert _call(chk, "pk29_pack_g2", bytes(128), 64) == (0, identity)
    before = chk.pk29_products()
    assert _call(chk, "pk29_unpack_g2", identity, 128) == (0, bytes(128))
    assert chk.pk29_products() == before


def _refused_g2(chk, word, want):
    kind, _ = PK.unpack_g2(word, in_subgroup)
    assert kind == want, (word.hex(), kind, want)
    before = chk.pk29_products()
    rc, out = _call(chk, "pk29_unpack_g2", word, 128)
    assert rc == kind and out == bytes(128), (word.hex(), rc, kind)
    return chk.pk29_products() - before


def test_g2_refusals(chk, pts):
    gx = [PK.to_file(c) for c in pts.g2(1)[:2]]
    for bad in (Q, (1 << 256) - 1):                                          # c0 has no flag bits: all 256 are the residue
        assert _refused_g2(chk, _words([bad, gx[1]]), NONCANONICAL) == 0
    for bad in (Q, (1 << 254) - 1):
        assert _refused_g2(chk, _words([gx[0], bad]), NONCANONICAL) == 0
    for extra in ((1, 0), (0, 1), (0, PK.SIGN_BIT), (gx[0], 0)):             # the identity flag with another bit set
        assert _refused_g2(chk, _words([extra[0], PK.IDENTITY_BIT | extra[1]]), NONCANONICAL) == 0
    # twist x = (k, 0) for k in {0, 3, 4, 5}: no point on the twist
    for k in (0, 3, 4, 5):
        assert PK.sqrt_fq2(PK.g2_rhs((k, 0))) is None
        assert _refused_g2(chk, _words([PK.to_file(k), 0]), OFF_CURVE) > 0
    # on the twist, outside the subgroup: never a point
    x0 = M.twist_point_outside_subgroup()
    outside = [((x0[0], x0[1]), (x0[2], x0[3]))] + T._twist_points_outside(4)
    g2 = lambda k: ((pts.g2(k)[0], pts.g2(k)[1]), (pts.g2(k)[2], pts.g2(k)[3]))
    mixed = [T._tw_add(P, g2(k)) for P, k in zip(outside[1:], (1, 2, 3, 12345))]
    mixed.append(T._tw_add(T._tw_mul(R, outside[1]), g2(T.X_BN)))            # a pure-cofactor point plus a subgroup point
    for P in outside + mixed:
        for Pn in (P, (P[0], (-P[1][0] % Q, -P[1][1] % Q))):                 # both signs
            assert not in_subgroup(Pn)
            word = PK.pack_g2(_words([PK.to_file(c) for c in Pn[0] + Pn[1]]))
            assert _refused_g2(chk, word, OFF_SUBGROUP) > 0
    bad = bytearray(_file_g2(pts, 3))
    bad[64] ^= 1
    assert _call(chk, "pk29_pack_g2", bytes(bad), 64) == (OFF_CURVE, bytes(64))
