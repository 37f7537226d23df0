"""Checked host build of csrc/prover/zkey_setup29.h — the scalars groth16_setup's kernels compute one lane per Lagrange value, per
(matrix, wire) column and per wire — compiled here with g++ -DF29_CHECK and compared with Python integers: synth.lagrange_at and
synth.key_scalars are the definition.  Every input below is CONSTRUCTED.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
import zkey_new_circuits as ZC

R = ZC.R
CLASSES = ZC.CLASSES
BINDING = 0xffffffff
PIECES = [0, 8, 64]                     # one walk; items of 8 and of 64 terms, as heavy_column_terms cuts them


@pytest.fixture(scope="module")
def chk():
    out = os.path.join(ROOT, "build", "zkey_setup29_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "zkey_setup29_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-DF29_CHECK", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc"), "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.zs29_last_failure.restype = C.c_char_p
    lib.zs29_reset()
    yield lib
    assert lib.zs29_last_failure().decode() == "", "F29_CHECK bound fired"


def _words(v):
    return int(v).to_bytes(32, "little")


def _toxic(t):
    return C.c_char_p(b"".join(_words(x) for x in t))


def _int(buf):
    return int.from_bytes(bytes(buf), "little")


def _fe():
    return (C.c_uint8 * 32)()


def test_roots_are_the_synthesisers(chk, S):
    for p in (0, 1, 3, 10, 27, 28):
        out = _fe()
        chk.zs29_root(p, out)
        assert _int(out) == S.omega(p), p


@pytest.mark.parametrize("logn", [1, 3, 9])
def test_lagrange_lanes(chk, S, logn):
    n = 1 << logn
    T = S.toxic_waste()
    tau, delta = T[0], T[4]
    assert chk.zs29_toxic_check(_toxic(T), logn, None) == 0
    g = S.omega(logn + 1)
    L = S.lagrange_at(n, logn, tau)
    Lc = S.lagrange_at(n, logn, tau * pow(g, -1, R) % R)
    zt = (pow(tau, n, R) - 1) * pow((-2 * delta) % R, -1, R) % R
    for j in sorted({0, 1, n - 1}):
        out = _fe()
        chk.zs29_lagrange(_toxic(T), logn, 0, j, out)
        assert _int(out) == L[j], (logn, j)
        chk.zs29_lagrange(_toxic(T), logn, 1, j, out)
        assert _int(out) == Lc[j] * zt % R, (logn, j)                # section 9's scalar: key_scalars' h
    assert chk.zs29_last_failure().decode() == ""


def _column(chk, terms, L, piece, binding=()):
    """terms: (row, v); binding: the positions whose entry is a public-binding row (v must be 1)"""
    ents, vals = [], []
    for i, (row, v) in enumerate(terms):
        if i in binding:
            assert v == 1
            ents += [row, BINDING]
        else:
            ents += [row, len(vals)]
            vals.append(v)
    out = _fe()
    chk.zs29_column((C.c_uint32 * max(1, len(ents)))(*ents), len(terms), C.c_char_p(b"".join(_words(v) for v in vals) or b"\0"), len(vals),
                    C.c_char_p(b"".join(_words(x) for x in L)), piece, out)
    assert chk.zs29_last_failure().decode() == ""
    return _int(out)


def test_column_sums(chk, S):
    L = S.lagrange_at(512, 9, S.toxic_waste()[0])
    want = lambda terms: sum(v * L[row] for row, v in terms) % R
    cases = [
        [],                                                                              # a wire in no matrix
        [(5, c) for c in CLASSES[:1]],                                                   # one zero coefficient
        [(3 + i, c) for i, c in enumerate(CLASSES)],                                     # every class
        [(7, 0x1234567), (7, R - 0x1234567)],                                            # a cancelling column
        [(7, ZC.FULL), (9, 1), (7, R - ZC.FULL), (9, R - 1)],
        [(j, CLASSES[j % len(CLASSES)]) for j in range(300)],                            # cut at 8 and at 64, the last item short
        [(j % 512, CLASSES[(3 * j) % len(CLASSES)]) for j in range(64 * 9)],             # whole items
        [(j, 1) for j in range(65)],                                                     # one over the threshold
    ]
    assert want(cases[3]) == 0 and want(cases[4]) == 0
    for terms in cases:
        for piece in PIECES:
            assert _column(chk, terms, L, piece) == want(terms), (len(terms), piece)
    # public-binding rows among stored coefficients: coefficient 1, no stored value
    terms = [(300, 1), (4, 9), (301, 1)] + [(j, 2) for j in range(20)]
    for piece in PIECES:
        assert _column(chk, terms, L, piece, binding={0, 2}) == want(terms)


@pytest.mark.parametrize("name", ["mixed", "tiny", "chain7"])
@pytest.mark.parametrize("unit", [False, True])
def test_outputs_are_key_scalars(chk, S, name, unit):
    """from the circuit's columns to a, b, comb and the two quotients, against key_scalars"""
    r = ZC.circuits(S)[name]
    T = S.toxic_waste()
    if unit:
        T = T[:3] + (1, 1)
    ks = S.key_scalars(r, T)
    n, nc, npub, m = ks["n"], r.n_constraints, r.n_public, r.n_vars
    logn = n.bit_length() - 1
    L = S.lagrange_at(n, logn, T[0])
    cols = [[[] for _ in range(m)] for _ in range(3)]
    for k, mat in enumerate((r.A, r.B, r.C)):
        for (j, i, v) in mat:
            cols[k][i].append((j, v))
    h1, h2 = (C.c_uint8 * 96)(), (C.c_uint8 * 96)()
    chk.zs29_heads(_toxic(T), logn, h1, h2)
    heads = lambda b: [int.from_bytes(bytes(b)[32 * i:32 * i + 32], "little") for i in range(3)]
    assert heads(h1) == [T[1], T[2], T[4]] and heads(h2) == [T[2], T[3], T[4]]
    for s in range(m):
        bind = [(nc + s, 1)] if s <= npub else []
        a = _column(chk, cols[0][s] + bind, L, 8, binding={len(cols[0][s])} if bind else ())
        b = _column(chk, cols[1][s], L, 0)
        c = _column(chk, cols[2][s], L, 64)
        assert (a, b) == (ks["a"][s], ks["b"][s]), (name, s)
        comb, ic, cq = _fe(), _fe(), _fe()
        chk.zs29_outputs(_toxic(T), logn, C.c_char_p(_words(a)), C.c_char_p(_words(b)), C.c_char_p(_words(c)), comb, ic, cq)
        assert _int(comb) == (T[2] * a + T[1] * b + c) % R
        if s <= npub:
            assert _int(ic) == ks["ic"][s], (name, s)
        else:
            assert _int(cq) == ks["c"][s - npub - 1], (name, s)
    if name == "mixed":
        assert ks["a"][164] == 0 and ks["a"][165] == 0 and ks["a"][163] != 0     # the cancelling wire, the wire in no matrix
