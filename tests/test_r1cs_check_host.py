"""Checked host build of csrc/prover/r1cs_check.h — r1cs_eval / r1cs_holds, the per-constraint evaluation groth16_witness_check
runs on the GPU, one lane per constraint — compiled here with g++ -DR1CS_CHECK (a non-canonical operand of a field multiplication
is a recorded failure) and compared with Python integers.  Every case is CONSTRUCTED; the integer model decides what each must
give.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


@pytest.fixture(scope="module")
def chk():
    out = os.path.join(ROOT, "build", "r1cs_check_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "r1cs_check_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-DR1CS_CHECK", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc"), "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.r1cs_chk_last_failure.restype = C.c_char_p
    lib.r1cs_chk_reset()
    yield lib
    assert lib.r1cs_chk_last_failure().decode() == "", "a non-canonical operand reached a multiplication"


def _arr(xs):
    """32-byte little-endian elements, 16-byte aligned like `fe`"""
    raw = b"".join(int(x).to_bytes(32, "little") for x in xs) or b"\0" * 32
    buf = np.zeros(len(raw) // 8 + 2, dtype=np.uint64)
    off = (-buf.ctypes.data % 16) // 8
    view = buf[off:off + len(raw) // 8]
    view[:] = np.frombuffer(raw, dtype=np.uint64)
    return view


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def evaluate(chk, constraints, w):
    """constraints: [(A, B, C)] with each row a list of (wire, coefficient).  → [(holds, a, b, c)] from the header's text, after
    the model's own answer has been compared with it."""
    rowptr, wires, vals = [0], [], []
    for rows in constraints:
        for row in rows:
            wires += [i for i, _ in row]
            vals += [v for _, v in row]
            rowptr.append(len(wires))
    n = len(wires)
    d_rowptr = np.array(rowptr, dtype=np.uint32)
    d_wires = np.array(wires or [0], dtype=np.uint32)
    d_cols = np.zeros(max(n, 1), dtype=np.uint32)
    std, mont, wit, out = _arr(vals), _arr([0] * max(n, 1)), _arr(w), _arr([0, 0, 0])
    assert chk.r1cs_chk_fill(_ptr(d_wires), _ptr(std), n, len(w), _ptr(d_cols), _ptr(mont)) == 0
    got = []
    for j, rows in enumerate(constraints):
        holds = chk.r1cs_chk_constraint(_ptr(d_rowptr), _ptr(d_cols), _ptr(mont), _ptr(wit), j, _ptr(out))
        assert chk.r1cs_chk_last_failure().decode() == ""
        abc = tuple(int.from_bytes(out[4 * k:4 * k + 4].tobytes(), "little") for k in range(3))
        want = tuple(sum(v * w[i] for i, v in row) % R for row in rows)
        assert abc == want, (j, abc, want)
        assert holds == (1 if want[0] * want[1] % R == want[2] else 0), (j, holds, want)
        got.append((holds,) + abc)
    return got


def test_coefficient_and_witness_at_the_top_of_the_field(chk):
    for coef, val in ((R - 1, 5), (7, R - 1), (R - 1, R - 1)):
        w = [1, val, 3, coef * val % R * 3 % R]
        (holds, a, b, c), = evaluate(chk, [([(1, coef)], [(2, 1)], [(3, 1)])], w)
        assert holds == 1 and a == coef * val % R and b == 3
        # the same with the large coefficient on B and on C
        assert evaluate(chk, [([(2, 1)], [(1, coef)], [(3, 1)])], w)[0][0] == 1
        w2 = [1, val, 0, 0]
        w2[2] = coef * val % R
        assert evaluate(chk, [([(2, 1)], [(0, 1)], [(1, coef)])], w2)[0][0] == 1


def test_empty_rows(chk):
    w = [1, 5, 7, 35]
    full = ([(1, 1)], [(2, 1)], [(3, 1)])
    assert evaluate(chk, [full], w)[0][0] == 1
    # an empty A or B makes the left side 0; an empty C the right side
    assert evaluate(chk, [([], full[1], full[2])], w)[0] == (0, 0, 7, 35)
    assert evaluate(chk, [(full[0], [], full[2])], w)[0] == (0, 5, 0, 35)
    assert evaluate(chk, [(full[0], full[1], [])], w)[0] == (0, 5, 7, 0)
    assert evaluate(chk, [([], full[1], [])], w)[0] == (1, 0, 7, 0)
    assert evaluate(chk, [([], [], [])], w)[0] == (1, 0, 0, 0)
    # empty constraints between full ones: the rows behind them start where they should
    got = evaluate(chk, [full, ([], [], []), full, ([], [], full[2]), full], w)
    assert [g[0] for g in got] == [1, 1, 1, 0, 1]


def test_uneven_rows_advance_in_lockstep(chk):
    """a 40-term A beside one-term B and C, then each of the other two the long one"""
    w = [1] + [(i * 0x9E3779B97F4A7C15 + 11) % R for i in range(1, 48)]
    long = [(1 + k, (k * k + 3) % R) for k in range(40)]
    s = sum(v * w[i] for i, v in long) % R
    for pos in range(3):
        rows = [[(45, 1)], [(46, 1)], [(47, 1)]]
        rows[pos] = long
        ww = list(w)
        if pos == 0:
            ww[47] = s * ww[46] % R
        elif pos == 1:
            ww[47] = ww[45] * s % R
        else:
            ww[45], ww[46] = s, 1
        assert evaluate(chk, [tuple(rows)], ww)[0][0] == 1
        for wire in (1, 40):                                   # the first and the last wire only the long row reads
            bad = list(ww)
            bad[wire] = (bad[wire] + 1) % R
            assert evaluate(chk, [tuple(rows)], bad)[0][0] == 0


def test_a_wire_named_twice_sums(chk):
    w = [1, 6, 4, 0]
    w[3] = (2 * 6 + 5 * 6) * 4 % R
    (holds, a, b, c), = evaluate(chk, [([(1, 2), (1, 5)], [(2, 1)], [(3, 1)])], w)
    assert holds == 1 and a == 42
    # r − 1 and 1 on the same wire cancel
    assert evaluate(chk, [([(1, R - 1), (1, 1)], [(2, 1)], [])], w)[0] == (1, 0, 4, 0)


def test_product_reduces_modulo_r(chk):
    """a·b ≡ c only modulo r: a·b ≥ r as integers"""
    a, b = R - 2, R - 3
    assert a * b >= R
    w = [1, a, b, a * b % R]
    assert w[3] == 6
    assert evaluate(chk, [([(1, 1)], [(2, 1)], [(3, 1)])], w)[0] == (1, a, b, 6)
    a, b = 1 << 200, 1 << 100
    w = [1, a, b, (a * b) % R]
    assert evaluate(chk, [([(1, 1)], [(2, 1)], [(3, 1)])], w)[0][0] == 1
    w[3] = (a * b) % (1 << 254)         # the integer product cut instead of reduced
    assert w[3] < R and evaluate(chk, [([(1, 1)], [(2, 1)], [(3, 1)])], w)[0][0] == 0


def test_c_off_by_one(chk):
    for a, b in ((5, 7), (R - 1, R - 1), (0, 9), (R - 1, 1)):
        c = a * b % R
        for d, want in ((0, 1), (1, 0), (-1, 0)):
            w = [1, a, b, (c + d) % R]
            assert evaluate(chk, [([(1, 1)], [(2, 1)], [(3, 1)])], w)[0][0] == want, (a, b, d)


def test_fill_refuses_what_the_load_refuses(chk):
    cols, vals = np.zeros(1, dtype=np.uint32), _arr([0])
    for wire, value, want in ((3, 1, 0), (4, 1, -1), (0, R - 1, 0), (0, R, -2), (0, (1 << 256) - 1, -2), (4, R, -1)):
        assert chk.r1cs_chk_fill(_ptr(np.array([wire], dtype=np.uint32)), _ptr(_arr([value])), 1, 4, _ptr(cols), _ptr(vals)) == want
    for v, want in ((0, 1), (R - 1, 1), (R, 0), ((1 << 256) - 1, 0)):
        assert chk.r1cs_chk_value_in_range(_ptr(_arr([v]))) == want


def test_the_checked_build_sees_a_noncanonical_operand(chk):
    """the instrument itself: a witness value of r reaches a multiplication only here, and is recorded"""
    rowptr = np.array([0, 1, 1, 1], dtype=np.uint32)
    cols, vals, out = np.zeros(1, dtype=np.uint32), _arr([1]), _arr([0, 0, 0])
    chk.r1cs_chk_constraint(_ptr(rowptr), _ptr(cols), _ptr(vals), _ptr(_arr([R])), 0, _ptr(out))
    assert chk.r1cs_chk_last_failure().decode() == "witness value read by A"
    chk.r1cs_chk_reset()
