"""Checked host build of csrc/prover/zkey_new29.h — the signed short form of a coefficient and the per-column sums that
groth16_zkey_new's kernels run one lane per (wire, output) — compiled here with g++ -DF29_CHECK (every lazy bound a recorded
failure) and compared with Python integers: the bases are k·G from the oracle, the expected sum is (Σ v_t·k_t mod r)·G from the
oracle, in the file's own bytes (affine, Montgomery form, the identity all zero).  Every column below is CONSTRUCTED.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
import groth16_dlog_model as M

Q, R_ORDER = M.Q, M.R
MONT = 1 << 256
FULL = 0x2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f80919 % R_ORDER
# the coefficient classes: zero, ±1, ±2, a short one, one word boundary crossed, both sides of the sign rule's boundary, full width
CLASSES = [0, 1, 2, R_ORDER - 1, R_ORDER - 2, (1 << 16) - 1, 1 << 127, (R_ORDER - 1) // 2, (R_ORDER + 1) // 2, FULL]
BINDING = 0xffffffff
PIECES = [0, 1, 2, 3, 5]


@pytest.fixture(scope="module")
def chk():
    out = os.path.join(ROOT, "build", "zkey_new29_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "zkey_new29_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-DF29_CHECK", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc"), "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.zn29_last_failure.restype = C.c_char_p
    lib.zn29_reset()
    yield lib
    assert lib.zn29_last_failure().decode() == "", "F29_CHECK bound fired"


def _words(v, n=32):
    return int(v).to_bytes(n, "little")


def test_signed_short_form(chk):
    assert FULL.bit_length() >= 253 and (R_ORDER - 1) // 2 < FULL          # full width, and on the negative side
    for v in CLASSES + [R_ORDER - FULL, 3, (1 << 32) - 1, 1 << 32, (1 << 64) + 1]:
        w, bits = (C.c_uint32 * 8)(), C.c_int()
        neg = chk.zn29_signed_short(C.c_char_p(_words(v)), w, C.byref(bits))
        mag = sum(int(x) << (32 * i) for i, x in enumerate(w))
        want_neg = v > (R_ORDER - 1) // 2                                   # whichever of v and r − v is smaller; r is odd: no tie
        want = R_ORDER - v if want_neg else v
        assert (neg, mag, bits.value) == (int(want_neg), want, want.bit_length()), hex(v)
        assert want <= (R_ORDER - 1) // 2
    # the boundary, by value: (r − 1)/2 stays, (r + 1)/2 is −(r − 1)/2
    w, bits = (C.c_uint32 * 8)(), C.c_int()
    assert chk.zn29_signed_short(C.c_char_p(_words((R_ORDER - 1) // 2)), w, C.byref(bits)) == 0
    assert chk.zn29_signed_short(C.c_char_p(_words((R_ORDER + 1) // 2)), w, C.byref(bits)) == 1 and bits.value == 253


class Columns:
    """runs columns of (k, v) terms — the base k·G, the coefficient v — through the checked build and the integer model"""

    def __init__(self, chk, O):
        self.chk, self.pts = chk, M.Points(O)

    def file_point(self, group, k):
        p = self.pts.memo[group].get(k % R_ORDER)
        if k % R_ORDER == 0:
            p = (0,) * (2 if group == "g1" else 4)
        return b"".join(_words(c * MONT % Q) for c in p)

    def run(self, group, lists, piece, binding=()):
        """lists: one or three lists of (k, v); binding: positions (list, index) whose entry is a public-binding row (v must be 1)"""
        size = 64 if group == "g1" else 128
        vals, bufs, ents, lens = [], [], [], []
        for li, terms in enumerate(lists):
            bufs.append(C.create_string_buffer(b"".join(self.file_point(group, k) for k, _ in terms) or b"\0", max(1, size * len(terms))))
            e = []
            for i, (_, v) in enumerate(terms):
                if (li, i) in binding:
                    assert v == 1
                    e += [i, BINDING]
                else:
                    e += [i, len(vals)]
                    vals.append(v)
            ents.append((C.c_uint32 * max(1, len(e)))(*e))
            lens.append(len(terms))
        nl = len(lists)
        base_p = (C.c_void_p * nl)(*[C.cast(b, C.c_void_p) for b in bufs])
        ent_p = (C.c_void_p * nl)(*[C.cast(e, C.c_void_p) for e in ents])
        out = C.create_string_buffer(size)
        f = self.chk.zn29_column_g1 if group == "g1" else self.chk.zn29_column_g2
        f(nl, base_p, ent_p, (C.c_uint32 * nl)(*lens), C.c_char_p(b"".join(_words(v) for v in vals) or b"\0"), len(vals), piece, out)
        assert self.chk.zn29_last_failure().decode() == "", (group, lists, piece)
        return out.raw

    def check(self, group, lists, binding=()):
        total = sum(k * v for terms in lists for k, v in terms) % R_ORDER
        self.pts.need(group, [k for terms in lists for k, _ in terms] + [total])
        self.pts.resolve()
        want = self.file_point(group, total)
        for piece in PIECES:
            assert self.run(group, lists, piece, binding) == want, (group, lists, piece)
        return total


@pytest.fixture(scope="module")
def cols(chk, O):
    return Columns(chk, O)


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_constructed_columns(cols, group):
    P, P2, P3 = 5, 11, 12345
    v = 0x1234567
    assert cols.check(group, [[]]) == 0                                              # empty
    cols.check(group, [[(P, 7)]])                                                    # one term
    cols.check(group, [[(P, 1)]])
    cols.check(group, [[(P, 1), (P, 1)]])                                            # the doubling branch from a fresh accumulator
    cols.check(group, [[(P2, 1), (P, 1), (P, 1)]])
    assert cols.check(group, [[(P, v), (P, R_ORDER - v)]]) == 0                      # cancelling to the identity
    assert cols.check(group, [[(P, 1), (P, R_ORDER - 1)]]) == 0
    cols.check(group, [[(P, 3), (P2, 0), (P3, 5)]])                                  # a zero coefficient between two others
    assert cols.check(group, [[(P, 0)]]) == 0
    for c in CLASSES:                                                                # every class alone, then all in one column
        cols.check(group, [[(P3, c)]])
    cols.check(group, [[(100 + i, c) for i, c in enumerate(CLASSES)]])
    cols.check(group, [[(P, 2), (P, R_ORDER - 2), (P2, 3), (P3, 1)]])                # the partial sum passes through the identity
    cols.check(group, [[(P, 1), (P2, FULL), (P, R_ORDER - 1), (P2, R_ORDER - FULL), (P3, 1), (P3, 1)]])
    cols.check(group, [[(P, 1), (P2, 9), (P3, 1)]], binding={(0, 0), (0, 2)})        # public-binding rows: coefficient 1, no value
    cols.check(group, [[(0, 5), (P, 2)]])                                            # an identity base contributes nothing


def test_three_lists_into_one_accumulator(cols):
    """comb_s: A's column against one base range, B's against another, C's against a third"""
    a = [(3, 1), (7, FULL), (9, 0)]
    b = [(21, 2), (22, R_ORDER - 1)]
    c = [(31, (1 << 16) - 1), (32, 1), (33, 1 << 127), (31, 1)]
    cols.check("g1", [a, b, c])
    cols.check("g1", [a, b, c], binding={(0, 0)})
    cols.check("g1", [[], b, c])
    cols.check("g1", [a, [], c])
    cols.check("g1", [a, b, []])
    cols.check("g1", [[], [], []])
    assert cols.check("g1", [[(3, 5)], [(3, R_ORDER - 2)], [(3, R_ORDER - 3)]]) == 0  # the three lists cancel each other
