"""Checked host build of csrc/prover/zkey_contribute29.h — the non-adjacent form of the scalar every lane of
groth16_zkey_contribute's kernel shares, and the walk over it — compiled here with g++ -DF29_CHECK (every lazy bound a recorded
failure) and compared with Python integers: the digits against the textbook's NAF, k·(j·G) against (k·j mod r)·G from the oracle,
in the file's own bytes (affine, Montgomery form, the identity all zero).  Every scalar below is CONSTRUCTED.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
import groth16_dlog_model as M
import zkey_contribute_model as ZM

Q, R_ORDER = M.Q, M.R
MONT = 1 << 256
# 1 and 2: the first addition copies P, nothing else adds; 3: one digit −1 under the top; r − 1: the result is −P; r − 2: the
# accumulator is −P when the last digit −1 arrives (x_madd's doubling branch); both sides of r/2; one bit in the middle of a word,
# a word of ones, a word boundary; 3·2^252: the form's length is 255, the longest there is below r; a full-width value
SCALARS = ZM.EDGE_SCALARS
BASES = [1, 5, 12345, R_ORDER - 1]


@pytest.fixture(scope="module")
def chk():
    out = os.path.join(ROOT, "build", "zkey_contribute29_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "zkey_contribute29_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-DF29_CHECK", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc"), "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.zc29_last_failure.restype = C.c_char_p
    lib.zc29_reset()
    yield lib
    assert lib.zc29_last_failure().decode() == "", "F29_CHECK bound fired"


def _words(v, n=32):
    return int(v).to_bytes(n, "little")


def _digits(chk, k):
    nz, ng = (C.c_uint32 * 8)(), (C.c_uint32 * 8)()
    ln = chk.zc29_recode(C.c_char_p(_words(k)), nz, ng)
    nzi, ngi = (sum(int(x) << (32 * i) for i, x in enumerate(m)) for m in (nz, ng))
    assert ngi & ~nzi == 0                                                  # a negative digit is a non-zero digit
    return ln, [(-1 if ngi >> i & 1 else 1) if nzi >> i & 1 else 0 for i in range(256)]


def test_the_scalars_are_what_the_cases_need():
    """conditions on the inputs, not measurements"""
    assert all(0 < k < R_ORDER for k in SCALARS) and len(set(SCALARS)) == len(SCALARS)
    assert 3 << 252 in SCALARS and len(ZM.naf(3 << 252)) == 255            # 2^254 − 2^252: the longest form below r
    assert max(len(ZM.naf(k)) for k in SCALARS) == 255
    assert ZM.FULL.bit_length() >= 253 and sum(1 for d in ZM.naf(ZM.FULL) if d) > 60
    assert ZM.naf(R_ORDER - 2)[0] == -1 and ZM.naf(3) == [-1, 0, 1]
    for k in SCALARS:                                                       # the model's NAF is one
        d = ZM.naf(k)
        assert sum(x << i for i, x in enumerate(d)) == k and all(not (a and b) for a, b in zip(d, d[1:])) and d[-1] == 1


@pytest.mark.parametrize("k", SCALARS + [0, 7, (1 << 253) - 1, 1 << 253], ids=hex)
def test_recode_is_the_non_adjacent_form(chk, k):
    ln, d = _digits(chk, k)
    want = ZM.naf(k)
    assert ln == len(want) and d[:ln] == want and not any(d[ln:])
    assert set(d) <= {-1, 0, 1} and all(not (a and b) for a, b in zip(d, d[1:]))
    assert sum(x << i for i, x in enumerate(d)) == k
    if k == 3 << 252:
        assert ln == 255


class Mul:
    def __init__(self, chk, O):
        self.chk, self.pts = chk, M.Points(O)

    def file_point(self, group, k):
        k %= R_ORDER
        p = self.pts.memo[group].get(k) if k else (0,) * (2 if group == "g1" else 4)
        return b"".join(_words(c * MONT % Q) for c in p)

    def check(self, group, cases):
        self.pts.need(group, [j for j, _ in cases] + [j * k for j, k in cases])
        self.pts.resolve()
        size = 64 if group == "g1" else 128
        f = self.chk.zc29_mul_g1 if group == "g1" else self.chk.zc29_mul_g2
        for j, k in cases:
            out = C.create_string_buffer(size)
            f(C.c_char_p(self.file_point(group, j)), C.c_char_p(_words(k)), out)
            assert self.chk.zc29_last_failure().decode() == "", (group, j, hex(k))
            assert out.raw == self.file_point(group, j * k), (group, j, hex(k))


@pytest.fixture(scope="module")
def mul(chk, O):
    return Mul(chk, O)


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_scale_is_the_oracles_multiple(mul, group):
    """G1: the kernel's walk; G2: the host path that scales the header's δ₂"""
    mul.check(group, [(j, k) for j in BASES for k in SCALARS])
    # k = r − 1 gives −P: the same x, the other y
    mul.pts.need(group, [5])
    mul.pts.resolve()
    half = 32 if group == "g1" else 64
    p, n = mul.file_point(group, 5), mul.file_point(group, 5 * (R_ORDER - 1))
    assert p[:half] == n[:half] and p[half:] != n[half:]
    # the identity in, and k = 0: the identity out
    mul.check(group, [(0, 7), (0, R_ORDER - 1), (5, 0)])
