"""Checked host build of csrc/prover/ptau_prepare29.h — the butterfly of groth16_ptau_prepare's inverse transform over curve
points — compiled here with g++ -DF29_CHECK (every lazy bound a recorded failure) and compared with Python integers in the
exponent: for P = a·G and Q = b·G the outputs must be ((a + w·b) mod r)·G and ((a − w·b) mod r)·G from the oracle, in the file's own
bytes (affine, Montgomery form, the identity all zero).  Every case is CONSTRUCTED.  Also here, host only: the reader of an
UNPREPARED .ptau (groth16_ptau_prepared_size) and its messages.  No GPU."""
import ctypes as C
import os
import struct
import subprocess

import pytest

from conftest import ROOT
import groth16_dlog_model as M
import ptau_prepare_model as PM
import zkey_contribute_model as ZM

Q, R = M.Q, M.R
MONT = 1 << 256
# real twiddles: ω₁⁻¹ = −1 is in EDGE_SCALARS as r − 1; a fourth root, an eighth root and a root of the largest domain
TWIDDLES = [pow(PM.omega(k), -j, R) for k, j in ((2, 1), (3, 3), (28, 12345))]
SCALARS = ZM.EDGE_SCALARS + TWIDDLES
A_B = [(5, 7), (12345, R - 2), (R - 1, 1)]


@pytest.fixture(scope="module")
def chk():
    out = os.path.join(ROOT, "build", "ptau_prepare29_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "ptau_prepare29_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-DF29_CHECK", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc"), "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.pp29_last_failure.restype = C.c_char_p
    lib.pp29_reset()
    yield lib
    assert lib.pp29_last_failure().decode() == "", "F29_CHECK bound fired"


def _words(v, n=32):
    return int(v).to_bytes(n, "little")


class Fly:
    def __init__(self, chk, O):
        self.chk, self.pts = chk, M.Points(O)

    def file_point(self, group, k):
        k %= R
        p = self.pts.memo[group].get(k) if k else (0,) * (2 if group == "g1" else 4)
        return b"".join(_words(c * MONT % Q) for c in p)

    def check(self, group, cases):
        """cases: (a, b, w) with w None for level 0"""
        eff = lambda w: 1 if w is None else w
        self.pts.need(group, [x for a, b, w in cases for x in (a, b, a + eff(w) * b, a - eff(w) * b)])
        self.pts.resolve()
        size = 64 if group == "g1" else 128
        f = self.chk.pp29_butterfly_g1 if group == "g1" else self.chk.pp29_butterfly_g2
        for a, b, w in cases:
            s, d = C.create_string_buffer(size), C.create_string_buffer(size)
            f(C.c_char_p(self.file_point(group, a)), C.c_char_p(self.file_point(group, b)), None if w is None else C.c_char_p(_words(w)), s, d)
            what = (group, a, b, None if w is None else hex(w))
            assert self.chk.pp29_last_failure().decode() == "", what
            assert s.raw == self.file_point(group, a + eff(w) * b), what
            assert d.raw == self.file_point(group, a - eff(w) * b), what


@pytest.fixture(scope="module")
def fly(chk, O):
    return Fly(chk, O)


def test_the_cases_are_what_they_claim():
    """conditions on the inputs, not measurements"""
    assert all(0 < w < R for w in SCALARS) and len(set(SCALARS)) == len(SCALARS)
    assert 1 in SCALARS and R - 1 in SCALARS and pow(TWIDDLES[0], 4, R) == 1 and pow(TWIDDLES[0], 2, R) == R - 1
    assert pow(TWIDDLES[1], 8, R) == 1 and pow(TWIDDLES[1], 4, R) != 1 and pow(TWIDDLES[2], 1 << 28, R) == 1
    assert all(a % R and b % R for a, b in A_B)


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_the_common_path(fly, group):
    fly.check(group, [(a, b, w) for a, b in A_B for w in SCALARS])
    fly.check(group, [(a, b, None) for a, b in A_B])                         # level 0: no multiplication


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_the_degenerate_cases_are_exact(fly, group):
    cases = []
    for w in SCALARS + [None]:
        e = 1 if w is None else w
        cases += [(5, 0, w),                                                 # Q the identity: both outputs are P
                  (0, 7, w),                                                 # P the identity: T and −T
                  (0, 0, w),                                                 # both
                  (e * 7 % R, 7, w),                                         # T = P: the sum doubles, the difference is the identity
                  (-e * 7 % R, 7, w)]                                        # T = −P: the sum is the identity, the difference doubles
    assert all((a - (1 if w is None else w) * b) % R == 0 for a, b, w in cases[3::5])
    assert all((a + (1 if w is None else w) * b) % R == 0 for a, b, w in cases[4::5])
    fly.check(group, cases)
    # the identity comes out as all-zero bytes, and P − T ≠ P + T otherwise
    size = 64 if group == "g1" else 128
    assert fly.file_point(group, 0) == bytes(size) and fly.file_point(group, 14) != fly.file_point(group, 0)


# ---- the unprepared file's reader ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(S, O):
    gen = {g: O.ec_to_affine(g, O.ec_generator(g)) for g in ("g1", "g2")}
    fbm = lambda g, sc: O.fixed_base_mul(g, gen[g], sc)
    to_mont = lambda a: O.fq_convert_montgomery(a, True)
    tau, alpha, beta = S.toxic_waste()[:3]
    return {p: PM.write_unprepared(p, tau, alpha, beta, fbm, to_mont) for p in (0, 3)}, S.write_ptau(3, fbm, points_to_mont=to_mont)


def test_prepared_size(K, files):
    raw, full = files
    for p, image in raw.items():
        assert K.ptau_prepared_size(image) == PM.prepared_size(p, len(image))
    assert K.ptau_prepared_size(raw[3]) == len(full)
    # the prepared-file reader still refuses the unprepared file with its own text, and reads the prepared one
    with pytest.raises(K.ProverError, match=r"\(-2\).*has not been prepared for phase 2"):
        K.ptau_info(raw[3])
    assert K.ptau_info(full).power == 3


def test_each_malformed_unprepared_file_has_its_own_message(K, files):
    raw, full = files
    image = raw[3]

    def refused(bad, code, text):
        with pytest.raises(K.ProverError, match=rf"\({code}\)") as e:
            K.ptau_prepared_size(bad)
        assert text in str(e.value), str(e.value)

    refused(full, -2, "section 12 is present: the file is already prepared for phase 2")
    refused(PM.without(full, {12, 13, 14}), -2, "section 15 is present: the file is already prepared")
    refused(image[:len(image) - 100], -2, "exceeds the file")
    refused(image[:20], -2, "truncated section table")
    refused(b"zkey" + image[4:], -2, "expected 'ptau'")
    refused(image[:4] + struct.pack("<I", 2) + image[8:], -2, "Version not supported")
    hdr = PM.sections(image)[0][1][0]
    e = bytearray(image)
    e[hdr + 4] ^= 2                                                          # q
    refused(bytes(e), -2, "not the BN254 base field's")
    e = bytearray(image)
    e[hdr:hdr + 4] = struct.pack("<I", 48)                                   # n8
    refused(bytes(e), -2, "unsupported base field size 48")
    e = bytearray(image)
    e[hdr + 36:hdr + 40] = struct.pack("<I", 29)                             # power
    refused(bytes(e), -2, "power 29 is above the field's two-adicity")
    for sid in (2, 3, 4, 5, 6, 7):
        refused(PM.without(image, {sid}), -2, "Missing section %d" % sid)
    refused(image[:8] + struct.pack("<I", 8) + image[12:] + struct.pack("<IQ", 7, 4) + bytes(4), -2, "Section Duplicated 7")
    # exactly the element counts of the layout: one short, one long
    want = {2: 15 * 64, 3: 8 * 128, 4: 8 * 64, 5: 8 * 64, 6: 128}
    for sid, size in want.items():
        assert PM.sections(image)[0][sid][1] == size
        body = PM.payload(image, sid)
        step = 128 if sid in (3, 6) else 64
        refused(PM.with_payload(image, sid, body[:-step]), -2, "section %d holds %d bytes, an unprepared file of power 3 has %d" % (sid, size - step, size))
        refused(PM.with_payload(image, sid, body + bytes(step)), -2, "section %d holds %d bytes, an unprepared file of power 3 has %d" % (sid, size + step, size))
    refused(b"ptau\1\0\0\0", -2, "expected 'ptau'")                          # shorter than a container's head
