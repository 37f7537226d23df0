"""The pure host pieces the key tools share (csrc/prover/device_call.h's neighbours: circuit_domain in prover_internal.h, words_zero /
same_point / pairing_eq in verify_host.h, PtauRanges::verdict in ptau_ranges.h), compiled here with g++ and linked with the product
library for its host pairing.  The points are k·G from the oracle and the expected answers come from the discrete-log model
(tests/groth16_dlog_model.py): e(a₁·G₁, a₂·G₂) = e(b₁·G₁, b₂·G₂) exactly when a₁·a₂ = b₁·b₂ mod r.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
import groth16_dlog_model as M

Q, R_ORDER = M.Q, M.R
NO_FAULT = (1 << 64) - 1


@pytest.fixture(scope="module")
def chk():
    out = os.path.join(ROOT, "build", "device_call_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    libdir = os.path.join(ROOT, "icicle-snark_amd", "lib")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc"), "-o", out,
                    os.path.join(ROOT, "tests", "device_call_check.cpp"), "-L" + libdir, "-licicle_snark_hip", "-Wl,-rpath," + libdir], check=True)
    lib = C.CDLL(out)
    lib.dc_circuit_domain.restype = C.c_uint64
    lib.dc_circuit_domain.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]
    return lib


def _words(v):
    return int(v).to_bytes(32, "little")


def _affine(coords):
    return b"".join(_words(c) for c in coords)


def test_circuit_domain(chk):
    def dom(total):
        k = C.c_uint32(99)
        n = chk.dc_circuit_domain(total - 1, 0, C.byref(k))              # n_constraints + n_public + 1 = total
        return n, k.value

    assert [dom(t) for t in (1, 2, 3, 4, 5)] == [(1, 0), (2, 1), (4, 2), (4, 2), (8, 3)]
    assert dom(1 << 28) == (1 << 28, 28) and dom((1 << 28) + 1) == (1 << 29, 29)
    # the sum is what counts, however it is split
    k = C.c_uint32()
    assert chk.dc_circuit_domain(153, 2, C.byref(k)) == 256 and k.value == 8
    assert chk.dc_circuit_domain(253, 2, C.byref(k)) == 256 and chk.dc_circuit_domain(253, 3, C.byref(k)) == 512 and k.value == 9


def test_words_zero(chk):
    assert chk.dc_words_zero(bytes(96), 96) == 1 and chk.dc_words_zero(b"", 0) == 1
    for at in (0, 31, 95):
        b = bytearray(96)
        b[at] = 1
        assert chk.dc_words_zero(bytes(b), 96) == 0
    assert chk.dc_words_zero(bytes(32) + b"\x01", 32) == 1                  # only the bytes asked about


def test_pairing_eq_against_the_dlog_model(chk, O):
    pts = M.Points(O)
    # (a₁, a₂, b₁, b₂): every identity / non-identity combination of the two left operands against identity and non-identity right
    # sides, then true and false equations on non-identity points
    cases = [(a1, a2, b1, b2) for a1 in (0, 3) for a2 in (0, 5) for (b1, b2) in ((0, 7), (7, 0), (0, 0), (15, 1), (2, 7))]
    cases += [(6, 35, 21, 10), (6, 35, 10, 21), (1, 1, 1, 1), (R_ORDER - 1, 2, 1, R_ORDER - 2), (6, 35, 21, 11), (1, 1, 1, 2), (R_ORDER - 1, 2, 1, 2)]
    pts.need("g1", [c[0] for c in cases] + [c[2] for c in cases])
    pts.need("g2", [c[1] for c in cases] + [c[3] for c in cases])
    pts.resolve()
    seen = set()
    for a1, a2, b1, b2 in cases:
        want = (a1 * a2 - b1 * b2) % R_ORDER == 0
        got = chk.dc_pairing_eq(_affine(pts.g1(a1)), _affine(pts.g2(a2)), _affine(pts.g1(b1)), _affine(pts.g2(b2)))
        assert got == int(want), (a1, a2, b1, b2)
        seen.add((a1 == 0, a2 == 0, want))
    # all four combinations of the left operands were asked about, each with both answers where both can occur
    assert {s[:2] for s in seen} == {(False, False), (False, True), (True, False), (True, True)}
    assert {(z1, z2) for z1, z2, w in seen if not w} == {(False, False), (False, True), (True, False), (True, True)}


def _scaled(coords, lam, width):
    """the homogeneous projective point (x·λ, y·λ, λ) of an affine one, λ in Fq; coordinates of `width` Fq words"""
    z = [lam] + [0] * (width - 1)
    return b"".join(_words(c * lam % Q) for c in coords) + b"".join(_words(c) for c in z)


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_same_point(chk, O, group):
    pts = M.Points(O)
    pts.need(group, [5, 6])
    pts.resolve()
    width = 1 if group == "g1" else 2
    f = chk.dc_same_point_g1 if group == "g1" else chk.dc_same_point_g2
    p5, p6 = pts.memo[group][5], pts.memo[group][6]
    assert f(_scaled(p5, 1, width), _scaled(p5, 0x1234567 * (1 << 200) % Q, width)) == 1   # two representations of one point
    assert f(_scaled(p5, 9, width), _scaled(p6, 9, width)) == 0
    identity, other_identity = bytes(96 * width), _scaled(p5, 1, width)[:64 * width] + bytes(32 * width)
    assert f(identity, identity) == 1 and f(identity, _scaled(p6, 0, width)) == 1            # z = 0, whatever x and y hold
    assert f(other_identity, identity) == 1 and f(identity, _scaled(p5, 1, width)) == 0


def test_ptau_verdict(chk):
    def verdict(first, k):
        text = C.create_string_buffer(256)
        rc = chk.dc_ptau_verdict((C.c_ulonglong * 5)(*first), k, text, 256)
        return rc, text.value.decode()

    assert verdict([NO_FAULT] * 5, 8) == (0, "")
    # the texts tests/test_gpu_zkey_verify.py and tests/test_gpu_zkey_new.py match
    first = [NO_FAULT] * 5
    first[2] = 7 << 3 | 2
    assert verdict(first, 8) == (-2, "ptau: section 14, block 8, element 7: the point is not on the curve")
    sections, kinds = [12, 13, 14, 15, 12], ["a coordinate is not below q", "the point is not on the curve", "the point is outside the subgroup"]
    for i in range(5):
        for kind in (1, 2, 3):
            first = [NO_FAULT] * 5
            first[i] = (100 + i) << 3 | kind
            assert verdict(first, 4) == (-2, "ptau: section %d, block %d, element %d: %s" % (sections[i], 5 if i == 4 else 4, 100 + i, kinds[kind - 1]))
    # the first range at fault is the one named
    assert verdict([NO_FAULT, 1 << 3 | 3, NO_FAULT, 2 << 3 | 1, NO_FAULT], 3)[1] == "ptau: section 13, block 3, element 1: the point is outside the subgroup"
