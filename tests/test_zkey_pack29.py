"""Host build of csrc/prover/zkey_pack29.h — the lane codec of a packed key's coefficient: the value v = file·R⁻² mod r coded by the
wtnz rules, and back through to_mont twice — compiled here with g++ and compared with tests/zkey_pack_model.py's Python integers,
byte for byte in both directions.  Every case is CONSTRUCTED.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
import zkey_pack_model as ZM

R = ZM.R_MOD
FULL = R // 3                                                               # 32 significant bytes, its negation too


@pytest.fixture(scope="module")
def chk():
    out = os.path.join(ROOT, "build", "zkey_pack29_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "zkey_pack29_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc"),
                    "-o", out, src], check=True)
    return C.CDLL(out)


def _encode(chk, file_value):
    code, pay = C.c_uint8(0xee), C.create_string_buffer(b"\xee" * 32, 32)
    n = chk.zp29_encode(int(file_value).to_bytes(32, "little"), C.byref(code), pay)
    return n, code.value, pay.raw


def _decode(chk, code, payload):
    out = C.create_string_buffer(32)
    kind = chk.zp29_decode(C.c_uint8(code), payload, len(payload), out)
    return kind, int.from_bytes(out.raw, "little")


def _round_trip(chk, v):
    """the standard-form value v: the library's code of v·R² is the model's, and decodes to v·R² again"""
    f = ZM.to_file(v)
    assert ZM.from_file(f) == v
    want_code, want_pay = ZM.WM.encode(v)
    n, code, pay = _encode(chk, f)
    assert (n, code, pay) == (len(want_pay), want_code, want_pay + bytes(32 - len(want_pay))), hex(v)
    assert _decode(chk, code, want_pay) == (0, f), hex(v)
    return code


def test_the_edges_of_every_rule(chk):
    codes = {v: _round_trip(chk, v) for v in (0, 1, R - 1, R - 2, (1 << 248) - 1, 1 << 248, R - (1 << 248), R - (1 << 248) + 1)}
    assert codes[0] == 0x00 and codes[1] == 0x40 and codes[R - 1] == 0x81 and codes[R - 2] == 0x81
    assert codes[(1 << 248) - 1] == 31 and codes[1 << 248] == 32
    assert codes[R - (1 << 248)] == 32                                       # m = 2^248 has 32 bytes: no shorter
    assert codes[R - (1 << 248) + 1] == 0x80 | 31
    for v in ZM.WM.edge_values():
        _round_trip(chk, v)


def test_every_payload_length_in_both_forms(chk):
    positive = {k: (1 << (8 * k)) - 1 for k in range(1, 32)}
    positive[32] = FULL
    for k, v in positive.items():
        assert _round_trip(chk, v) == k
    # a negated form has at most 31 bytes: below that r − m has 32 and the rule prefers m
    for k in range(1, 32):
        assert _round_trip(chk, R - ((1 << (8 * k)) - 1)) == 0x80 | k
        assert _round_trip(chk, R - (1 << (8 * (k - 1)))) == 0x80 | k     # the least m of k bytes
    assert _round_trip(chk, R - FULL) == 32


def test_file_values_not_below_r_are_refused(chk):
    for f in (R, R + 1, (1 << 256) - 1, 1 << 255):
        assert _encode(chk, f) == (-1, 0xee, b"\xee" * 32)
    assert _encode(chk, R - 1)[0] >= 0


def test_the_decoders_refusals_are_the_value_codes(chk):
    for code, payload, kind in ((0x21, b"", ZM.CODE), (0xa0, b"", ZM.CODE), (0x41, b"", ZM.CODE), (0x02, b"\x05\x00", ZM.NONCANONICAL), (0x83, b"\x01\x02\x00", ZM.NONCANONICAL),
                                (0x01, b"\x01", ZM.NONCANONICAL), (0x20, (R - 1).to_bytes(32, "little"), ZM.NONCANONICAL), (0x20, R.to_bytes(32, "little"), ZM.RANGE),
                                (0x20, b"\xff" * 32, ZM.RANGE)):
        assert ZM.decode_file(code, payload) == (None, kind)
        assert _decode(chk, code, payload) == (kind, 0)


def test_a_sweep_of_file_values(chk):
    """the bijection the other way round: file values chosen as such (v is whatever they decode to)"""
    import random
    rng = random.Random(5)
    for f in [0, 1, 2, R - 1, ZM.R2, R - ZM.R2] + [rng.randrange(R) for _ in range(200)]:
        want_code, want_pay = ZM.encode_file(f)
        n, code, pay = _encode(chk, f)
        assert (n, code, pay[:n]) == (len(want_pay), want_code, want_pay)
        assert _decode(chk, code, want_pay) == (0, f)
