"""Checked host build of csrc/prover/transcript.h — the one text of a ceremony contribution's Fiat–Shamir transcript that
groth16_ptau_contribute(s) and groth16_zkey_contribute(s) share — compiled here with g++ -DF29_CHECK and compared with hashlib and
Python integers: the wide hash at SHA-256's padding boundaries (and that it wipes its argument), the big-endian reduction mod r,
the challenge of a digest, and the walk over a section of records in both layouts with every way a section can be malformed.  The
walker and the reduction run once more in a program of their own built with -fsanitize=address,undefined, every input in a heap
block of exactly its size, as a child process.  Every case is CONSTRUCTED.  No GPU."""
import ctypes as C
import hashlib
import os
import struct
import subprocess

import pytest

from conftest import ROOT
import groth16_dlog_model as M

R = M.R
SRC = os.path.join(ROOT, "tests", "transcript_check.cpp")
FLAGS = ["-std=c++17", "-DF29_CHECK", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc")]
# (fixed bytes of a record, offset of name_len in them): section 7 of a .ptau, section 10 of a .zkey
LAYOUTS = {"ptau": (740, 736), "zkey": (164, 160)}

WIDE_LENGTHS = [0, 1, 54, 55, 56, 63, 64, 200]  # with the appended byte: 55 | 56 and 63 | 64 | 65 are SHA-256's padding boundaries
BE_VALUES = [0, R - 1, R, R + 1, (1 << 512) - 1]


def _record(layout, name, name_len=None):
    fixed, off = LAYOUTS[layout]
    body = bytes((7 * i + 1) & 0xff for i in range(fixed))
    return body[:off] + struct.pack("<I", len(name) if name_len is None else name_len) + body[off + 4:] + name


def walker_cases(layout):
    """(what, the section's bytes or None for no section, (rc, count, bad, len(recs)))"""
    rec = lambda name, name_len=None: _record(layout, name, name_len)
    n = lambda k: struct.pack("<I", k)
    return [
        ("no section", None, (0, 0, 0, 0)),
        ("an empty section", b"", (1, 0, 0, 0)),
        ("three bytes", b"\0\0\0", (1, 0, 0, 0)),
        ("a count of 0", n(0), (0, 0, 0, 0)),
        ("two records", n(2) + rec(b"alice") + rec(b""), (0, 2, 2, 2)),
        ("a name of 255 bytes", n(1) + rec(b"x" * 255), (0, 1, 1, 1)),
        ("a count of 2^32 - 1 in a 4-byte section", n(0xffffffff), (1, 0, 0, 0)),
        ("the count's records do not fit", n(1) + rec(b"")[:-1], (1, 0, 0, 0)),
        ("the second record cut one byte short", n(2) + rec(b"alice") + rec(b"")[:-1], (1, 2, 2, 1)),
        ("a name cut one byte short", n(1) + rec(b"bob")[:-1], (1, 1, 1, 0)),
        ("name_len = 256", n(1) + rec(b"y" * 256), (1, 1, 1, 0)),
        ("one trailing byte", n(1) + rec(b"carol") + b"\0", (1, 1, 1, 1)),
    ]


@pytest.fixture(scope="module")
def chk():
    out = os.path.join(ROOT, "build", "transcript_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-O1", "-fPIC", "-shared"] + FLAGS + ["-o", out, SRC], check=True)
    lib = C.CDLL(out)
    lib.ts_last_failure.restype = C.c_char_p
    yield lib
    assert lib.ts_last_failure().decode() == "", "F29_CHECK bound fired"


def _fe(buf):
    return int.from_bytes(buf.raw, "little")


def test_the_cases_are_what_they_claim():
    """conditions on the inputs, not measurements"""
    # a message of 55 bytes is the longest that SHA-256 pads inside its block (0x80 and the 8-byte length), 64 fills one exactly
    hashed = [length + 1 for length in WIDE_LENGTHS]
    assert {55, 56}.issubset(hashed) and {64, 65}.issubset(hashed) and 55 + 9 == 64
    assert BE_VALUES[1] < R <= BE_VALUES[2] and BE_VALUES[4].bit_length() == 512
    for layout, (fixed, off) in LAYOUTS.items():
        assert off + 4 == fixed
        r = _record(layout, b"alice")
        assert len(r) == fixed + 5 and struct.unpack_from("<I", r, off)[0] == 5 and r[fixed:] == b"alice"
        assert len(_record(layout, b"y" * 256)) == fixed + 256
        # the second record of the "cut short" case is reached: the count's own bound passes
        assert 4 + 2 * fixed <= len(struct.pack("<I", 2) + _record(layout, b"alice") + _record(layout, b"")[:-1])


@pytest.mark.parametrize("length", WIDE_LENGTHS)
def test_wide_hash_is_two_digests_mod_r_and_wipes_its_argument(chk, length):
    msg = bytes((11 * i + 3) & 0xff for i in range(length))
    out = C.create_string_buffer(32)
    wiped = chk.ts_wide_hash(C.c_char_p(msg), C.c_size_t(length), out)
    want = int.from_bytes(hashlib.sha256(msg + b"\0").digest() + hashlib.sha256(msg + b"\1").digest(), "big") % R
    assert _fe(out) == want
    assert wiped == 1


@pytest.mark.parametrize("value", BE_VALUES)
def test_fr_from_be_reduces_mod_r(chk, value):
    out = C.create_string_buffer(32)
    chk.ts_fr_from_be(C.c_char_p(value.to_bytes(64, "big")), C.c_size_t(64), out)
    assert _fe(out) == value % R


def test_the_challenge_is_sixteen_bytes_little_endian_and_never_zero(chk):
    out = C.create_string_buffer(32)
    for digest, want in ((bytes(16) + b"\xff" * 16, 1), (b"\xff" * 32, (1 << 128) - 1), (bytes(range(1, 33)), int.from_bytes(bytes(range(1, 17)), "little"))):
        chk.ts_challenge(C.c_char_p(digest), out)
        assert _fe(out) == want


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_the_record_walk(chk, layout):
    fixed, off = LAYOUTS[layout]
    for what, sec, want in walker_cases(layout):
        out = (C.c_uint32 * 4)()
        chk.ts_walk(C.c_char_p(sec), C.c_uint64(len(sec or b"")), C.c_int(sec is not None), C.c_uint64(fixed), C.c_uint64(off), out)
        assert tuple(out) == want, (layout, what)


def test_the_walk_and_the_reduction_under_the_sanitizers(tmp_path):
    """a program of its own (-DTRANSCRIPT_MAIN), run as a child process: nothing is loaded into this interpreter"""
    prog = str(tmp_path / "transcript_check")
    subprocess.run(["g++", "-O1", "-g", "-DTRANSCRIPT_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS + ["-o", prog, SRC], check=True)
    args, want = [], []
    for layout, (fixed, off) in sorted(LAYOUTS.items()):
        for what, sec, verdict in walker_cases(layout):
            args.append("w:%d:%d:%s" % (fixed, off, "-" if sec is None else sec.hex()))
            want.append("%d %d %d %d" % verdict)
    for value in BE_VALUES:
        args.append("b:" + value.to_bytes(64, "big").hex())
        want.append("%064x" % (value % R))
    run = subprocess.run([prog] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.split("\n")[:-1] == want
