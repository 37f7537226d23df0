"""Checked host build of csrc/prover/ptau_verify29.h — the scalars of groth16_ptau_verify's Lagrange equations: x, y, μ_p, C, T from
the seed, and λ_e and d_i as one lane computes them from the two small tables — compiled here with g++ -DF29_CHECK and compared
with the Python model (tests/ptau_verify_model.py).  Elements: 0, 1, both sides of every block border up to 8, both sides of the
table border 2^k, the last; powers 0, 1, 3, 7 and 27; x from three seeds.  Every case is CONSTRUCTED.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
import ptau_contribute_model as CM
import ptau_prepare_model as PM
import ptau_verify_model as VM

R = PM.R
POWERS = [0, 1, 3, 7, 27]
SEEDS = [bytes(range(32)), bytes([0xA5]) * 32, bytes(range(255, 223, -1))]
BLOCKS = 29


@pytest.fixture(scope="module")
def chk():
    out = os.path.join(ROOT, "build", "ptau_verify29_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "ptau_verify29_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-DF29_CHECK", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc"), "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.pv29_last_failure.restype = C.c_char_p
    lib.pv29_table_bits.restype = C.c_uint32
    lib.pv29_derive.restype = C.c_uint32
    lib.pv29_lagrange.restype = C.c_uint64
    lib.pv29_reset()
    yield lib
    assert lib.pv29_last_failure().decode() == "", "F29_CHECK bound fired"


def _words(v):
    return int(v).to_bytes(32, "little")


def _ints(buf):
    return [int.from_bytes(buf.raw[32 * i:32 * i + 32], "little") for i in range(len(buf.raw) // 32)]


class Derived:
    """pv_derive's values and the four tables of (seed, power) from the checked build"""

    def __init__(self, chk, seed, power):
        self.chk, self.power, self.k = chk, power, chk.pv29_table_bits(power)
        bufs = [C.create_string_buffer(32) for _ in range(2)] + [C.create_string_buffer(32 * BLOCKS) for _ in range(4)]
        self.tries = chk.pv29_derive(C.c_char_p(seed), C.c_uint32(power), *bufs)
        self.x, self.y = _ints(bufs[0])[0], _ints(bufs[1])[0]
        self.mu, self.c, self.t12, self.t13 = (_ints(b) for b in bufs[2:])
        self.c_buf, self.t_buf = bufs[3], {power + 1: bufs[4], power: bufs[5]}
        n_lo, self.n_hi = 1 << self.k, 1 << (power + 1 - self.k)
        self.tab = {}
        for name, base, start in (("y", self.y, self.y), ("w", PM.omega(power + 1), 1)):
            lo, hi = C.create_string_buffer(32 * n_lo), C.create_string_buffer(32 * self.n_hi)
            chk.pv29_tables(C.c_char_p(_words(base)), C.c_char_p(_words(start)), C.c_uint32(self.k), C.c_uint32(self.n_hi), lo, hi)
            self.tab[name] = (lo, hi)

    def d(self, i, pmax):
        out = C.create_string_buffer(32)
        lo, hi = self.tab["y"]
        assert i >> self.k < self.n_hi
        self.chk.pv29_power(lo, hi, C.c_uint32(self.k), C.c_uint64(i), self.t_buf[pmax], out)
        return _ints(out)[0]

    def lam(self, e):
        out = C.create_string_buffer(32)
        lo, hi = self.tab["w"]
        t = self.chk.pv29_lagrange(lo, hi, C.c_uint32(self.k), C.c_uint32(self.power), C.c_uint64(e), C.c_char_p(_words(self.x)), self.c_buf, out)
        assert t >> self.k < self.n_hi
        return _ints(out)[0], t


def _source_indices(power, pmax):
    """0, 1, both sides of every block border up to 8, both sides of the table border, the last — those that exist"""
    k, last = CM.table_bits(power), min((2 << power) - 2, (1 << pmax) - 1)
    return sorted({i for i in list(range(9)) + [(1 << k) - 1, 1 << k, (1 << k) + 1, last] if i <= last})


def _prepared_elements(power):
    """the same for section 12's 4N − 1 elements; the table border is crossed by Ω's exponent, which is j in the last block"""
    k, last, top = CM.table_bits(power), (4 << power) - 2, (2 << power) - 1
    return sorted({e for e in list(range(9)) + [top - 1, top, top + (1 << k) - 1, top + (1 << k), last] if e <= last})


def test_the_cases_are_what_they_claim():
    assert [CM.table_bits(p) for p in POWERS] == [1, 1, 2, 4, 14]
    assert _source_indices(0, 1) == [0] and _source_indices(0, 0) == [0] and _source_indices(1, 2) == [0, 1, 2] and _source_indices(1, 1) == [0, 1]
    assert _source_indices(3, 4) == list(range(9)) + [14] and _source_indices(3, 3) == list(range(8))
    assert _source_indices(7, 8)[-4:] == [15, 16, 17, 254] and _source_indices(27, 28)[-4:] == [(1 << 14) - 1, 1 << 14, (1 << 14) + 1, (1 << 28) - 2]
    assert _prepared_elements(0) == [0, 1, 2] and _prepared_elements(3) == list(range(9)) + [14, 15, 18, 19, 30]
    assert _prepared_elements(27)[-1] == (1 << 29) - 2
    # block borders: e = 2^p − 1 begins block p; 0 … 8 holds both sides of the borders 1, 3, 7
    assert [VM.block_of(e) for e in range(9)] == [0, 1, 1, 2, 2, 2, 2, 3, 3]
    assert len(set(SEEDS)) == 3


@pytest.mark.parametrize("power", POWERS)
def test_the_derived_values_are_the_models(chk, power):
    for seed in SEEDS:
        d = Derived(chk, seed, power)
        x, c = VM.x_of(seed, power)
        mu = lambda p: VM.mu_of(seed, p)
        assert (d.x, d.tries) == (x, c) and d.y == pow(x, -1, R)
        for p in range(BLOCKS):
            live = p <= power + 1
            assert d.mu[p] == (mu(p) if live else 0)
            assert d.c[p] == (mu(p) * (pow(x, 1 << p, R) - 1) % R if live else 0)
            assert d.t12[p] == (VM.t_of(p, power + 1, x, mu) if live else 0)
            assert d.t13[p] == (VM.t_of(p, power, x, mu) if p <= power else 0)
    assert chk.pv29_last_failure().decode() == ""


@pytest.mark.parametrize("power", POWERS)
def test_the_lanes_scalars_are_the_models(chk, power):
    k = CM.table_bits(power)
    for seed in SEEDS:
        d = Derived(chk, seed, power)
        x, _ = VM.x_of(seed, power)
        mu = lambda p: VM.mu_of(seed, p)
        for pmax in (power + 1, power):
            for i in _source_indices(power, pmax):
                assert d.d(i, pmax) == VM.d_of(i, pmax, x, mu), (power, pmax, i)
        sides = set()
        for e in _prepared_elements(power):
            got, t = d.lam(e)
            assert got == VM.lam(power, e, x, mu), (power, e)
            sides.add(t >> k != 0)
        assert sides == ({False, True} if power >= 1 else {False})          # Ω's exponent on both sides of the table border
    assert chk.pv29_last_failure().decode() == ""
