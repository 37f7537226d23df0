"""Which part of a key's base arrays a shard holds (csrc/prover/shard_ranges.h), printed by the stand-alone program
tests/shard_ranges_check.cpp for a grid of small shapes and checked here by property — not by the header's formulas again.  The program
is built twice, plainly and with the address and undefined-behaviour sanitizers; both builds must print the same.  No GPU."""
import collections
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

Line = collections.namedtuple("Line", "n_vars n_public domain count rank wlo whi clo chi hlo hhi h_stride h_first slice_aligned h_strided")


def _build_and_run(name, *flags):
    out = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-O1", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc"), "-o", out,
                    os.path.join(ROOT, "tests", "shard_ranges_check.cpp")], check=True)
    return subprocess.run([out], check=True, capture_output=True, text=True).stdout


@pytest.fixture(scope="module")
def groups():
    """{(n_vars, n_public, domain, count): [Line of rank 0, 1, …]}"""
    text = _build_and_run("shard_ranges_check")
    g = collections.OrderedDict()
    for ln in text.splitlines():
        r = Line(*map(int, ln.split()))
        g.setdefault(r[:4], []).append(r)
    return text, g


def test_grid_is_complete(groups):
    _, g = groups
    shapes = {k[:3] for k in g}
    assert {s[0] for s in shapes} == {1, 2, 7, 64, 1000, 1025} and {s[2] for s in shapes} == {1024, 4096, 8192}
    for n_vars in (7, 64, 1000, 1025):
        assert {s[1] for s in shapes if s[0] == n_vars} == {0, 1, n_vars - 1}
    assert {s[1] for s in shapes if s[0] == 1} == {0} and {s[1] for s in shapes if s[0] == 2} == {0, 1}
    for key, rows in g.items():
        assert [r.rank for r in rows] == list(range(key[3])), key
    assert {k[3] for k in g} == set(range(1, 9))


def test_sanitized_build_prints_the_same(groups):
    text, _ = groups
    assert _build_and_run("shard_ranges_check_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all") == text


def test_witness_ranges_tile_the_wires_in_order(groups):
    _, g = groups
    for key, rows in g.items():
        n_vars = key[0]
        assert rows[0].wlo == 0 and rows[-1].whi == n_vars, key
        for a, b in zip(rows, rows[1:]):
            assert a.whi == b.wlo, key
        assert all(r.wlo <= r.whi for r in rows), key


def test_c_range_is_the_witness_range_cut_to_the_private_wires(groups):
    _, g = groups
    for key, rows in g.items():
        n_vars, n_public = key[0], key[1]
        private = range(n_public + 1, n_vars)
        for r in rows:
            want = [w - (n_public + 1) for w in range(r.wlo, r.whi) if w in private]
            assert list(range(r.clo, r.chi)) == want, (key, r.rank)
            assert r.clo <= r.chi <= n_vars - n_public - 1, (key, r.rank)


def test_h_pieces_cover_the_domain_exactly_once(groups):
    _, g = groups
    for key, rows in g.items():
        domain, count = key[2], key[3]
        strided = {r.h_strided for r in rows}
        assert len(strided) == 1, key
        if strided == {1}:
            # a residue class per rank: the elements h_first + k·h_stride, k in [hlo, hhi)
            assert all(r.h_stride == count and r.hlo == 0 for r in rows), key
            pieces = [r.h_first + np.arange(r.hlo, r.hhi) * r.h_stride for r in rows]
        else:
            assert all(r.h_stride == 1 and r.h_first == 0 for r in rows), key
            pieces = [np.arange(r.hlo, r.hhi) for r in rows]
        assert np.array_equal(np.sort(np.concatenate(pieces)), np.arange(domain)), key
        # the folded front end serves a class only for a power-of-two count (csrc/prover/qap.h: qap_coset_fold3)
        if strided == {1}:
            assert count > 1 and count & (count - 1) == 0, key


def test_slice_aligned_exactly_when_the_slice_split_leaves_no_rank_empty(groups):
    _, g = groups
    seen = set()
    for key, rows in g.items():
        n_vars, count = key[0], key[3]
        aligned = {r.slice_aligned for r in rows}
        assert len(aligned) == 1, key
        if count == 1:
            continue  # (one shard holds everything: test_witness_ranges_tile…; no slice to be aligned with)
        per_rank = -(-n_vars // count)  # what a rank uploads of the witness: ⌈n_vars / count⌉ wires from rank·per_rank
        slices = [(min(n_vars, k * per_rank), min(n_vars, (k + 1) * per_rank)) for k in range(count)]
        none_empty = all(lo < hi for lo, hi in slices)
        assert aligned == {int(none_empty)}, key
        seen.add(none_empty)
        if none_empty:
            assert [(r.wlo, r.whi) for r in rows] == slices, key
    assert seen == {True, False}
