"""Host check of csrc/msm_sort_plan.h — the shape msm_sort.hip allocates and enqueues for one digit sort, as the pure function
msm_sort_shape — as a stand-alone program (tests/msm_sort_plan_check.cpp), built with g++ once plainly and once with
-fsanitize=address,undefined and run over the combinations of the recode sweep (tests/test_msm_recode_host.py) with an entries hint
of 0 and of L: both workspace layouts keep their stated order, their regions are disjoint and end inside the allocation, large_items
is 8-byte aligned, and each sort path holds its own conditions and is reached.  The "digit sort" column of DESIGN §6 is pinned here.
No GPU."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
import msm_inputs as MI

SRC = os.path.join(ROOT, "tests", "msm_sort_plan_check.cpp")
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc")]

CLASSIC_TWO_LEVEL = [256, 257, 4097, 8192, 32768, 524289, 1 << 22]
TABLE_TWO_LEVEL = [32768, (1 << 22) + 1, 1 << 23, (1 << 23) + 1, 1 << 24]
TABLE_STAGED = {32769: (5, 10), 65537: (6, 10), 131072: (7, 9), 262145: (8, 10), 524289: (9, 10), 1_600_000: (10, 9), 3_200_000: (11, 8), 1 << 22: (11, 8)}
WITNESS_STAGED = {33_002: (16, (5, 10)), 262_202: (18, (8, 9))}   # wires: forced digit width, (pb, low)


def _build(name, extra):
    out = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", *extra, *FLAGS, "-o", out, SRC], check=True)
    return out


@pytest.fixture(scope="module")
def plain():
    return _build("msm_sort_plan_check", ["-O2"])


@pytest.fixture(scope="module")
def sanitized():
    return _build("msm_sort_plan_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def _sweep(exe):
    out = subprocess.run([exe, "sweep"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    m = re.search(r"combinations (\d+) staged (\d+) two_level (\d+) global (\d+) errors (\d+) failures (\d+)", out.stdout)
    assert m, out.stdout
    combos, staged, two_level, glob, errors, failures = map(int, m.groups())
    assert failures == 0
    assert combos == 55 * 25 * 10 * 7 * 4 * 2                               # lengths × c_cfg × tab × bits × pf × entries hint
    assert staged + two_level + glob + errors == combos
    for path in ("staged", "two-level", "global"):                         # one combination of each path, by name
        assert re.search(r"^path %s L=\d+ " % path, out.stdout, re.M), out.stdout
    return out.stdout


def test_sweep(plain):
    _sweep(plain)


def test_sweep_under_the_sanitizers(sanitized):
    _sweep(sanitized)


def _shapes(exe, queries):
    out = subprocess.run([exe, "shape"] + ["%d,0,%d,0,%d,0" % q for q in queries], capture_output=True, text=True, check=True)
    return [line.split() for line in out.stdout.strip().split("\n")]


def test_the_pinned_paths(plain):
    """DESIGN §6, "digit sort": automatic digit width; classic lengths and the table mode's c = 15 and lengths beyond 2^22 sort
    two-level, the table mode from 32769 to 2^22 points and the prover's witness tables LDS-staged with these partitions"""
    for f in _shapes(plain, [(L, 0, 1) for L in CLASSIC_TWO_LEVEL]):
        assert f[0] == "two-level", f
    rows = _shapes(plain, [(L, 1, 1) for L in TABLE_TWO_LEVEL])
    assert all(f[0] == "two-level" for f in rows), rows
    assert rows[0][3:5] == ["15", "17"]
    for (L, want), f in zip(TABLE_STAGED.items(), _shapes(plain, [(L, 1, 1) for L in TABLE_STAGED])):
        assert f[0] == "staged" and (int(f[1]), int(f[2])) == want, (L, f)
    for (wires, (c, want)), f in zip(WITNESS_STAGED.items(), _shapes(plain, [(w, c, 1) for w, (c, _) in WITNESS_STAGED.items()])):
        assert MI.WITNESS_GEOMS[wires][0] == c and int(f[3]) == c
        assert f[0] == "staged" and (int(f[1]), int(f[2])) == want, (wires, f)


def test_the_point_index_error(plain):
    """2^29 scalars with eight precomputed points each: 32 index bits — the one error msm_sort_run returns from its shape"""
    out = subprocess.run([plain, "shape", "%d,0,0,0,8,0" % (1 << 29), "%d,0,0,0,4,0" % (1 << 29)], capture_output=True, text=True, check=True)
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "error msm: 536870912 scalars x precompute_factor 8 exceed the 31-bit point index of a sort entry"
    assert lines[1].split()[0] == "global"
