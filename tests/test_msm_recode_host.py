"""Host check of csrc/msm_recode.h — the MSM's host plan and the signed-digit recoding its sort kernels run per scalar — as a
stand-alone program (tests/msm_recode_check.cpp), built with g++ once plainly and once with -fsanitize=address,undefined and run
over every length bracket, forced digit width, table request, scalar width and precompute factor the C ABI admits: the windows
cover the scalar, H holds one bit per window, and for the edge values of tests/msm_inputs.py, the edges of each geometry's own
windows and 4096 seeded random scalars the digits sum to s', stay inside their windows, leave nothing above the top window and land
inside the bucket array.  The plan restated in tests/msm_inputs.py (which names the geometries of the GPU sweeps) is held against
the C++ here.  No GPU."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
import msm_inputs as MI
from fr_inputs import edge_fr

SRC = os.path.join(ROOT, "tests", "msm_recode_check.cpp")
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc")]


def _build(name, extra):
    out = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", *extra, *FLAGS, "-o", out, SRC], check=True)
    return out


@pytest.fixture(scope="module")
def plain():
    return _build("msm_recode_check", ["-O2"])


@pytest.fixture(scope="module")
def sanitized():
    return _build("msm_recode_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


@pytest.fixture(scope="module")
def values(tmp_path_factory):
    p = tmp_path_factory.mktemp("msm_recode") / "edge_values.txt"
    vals = edge_fr() + MI.recode_limits()
    p.write_text("".join("%x\n" % v for v in vals))
    return str(p)


def _sweep(exe, values):
    out = subprocess.run([exe, "sweep", values], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    m = re.search(r"combinations (\d+) geometries (\d+) scalars (\d+) digits (\d+) all_windows_narrowed (\d+) failures (\d+)", out.stdout)
    assert m, out.stdout
    combos, geoms, scalars, digits, narrowed_all, failures = map(int, m.groups())
    assert failures == 0
    assert combos == 55 * 25 * 10 * 7 * 4                                   # lengths × c_cfg × tab × bits × pf
    assert geoms >= 200 and scalars >= geoms * 1000 and digits > scalars   # the sweep did not collapse to a handful of geometries
    assert narrowed_all >= 1                                                # c = 18 / 15 windows: every window one bit narrow
    return m.group(0)


def test_sweep(plain, values):
    _sweep(plain, values)


def test_sweep_under_the_sanitizers(sanitized, values):
    _sweep(sanitized, values)


def test_the_restated_plan_is_the_plan(plain):
    """tests/msm_inputs.py: geometry() and witness_geometry() against msm_geometry_plan, at every length of the sweeps and their
    neighbours, classic and table mode, and table mode with each forced digit width"""
    Ls = sorted({L + d for L in list(MI.TABLE_GEOMS) + list(MI.CLASSIC_GEOMS) + list(MI.WITNESS_GEOMS) + [1, 16, 1 << 20, 1 << 21, 1 << 22, 1 << 23, 3 << 20] for d in (-1, 0, 1)})
    queries = [(L, tab) for L in Ls for tab in (0, 1, 13, 16, 17, 18, 19, 20)]
    out = subprocess.run([plain, "geom"] + ["%d,0,%d,0,1" % q for q in queries], capture_output=True, text=True, check=True)
    lines = out.stdout.split("\n")
    for (L, tab), line in zip(queries, lines):
        c, W, wide, t, nbuckets, _, _ = map(int, line.split())
        g = MI.geometry(L, tab)
        assert (g["c"], g["W"], g["wide"], g["tab"], g["nbuckets"]) == (c, W, wide, t, nbuckets), (L, tab, line)
    for wires, geom in MI.WITNESS_GEOMS.items():
        g = MI.witness_geometry(wires)
        out = subprocess.run([plain, "geom", "%d,0,%d,0,1" % (wires, g["c"])], capture_output=True, text=True, check=True)
        assert tuple(map(int, out.stdout.split()[:3])) == geom == (g["c"], g["W"], g["wide"])
