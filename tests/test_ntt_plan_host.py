"""Host check of csrc/ntt_plan.h — everything ntt.hip enqueues for one transform, as the pure function ntt_plan — as a stand-alone
program (tests/ntt_plan_check.cpp), built with g++ once plainly and once with -fsanitize=address,undefined and run over every
log n in 0 … 27, the domain at log n, log n + 3 and 27, both directions, batch 1 … 3, every fusion, and the radix-2^29 kernels allowed
and not: the passes' bits sum to log n, dynamic LDS and grids fit, every pass's load and store map is a bijection onto [0, n), the
radix-2^29 bounds hold level by level as the kernels consume them, and up to 2^17 the plan, executed on the host over a 31-bit
prime, is the DFT in natural order.  The plan table of DESIGN §6 is pinned here.  No GPU."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "ntt_plan_check.cpp")
FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc")]

# log n: (bits per pass, (shrink_last, end bound) per pass forward, the same inverse); None: not pinned
PLANS29 = {
    11: ([6, 5], [(0, 71), (0, 131)], None),
    12: ([6, 6], [(0, 71), (0, 263)], None),
    13: ([8, 5], [(0, 259), (0, 131)], None),
    14: ([8, 6], [(0, 259), (0, 263)], None),
    15: ([8, 7], [(0, 259), (0, 513)], [(0, 259), (1, 133)]),
    16: ([8, 8], [(0, 259), (1, 267)], None),
    17: ([6, 6, 5], [(0, 71), (0, 263), (0, 131)], None),
    18: ([6, 6, 6], [(0, 71), (0, 263), (0, 263)], None),
    19: ([8, 6, 5], [(0, 259), (0, 263), (0, 131)], None),
    20: ([8, 6, 6], [(0, 259), (0, 263), (0, 263)], None),
    21: ([8, 8, 5], [(0, None), (1, None), (0, None)], None),
    22: ([8, 8, 6], [(0, None), (1, None), (0, None)], None),
    23: ([8, 8, 7], [(0, None), (1, None), (0, 513)], [(0, None), (1, None), (1, 133)]),
    24: ([8, 8, 8], [(0, None), (1, None), (1, None)], None),
}


def _build(name, extra):
    out = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", *extra, *FLAGS, "-o", out, SRC], check=True)
    return out


@pytest.fixture(scope="module")
def plain():
    return _build("ntt_plan_check", ["-O2"])


@pytest.fixture(scope="module")
def sanitized():
    return _build("ntt_plan_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def _sweep(exe):
    out = subprocess.run([exe, "sweep"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    m = re.search(r"plans (\d+) passes (\d+) enumerated_maps (\d+) executed (\d+) bound_walks (\d+) plan_errors (\d+) failures (\d+)", out.stdout)
    assert m, out.stdout
    plans, passes, enumerated, executed, walks, errors, failures = map(int, m.groups())
    assert failures == 0
    # (size, domain) pairs: three domains up to 2^23, two for 2^24 … 2^26, one for 2^27; × 2 directions × 2 families × 3 batches × 3 fusions
    assert plans + errors == (24 * 3 + 3 * 2 + 1) * 2 * 2 * 3 * 3 and errors < plans  # (errors: the fused epilogues that are refused)
    assert executed == 18 * 3 * 2 * 2 and enumerated >= 2 * 21 * 2 and walks >= 14 * 2 * 2 * 3 and passes > plans


def test_sweep(plain):
    _sweep(plain)


def test_sweep_under_the_sanitizers(sanitized):
    _sweep(sanitized)


def test_the_pinned_plans(plain):
    """The NTT table of DESIGN §6: 0 … 9 one pass, 10 [5,5], 11 … 24 the radix-2^29 splits with their shrinks and end bounds,
    25 … 27 three passes with 9 bits first; n / 2048 tiles per pass from 2^11 on; the one-dimensional grid from 2^14 on."""
    out = subprocess.run([plain, "table"], capture_output=True, text=True, check=True)
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "first_xcd_batch 14"
    rows = {}
    for line in lines[:-1]:
        f = line.split()
        rows[(int(f[0]), f[1])] = (f[2], [tuple(int(x) for x in p.split(":")) for p in f[3:]])
    assert len(rows) == 56
    for logn in range(28):
        for d in ("forward", "inverse"):
            family, passes = rows[(logn, d)]
            bits = [p[0] for p in passes]
            if logn >= 11:
                assert all(p[1] == (1 << logn) // 2048 for p in passes), (logn, passes)
            if logn in PLANS29:
                want_bits, fwd, inv = PLANS29[logn]
                want = fwd if d == "forward" or inv is None else inv
                assert family == "29" and bits == want_bits, (logn, d, passes)
                for p, (shrink, end) in zip(passes, want):
                    assert p[2] == shrink and (end is None or p[3] == end), (logn, d, passes)
            else:
                assert family == "8x32"
                assert bits == ([logn] if logn <= 9 else [5, 5] if logn == 10 else [9, (logn - 8) // 2, (logn - 9) // 2]), (logn, passes)
