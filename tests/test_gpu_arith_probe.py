"""The lane-level arithmetic on the DEVICE — the product-scanning Montgomery multiply and the fused mul2sum of ff.h, Fq2 in both
of its builds, the group law of ec.h with every exceptional branch, the lazy radix-2^29 fields and curves — one primitive per
case through the kernels of tests/arith_probe.hip (libisnark_arith_probe.so), lane by lane against Python integers.  The cases,
input lists and models are those of tests/test_arith_probe_host.py; only the runner differs.  A failure names the primitive,
the first failing lane and its inputs."""
import pytest

import arith_probe_cases as AP

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(AP.CASES))
def test_device_probe(gpu, O, case):
    build, variant = AP.CASES[case]
    build(O).run(AP.run_device, variant)     # every launcher's return code is asserted to be 0 before any comparison (AP._call)
