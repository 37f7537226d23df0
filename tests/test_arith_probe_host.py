"""The lane-level arithmetic (csrc/ff.h, ec.h, ff29.h, fr29.h, ec29.h) through the HOST twin of tests/arith_probe.hip, one
primitive per case, against Python integers (tests/arith_probe_model.py).  This proves the models and the input lists of
tests/test_gpu_arith_probe.py on a machine without a GPU, gives the portable CIOS paths the same edge inputs, and runs the lazy
radix-2^29 operations in the bound-checked build as well.  No GPU."""
import numpy as np
import pytest

import arith_probe_cases as AP
import arith_probe_model as M
from field_inputs import ints_to_words, words_to_ints


@pytest.mark.parametrize("case", AP.HOST_CASES)
def test_host_twin(O, case):
    build, _ = AP.CASES[case]
    build(O).run(AP.run_host)


@pytest.mark.parametrize("grp", ["g1", "g2"])
def test_integer_group_law_matches_the_oracle(O, grp):
    """the affine law of the model against O.ec_add / O.ec_dbl on the generic pairs, and k·G + l·G = (k + l)·G on the small multiples"""
    F, B = M.FIELD[grp], AP.base_points(O, grp)
    assert all(M.on_curve(F, P) for P in B)

    def arr(P):
        return ints_to_words(F.flat(P[0]) + F.flat(P[1])).reshape(2 * F.words, 4)

    def pt(a):
        w = words_to_ints(np.asarray(a).reshape(-1, 4))
        return None if not any(w) else (F.unflat(w[:F.words]), F.unflat(w[F.words:]))
    for P, Q in AP.point_pairs(O, grp)[:64]:
        s = O.ec_to_affine(grp, O.ec_add(grp, O.ec_from_affine(grp, arr(P)), O.ec_from_affine(grp, arr(Q))))
        assert pt(s) == M.ec_add(F, P, Q)
        d = O.ec_to_affine(grp, O.ec_dbl(grp, O.ec_from_affine(grp, arr(P))))
        assert pt(d) == M.ec_add(F, P, P)
    for k in range(1, 16):
        assert M.ec_add(F, B[k - 1], B[k]) == B[2 * k] and M.ec_add(F, B[k], M.ec_neg(F, B[k])) is None   # B[i] = (i + 1)·G
    assert M.ec_add(F, None, B[3]) == B[3] and M.ec_add(F, B[3], None) == B[3] and M.ec_add(F, None, None) is None


def test_every_probe_is_covered_and_the_lists_have_a_partial_last_wave(O):
    ops = set()
    for case, (build, _) in AP.CASES.items():
        c = build(O)
        ops.update(c.ops)
        assert len(c.lanes) % 64 or (case.endswith("-chain") and len(c.lanes) == AP.CHAIN_LANES), case
    assert ops == set(AP.SHAPES)
