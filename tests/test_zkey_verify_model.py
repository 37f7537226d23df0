"""The discrete-log model of groth16_zkey_verify_ptau (tests/zkey_verify_dlog_model.py) against the constructed cases
(tests/zkey_verify_cases.py): it accepts setup()'s key and rejects every mutation under the first kind the case names.  No GPU and
no curve arithmetic: the GPU test asks the library for exactly what the model says here."""
import hashlib

import pytest

import zkey_verify_cases as cases
import zkey_verify_dlog_model as M

SEED = hashlib.sha256(b"zkey-verify model").digest()


@pytest.fixture(scope="module")
def all_cases(S):
    return cases.cases(S)


def test_coefficients_are_the_combined_verifiers(K):
    assert [M.coefficient(SEED, i) for i in (0, 1, 162, 163, 418)] == [K.verify_combined_coefficients(SEED, i, 1)[0] for i in (0, 1, 162, 163, 418)]


def test_model_accepts_the_key_and_names_every_mutation(S, all_cases):
    ptau = S.toxic_waste()[:3]
    seen = set()
    for name, r, key, header, kind, mask in all_cases:
        got = M.evaluate(S, r, key, header, ptau, SEED)
        assert got[0] == kind, (name, got)
        if mask is not None:
            assert got[2] == mask, (name, got)
        assert (got[2] == 0) == (kind == 0) and (kind == 0 or got[2] & M.bit(kind))
        seen.add(kind)
    assert seen == {0, M.HEADER, M.A, M.B1, M.B2, M.IC, M.C, M.H}


def test_masks_of_the_wholesale_mutations(S, all_cases):
    by_name = {c[0]: c for c in all_cases}
    ptau = S.toxic_waste()[:3]
    ev = lambda name: M.evaluate(S, *by_name[name][1:4], ptau, SEED)
    # another circuit: everything that reads the matrices fails, H (which reads none) holds
    assert ev("another circuit of the same sizes")[2] == M.bit(M.A) | M.bit(M.B1) | M.bit(M.B2) | M.bit(M.IC) | M.bit(M.C)
    # another tau: every equation over the ptau's Lagrange points fails, H included
    assert ev("another tau, header alpha and beta the ptau's")[2] == sum(M.bit(k) for k in (M.A, M.B1, M.B2, M.IC, M.C, M.H))
    assert ev("another tau, alpha and beta") == (M.HEADER, 0, sum(M.bit(k) for k in range(M.HEADER, M.H + 1)))


def test_h_basis_is_snarkjs_odd_lagrange_points(S):
    """setup()'s section 9, L_i(τ/g)·(τⁿ − 1)/(−2δ), is L'_{2i+1}(τ)/δ for the doubled domain — the H row of the check"""
    tau, _, _, _, delta = S.toxic_waste()
    for nc in (1, 5, 29):
        r = S.squaring_chain(nc)[0]
        ks = S.key_scalars(r)
        n = ks["n"]
        L2 = S.lagrange_at(2 * n, n.bit_length(), tau)
        assert [h * delta % M.R for h in ks["h"]] == L2[1::2]
