"""Checked host build of the radix-2^29 pairing (csrc/pairing29.h) that the batched GPU verifier runs: compiled here with
g++ -DF29_CHECK, which turns every lazy bound of ff29.h / ec29.h / pairing29.h into a recorded failure, and compared with
the library's host pairing (bn254_pairing), its host verifier (groth16_verify_json) and a discrete-log model of the
verification equation that needs no pairing at all (tests/groth16_dlog_model.py).  No GPU."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden, unhex
import groth16_dlog_model as M

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R_ORDER = 21888242871839275222246405745257275088548364400416034343698204186575808495617


@pytest.fixture(scope="module")
def chk():
    out = os.path.join(ROOT, "build", "pairing29_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "pairing29_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-DF29_CHECK", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc"), "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.p29_last_failure.restype = C.c_char_p
    lib.p29_reset()
    yield lib
    assert lib.p29_last_failure().decode() == "", "F29_CHECK bound fired"


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _arr(ints):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in ints), dtype=np.uint64).reshape(-1, 4).copy()


def _ints(a):
    return [int.from_bytes(r.tobytes(), "little") for r in np.asarray(a).reshape(-1, 4)]


def _pairing29(chk, P, Qs):
    P = np.ascontiguousarray(P.reshape(-1, 2, 4))
    Qs = np.ascontiguousarray(Qs.reshape(-1, 4, 4))
    out = np.zeros((len(P), 12, 4), dtype=np.uint64)
    chk.p29_pairing(_p(P), _p(Qs), len(P), _p(out))
    assert chk.p29_last_failure().decode() == ""
    return out


def test_pairing_matches_host_on_golden_cases(chk, K):
    for c in load_golden("pairing.json")["cases"]:
        P, Qp = unhex(c["p"], 2, 4), unhex(c["q"], 4, 4)
        got = _pairing29(chk, P, Qp)[0]
        assert np.array_equal(got, unhex(c["e"], 12, 4)), (c["a"], c["b"])
        assert np.array_equal(got, K.pairing(P, Qp))


def test_pairing_matches_host_on_random_pairs(chk, K):
    rnd = random.Random(2929)
    g1, g2 = K.ec("g1", "generator"), K.ec("g2", "generator")
    Ps, Qs = [], []
    for _ in range(20):
        Ps.append(K.ec("g1", "to_affine", K.ec("g1", "mul_scalar", g1, rnd.randrange(1, R_ORDER))))
        Qs.append(K.ec("g2", "to_affine", K.ec("g2", "mul_scalar", g2, rnd.randrange(1, R_ORDER))))
    # P = −P', Q = the generator, and the identity on either side
    P0 = Ps[0].copy()
    P0[1] = _arr([(Q - int.from_bytes(Ps[0][1].tobytes(), "little")) % Q])[0]
    Ps.append(P0)
    Qs.append(K.ec("g2", "to_affine", g2))
    Ps += [np.zeros((2, 4), dtype=np.uint64), Ps[1]]
    Qs += [Qs[2], np.zeros((4, 4), dtype=np.uint64)]
    got = _pairing29(chk, np.stack(Ps), np.stack(Qs))
    for i in range(len(Ps)):
        assert np.array_equal(got[i], K.pairing(Ps[i], Qs[i])), i
    one = np.zeros((12, 4), dtype=np.uint64)
    one[0, 0] = 1
    assert np.array_equal(got[-1], one) and np.array_equal(got[-2], one)
    # e(−P, Q) = e(P, Q)⁻¹
    assert np.array_equal(got[20], K.gt_op("inv", K.pairing(Ps[0], Qs[20])))


def _dec(s):
    return int(s)


def _vk_arrays(S):
    from test_verify import _golden_vk_json
    g, vkj = _golden_vk_json(S)
    vk = json.loads(vkj)
    alpha = _arr([_dec(x) for x in vk["vk_alpha_1"][:2]])
    g2 = lambda v: _arr([_dec(v[0][0]), _dec(v[0][1]), _dec(v[1][0]), _dec(v[1][1])])
    ic = _arr([_dec(x) for p in vk["IC"] for x in p[:2]])
    return g, vkj, vk, alpha, g2(vk["vk_beta_2"]), g2(vk["vk_gamma_2"]), g2(vk["vk_delta_2"]), ic, int(vk["nPublic"])


def _verify29(chk, keyarrs, proof, public):
    _, _, _, alpha, beta, gamma, delta, ic, n_pub = keyarrs
    a = _arr([_dec(x) for x in proof["pi_a"][:2]])
    b = _arr([_dec(proof["pi_b"][0][0]), _dec(proof["pi_b"][0][1]), _dec(proof["pi_b"][1][0]), _dec(proof["pi_b"][1][1])])
    c = _arr([_dec(x) for x in proof["pi_c"][:2]])
    pub = _arr([_dec(x) for x in public[:n_pub]]) if n_pub else np.zeros((1, 4), dtype=np.uint64)
    rc = chk.p29_verify(_p(alpha), _p(beta), _p(gamma), _p(delta), _p(ic), n_pub, _p(pub), _p(a), _p(b), _p(c))
    assert chk.p29_last_failure().decode() == ""
    return rc


def test_multi_miller_verifier_agrees_with_host(chk, K, S):
    keyarrs = _vk_arrays(S)
    g, vkj = keyarrs[0], keyarrs[1]
    host = lambda pr, pu: K.lib().groth16_verify_json(json.dumps(pr).encode(), json.dumps(pu).encode(), vkj.encode())
    for c in g["cases"]:
        proof, public = c["proof"], c["public"]
        assert _verify29(chk, keyarrs, proof, public) == 1 == host(proof, public)
        flipped = [str(int(public[0]) ^ 1)] + public[1:]
        assert _verify29(chk, keyarrs, proof, flipped) == 0 == host(proof, flipped)
        swapped = dict(proof, pi_a=proof["pi_c"], pi_c=proof["pi_a"])
        assert _verify29(chk, keyarrs, swapped, public) == 0 == host(swapped, public)
        ident = dict(proof, pi_a=["0", "0", "0"])
        assert _verify29(chk, keyarrs, ident, public) == host(ident, public) == 0
    # the other case's public signals: the same statement, still accepted
    assert _verify29(chk, keyarrs, g["cases"][0]["proof"], g["cases"][1]["public"]) == 1


def test_g2_subgroup_check(chk, K):
    g2 = K.ec("g2", "generator")
    Qp = K.ec("g2", "to_affine", K.ec("g2", "mul_scalar", g2, 12345))
    assert chk.p29_g2_in_subgroup(_p(np.ascontiguousarray(Qp))) == 1
    # a twist point outside the order-r subgroup: x = 1, 2, … until x³ + 3/ξ is a square (as in test_verify.py)
    def f2mul(a, b):
        return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)

    def f2sqrt(a):
        n = (a[0] * a[0] + a[1] * a[1]) % Q
        sn = pow(n, (Q + 1) // 4, Q)
        if sn * sn % Q != n:
            return None
        for sgn in (1, -1):
            t = (a[0] + sgn * sn) * pow(2, -1, Q) % Q
            x0 = pow(t, (Q + 1) // 4, Q)
            if x0 * x0 % Q == t and x0:
                x1 = a[1] * pow(2 * x0, -1, Q) % Q
                if f2mul((x0, x1), (x0, x1)) == (a[0] % Q, a[1] % Q):
                    return (x0, x1)
        return None
    d = pow(82, -1, Q)
    bt = f2mul((3, 0), (9 * d % Q, -d % Q))
    for x0 in range(1, 50):
        rhs = f2mul(f2mul((x0, 0), (x0, 0)), (x0, 0))
        y = f2sqrt(((rhs[0] + bt[0]) % Q, (rhs[1] + bt[1]) % Q))
        if y:
            break
    pt = _arr([x0, 0, y[0], y[1]])
    assert chk.p29_g2_in_subgroup(_p(pt)) == 0
    assert chk.p29_last_failure().decode() == ""


# ---- the discrete-log case table (tests/groth16_dlog_model.py): verdicts from integers mod r, no pairing -------------------------
# Keys with 0, 2, 3, 8 and 40 public signals, and keys that reach the verifier's rare branches: IC₂ = ±IC₁ with equal signals
# (Straus doubles at the top set bit / cancels at every set bit), an identity ICⱼ (ic_zero), IC₀ = O, IC₀ = ±Σ sⱼ·ICⱼ₊₁ (the final
# addition doubles / cpub = O), γ₂ = O and δ₂ = O (use_gamma / use_delta = 0), α₁ = O and β₂ = O (target 1).  Per key and signal
# vector: a valid proof, c off by one, A = O, B = O, C = O, −A, a signal ±1, two signals swapped, pi_b outside the subgroup.


@pytest.fixture(scope="module")
def dlog(O):
    table = M.case_table()
    pts = M.Points(O)
    pts.need_items([it for _, items in table for it in items])
    pts.need("g1", [M.cpub_dlog(it.key, it.signals) for _, items in table for it in items])
    pts.resolve()
    return table, pts


def _key_arrays(pts, key):
    n = key.n_public
    return (_arr(pts.g1(key.alpha)), _arr(pts.g2(key.beta)), _arr(pts.g2(key.gamma)), _arr(pts.g2(key.delta)),
            _arr([v for k in key.ic[:n + 1] for v in pts.g1(k)]))


def _strided(items, n):
    """signal j of item k at [j·m + k], as verify_batch_kernel reads them"""
    return _arr([it.signals[j] for j in range(n) for it in items]) if n else np.zeros((1, 4), dtype=np.uint64)


def test_dlog_table_verdicts_equal_the_model(chk, dlog):
    table, pts = dlog
    bad, total = [], 0
    for key, items in table:
        items = [it for it in items if not it.json_only]  # a signal ≥ r never gets past the parser
        assert {0, 1} <= {it.want for it in items}, key.name
        m = len(items)
        a = _arr([v for it in items for v in pts.g1(it.proof.a)])
        b = _arr([v for it in items for v in (M.twist_point_outside_subgroup() if it.proof.b_outside else pts.g2(it.proof.b))])
        c = _arr([v for it in items for v in pts.g1(it.proof.c)])
        out = np.zeros(m, dtype=np.int32)
        chk.p29_verify_batch(*[_p(x) for x in _key_arrays(pts, key)], key.n_public, m, _p(_strided(items, key.n_public)),
                             _p(a), _p(b), _p(c), _p(out))
        assert chk.p29_last_failure().decode() == "", key.name
        bad += [(it.label, int(v), it.want) for it, v in zip(items, out) if v != it.want]
        total += m
    assert not bad, bad
    assert total > 200


def test_dlog_table_public_input_equals_the_model(chk, dlog):
    """public_input's Straus sum point for point against cpub = (ic₀ + Σ sⱼ·icⱼ₊₁)·G₁, cpub = O reported as such.  Verdicts cannot
    see that last flag: lines evaluated at (0, 0) are c·v·w, which the final exponentiation maps to 1."""
    table, pts = dlog
    for key, items in table:
        items = [it for it in items if not it.json_only]
        m = len(items)
        found = np.zeros(m, dtype=np.int32)
        xy = np.zeros((2 * m, 4), dtype=np.uint64)
        chk.p29_public_input(_p(_key_arrays(pts, key)[4]), key.n_public, m, _p(_strided(items, key.n_public)), _p(found), _p(xy))
        assert chk.p29_last_failure().decode() == "", key.name
        for k, it in enumerate(items):
            want = pts.g1(M.cpub_dlog(key, it.signals))
            if not any(want):
                assert found[k] == 0, it.label
            else:
                assert found[k] == 1 and _ints(xy[2 * k:2 * k + 2]) == list(want), it.label
    assert any(not any(pts.g1(M.cpub_dlog(k, it.signals))) for k, items in table for it in items)  # cpub = O was reached
