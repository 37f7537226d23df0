"""Checked host build of what the combined batch verifier (groth16_verify_batch_combined) adds to csrc/pairing29.h: the
endomorphism subgroup test, the 128-bit lane multiplication, the Miller product and the whole combined decision, compiled here
with g++ -DF29_CHECK (every lazy bound a recorded failure) and compared with the existing [r]·Q test, big-integer curve
arithmetic written here, the CPU oracle, the library's host pairing and the discrete-log model (tests/groth16_dlog_model.py).
Also the integer argument for the subgroup test's soundness, and the coefficient derivation against hashlib.  No GPU."""
import ctypes as C
import hashlib
import math
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import groth16_dlog_model as M

Q = M.Q
R_ORDER = M.R
X_BN = 4965661367192848881


@pytest.fixture(scope="module")
def chk():
    out = os.path.join(ROOT, "build", "pairing29_combined_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "pairing29_combined_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-DF29_CHECK", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc"), "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.p29c_last_failure.restype = C.c_char_p
    lib.p29c_reset()
    yield lib
    assert lib.p29c_last_failure().decode() == "", "F29_CHECK bound fired"


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _arr(ints):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in ints), dtype=np.uint64).reshape(-1, 4).copy()


def _ints(a):
    return [int.from_bytes(r.tobytes(), "little") for r in np.asarray(a).reshape(-1, 4)]


# ---- the twist E′: y² = x³ + 3/ξ over F_q², affine, with Python integers (None = the identity) -------------------------------
def _f2(a, b=0):
    return (a % Q, b % Q)


def _f2add(a, b):
    return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)


def _f2sub(a, b):
    return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)


_f2mul = M._f2mul


def _f2inv(a):
    d = pow(a[0] * a[0] + a[1] * a[1], -1, Q)
    return (a[0] * d % Q, -a[1] * d % Q)


def _tw_add(P, S):
    if P is None:
        return S
    if S is None:
        return P
    (x1, y1), (x2, y2) = P, S
    if x1 == x2:
        if _f2add(y1, y2) == (0, 0):
            return None
        lam = _f2mul(_f2mul(_f2(3), _f2mul(x1, x1)), _f2inv(_f2add(y1, y1)))
    else:
        lam = _f2mul(_f2sub(y2, y1), _f2inv(_f2sub(x2, x1)))
    x3 = _f2sub(_f2sub(_f2mul(lam, lam), x1), x2)
    return (x3, _f2sub(_f2mul(lam, _f2sub(x1, x3)), y1))


def _tw_mul(k, P):
    acc = None
    for bit in bin(k)[2:]:
        acc = _tw_add(acc, acc)
        if bit == "1":
            acc = _tw_add(acc, P)
    return acc


def _twist_points_outside(count):
    """twist points off the order-r subgroup: x = 1, 2, … as groth16_dlog_model.twist_point_outside_subgroup, all of them"""
    d = pow(82, -1, Q)
    bt = _f2mul((3, 0), (9 * d % Q, -d % Q))
    out, x0 = [], 0
    while len(out) < count:
        x0 += 1
        rhs = _f2mul(_f2mul((x0, 0), (x0, 0)), (x0, 0))
        y = M._f2sqrt(((rhs[0] + bt[0]) % Q, (rhs[1] + bt[1]) % Q))
        if y:
            out.append(((x0, 0), y))
    return out


def _both(chk, P):
    r = chk.p29c_g2_subgroup_both(_p(_arr([P[0][0], P[0][1], P[1][0], P[1][1]])))
    assert chk.p29c_last_failure().decode() == ""
    return r & 1, (r >> 1) & 1


def test_fast_subgroup_test_equals_the_plain_one(chk, O):
    pts = M.Points(O)
    rnd = random.Random(63)
    ks = [1, 2, 3, X_BN, X_BN + 1, 2 * X_BN, R_ORDER - 1, 12345] + [rnd.randrange(1, R_ORDER) for _ in range(12)]
    pts.need("g2", ks)
    pts.resolve()
    g2 = lambda k: ((pts.g2(k)[0], pts.g2(k)[1]), (pts.g2(k)[2], pts.g2(k)[3]))
    for k in ks:                                   # subgroup points
        assert _both(chk, g2(k)) == (1, 1), k
    outside = _twist_points_outside(20)
    t = 6 * X_BN * X_BN + 1
    h2 = Q - 1 + t
    assert _tw_mul(R_ORDER * h2, outside[0]) is None  # #E′(F_q²) = r·h₂
    for T in outside:                              # twist points outside the subgroup
        assert _tw_mul(R_ORDER, T) is not None
        assert _both(chk, T) == (0, 0), T[0]
    for T in outside[:6]:                          # pure-cofactor points r·T (order divides h₂) and sums T + k·G₂, r·T + k·G₂
        rT = _tw_mul(R_ORDER, T)
        assert _both(chk, rT) == (0, 0), T[0]
        k = rnd.choice(ks)
        assert _both(chk, _tw_add(T, g2(k))) == (0, 0)
        assert _both(chk, _tw_add(rT, g2(k))) == (0, 0)
        hT = _tw_mul(h2, T)                        # cofactor-cleared: back in the subgroup
        assert _tw_mul(R_ORDER, hT) is None and _both(chk, hT) == (1, 1)


def test_fast_subgroup_test_is_sound_by_integers():
    """ψ satisfies X² − tX + q on E′(F_q²) and acts as q on G2.  P(X) = (x+1) + xX + xX² − 2xX³ reduced modulo that polynomial is
    a + bX; its norm N = a² + abt + b²q is the determinant of P(ψ) on the (rank-2) group, so #ker P(ψ) divides what N shares with
    the group order r·h₂.  gcd(N, r·h₂) = r and gcd(N, h₂) = 1: the kernel has order dividing r.  P(q) ≡ 0 mod r: G2 lies in the
    kernel.  Hence the kernel is exactly G2."""
    x = X_BN
    q, r = Q, R_ORDER
    assert q == 36 * x**4 + 36 * x**3 + 24 * x**2 + 6 * x + 1 and r == 36 * x**4 + 36 * x**3 + 18 * x**2 + 6 * x + 1
    t = 6 * x * x + 1
    h2 = q - 1 + t
    assert r == q + 1 - t and r * h2 == (q + 1 - t) * (q - 1 + t)  # #E′(F_q²) = #E(F_q)·h₂
    # reduce P modulo X² − tX + q:  X² = tX − q,  X³ = (t² − q)X − tq
    c0, c1, c2, c3 = x + 1, x, x, -2 * x
    a = c0 - c2 * q - c3 * t * q
    b = c1 + c2 * t + c3 * (t * t - q)
    N = a * a + a * b * t + b * b * q
    assert N != 0
    assert math.gcd(N, r * h2) == r
    assert math.gcd(N, h2) == 1
    assert (c0 + c1 * q + c2 * q * q + c3 * q**3) % r == 0
    assert (q * q - t * q + q) % r == 0          # q is a root of the characteristic polynomial mod r: ψ = [q] on G2


def test_lane_multiplication_agrees_with_the_oracle(chk, O):
    rnd = random.Random(128)
    pts = M.Points(O)
    zs = [1, 2, 1 << 127, (1 << 128) - 1] + [rnd.randrange(1, 1 << 128) for _ in range(8)]
    avals = [1, 2, R_ORDER - 1] + [rnd.randrange(1, R_ORDER) for _ in range(3)]
    pts.need("g1", avals + [-z * a for z in zs for a in avals])
    pts.resolve()
    for a in avals:
        for z in zs:
            out = np.zeros((2, 4), dtype=np.uint64)
            zw = np.frombuffer(z.to_bytes(16, "little"), dtype=np.uint32).copy()
            got = chk.p29c_lane_mul(_p(_arr(pts.g1(a))), _p(zw), _p(out))
            assert chk.p29c_last_failure().decode() == ""
            want = pts.g1(-z * a)
            assert (got == 1 and tuple(_ints(out)) == want) if any(want) else got == 0, (a, z)


def test_miller_product_equals_the_product_of_host_pairings(chk, K, O):
    rnd = random.Random(6365)
    pts = M.Points(O)
    ab = [(rnd.randrange(1, R_ORDER), rnd.randrange(1, R_ORDER)) for _ in range(65)]
    pts.need("g1", [a for a, _ in ab])
    pts.need("g2", [b for _, b in ab])
    pts.resolve()
    P = [pts.g1(a) for a, _ in ab]
    Qs = [pts.g2(b) for _, b in ab]
    for k in (5, 40):
        P[k] = (0, 0)
    for k in (6, 63):
        Qs[k] = (0, 0, 0, 0)
    one = np.zeros((12, 4), dtype=np.uint64)
    one[0, 0] = 1
    each = [K.pairing(_arr(P[i]), _arr(Qs[i])) for i in range(65)]
    assert np.array_equal(each[5], one) and np.array_equal(each[63], one)
    for k in (1, 2, 63, 65):
        want = one
        for i in range(k):
            want = K.gt_op("mul", want, each[i])
        out = np.zeros((12, 4), dtype=np.uint64)
        chk.p29c_pairing_product(_p(_arr([v for p in P[:k] for v in p])), _p(_arr([v for q in Qs[:k] for v in q])), k, _p(out))
        assert chk.p29c_last_failure().decode() == ""
        assert np.array_equal(out, want), k
    out = np.zeros((12, 4), dtype=np.uint64)
    chk.p29c_pairing_product(_p(_arr([0, 0])), _p(_arr([0, 0, 0, 0])), 0, _p(out))
    assert np.array_equal(out, one)


# ---- the combined decision over the discrete-log case table ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dlog(O):
    table = M.case_table()
    pts = M.Points(O)
    pts.need_items([it for _, items in table for it in items])
    pts.resolve()
    return table, pts


def _combined(chk, pts, key, items, seed, index=None):
    n, m = key.n_public, len(items)
    keyarrs = (_arr(pts.g1(key.alpha)), _arr(pts.g2(key.beta)), _arr(pts.g2(key.gamma)), _arr(pts.g2(key.delta)),
               _arr([v for k in key.ic[:n + 1] for v in pts.g1(k)]))
    pub = _arr([it.signals[j] for it in items for j in range(n)]) if n else np.zeros((1, 4), dtype=np.uint64)
    a = _arr([v for it in items for v in pts.g1(it.proof.a)])
    b = _arr([v for it in items for v in (M.twist_point_outside_subgroup() if it.proof.b_outside else pts.g2(it.proof.b))])
    c = _arr([v for it in items for v in pts.g1(it.proof.c)])
    idx = np.array(index if index is not None else list(range(m)), dtype=np.uint64)
    rc = chk.p29c_combined(*[_p(x) for x in keyarrs], n, m, _p(pub), _p(a), _p(b), _p(c), seed, _p(idx))
    assert chk.p29c_last_failure().decode() == "", key.name
    return rc


def test_combined_decision_over_the_dlog_table(chk, dlog):
    """for every key of the table: each all-valid subset tried is accepted (all valid items, each alone, random subsets, repeated
    items), each subset with exactly one model-invalid item is rejected, a pi_b outside the subgroup is reported as such"""
    table, pts = dlog
    rnd = random.Random(0xc0b1)
    seed = bytes(rnd.randrange(256) for _ in range(32))
    labels = set()
    for key, items in table:
        items = [it for it in items if not it.json_only]
        valid = [it for it in items if it.want == 1]
        invalid = [it for it in items if it.want == 0]
        outside = [it for it in items if it.want == -2]
        assert valid and invalid and outside, key.name
        assert _combined(chk, pts, key, valid, seed) == 1, key.name
        twice = valid + valid[:2]
        assert _combined(chk, pts, key, twice, seed, index=[7 * k + 3 for k in range(len(twice))]) == 1, key.name
        for it in valid:
            assert _combined(chk, pts, key, [it], seed) == 1, it.label
            labels.add(it.label.split(" ")[-1])
        for _ in range(2):
            sub = rnd.sample(valid, rnd.randrange(1, len(valid) + 1))
            assert _combined(chk, pts, key, sub, bytes(rnd.randrange(256) for _ in range(32))) == 1, key.name
        for it in invalid:
            mates = rnd.sample(valid, min(2, len(valid)))
            batch = mates + [it]
            rnd.shuffle(batch)
            assert _combined(chk, pts, key, batch, seed) == 0, it.label
            assert _combined(chk, pts, key, [it], seed) == 0, it.label
        assert _combined(chk, pts, key, valid[:1] + outside[:1], seed) == -1, key.name
    # the edge cases took part as valid items: identity A / B / C, and the keys named in the table
    assert {"A=O", "B=O", "C=O"} <= labels
    assert {"gamma=0", "delta=0", "alpha=0", "beta=0", "ic0=-sum", "ic0=O"} <= {key.name for key, _ in table}


def test_unweighted_cancellations_are_rejected(chk, dlog):
    """two proofs whose errors cancel in an unweighted product (c + 1 and c − 1; public-signal vectors exchanged between two
    statements) are rejected under every seed tried"""
    table, pts = dlog
    rnd = random.Random(77)
    key = next(k for k, _ in table if k.name == "n=3")
    sig1 = [rnd.randrange(R_ORDER) for _ in range(3)]
    sig2 = [rnd.randrange(R_ORDER) for _ in range(3)]
    a, b = rnd.randrange(1, R_ORDER), rnd.randrange(1, R_ORDER)
    plus = M.Item(key, M.prove(key, sig1, a, b, e=1), sig1, "c+1")
    minus = M.Item(key, M.prove(key, sig1, a + 5, b + 9, e=R_ORDER - 1), sig1, "c-1")
    # exchanged signals: with equal A, B the γ terms of the two items swap places, so the unweighted product is unchanged
    p1, p2 = M.prove(key, sig1, a, b), M.prove(key, sig2, a + 1, b + 1)
    x1, x2 = M.Item(key, p1, sig2, "p1 with sig2"), M.Item(key, p2, sig1, "p2 with sig1")
    assert plus.want == minus.want == x1.want == x2.want == 0
    ok = M.Item(key, p1, sig1, "valid")
    pts.need_items([plus, minus, x1, x2, ok])
    pts.resolve()
    for s in range(3):
        seed = hashlib.sha256(b"cancel%d" % s).digest()
        assert _combined(chk, pts, key, [plus, minus], seed) == 0
        assert _combined(chk, pts, key, [x1, x2], seed) == 0
        assert _combined(chk, pts, key, [ok, plus, minus], seed) == 0
        assert _combined(chk, pts, key, [ok], seed) == 1


# ---- coefficients -----------------------------------------------------------------------------------------------------------------
def _z(seed, i):
    v = int.from_bytes(hashlib.sha256(seed + i.to_bytes(8, "little")).digest(), "little") & ((1 << 128) - 1)
    return v or 1


def test_coefficients_equal_the_hashlib_construction(chk):
    for seed in (bytes(32), bytes(range(32)), hashlib.sha256(b"seed").digest(), b"\xff" * 32):
        for first, count in ((0, 5), (63, 3), (1 << 16, 4), ((1 << 32) - 2, 4), ((1 << 64) - 3, 3)):
            out = (C.c_uint8 * (16 * count))()
            chk.p29c_coefficients(seed, C.c_uint64(first), C.c_uint64(count), out)
            got = [int.from_bytes(bytes(out)[16 * k:16 * k + 16], "little") for k in range(count)]
            assert got == [_z(seed, first + k) for k in range(count)], (seed[:2], first)
    # the hash itself on lengths around its block boundaries
    for n in (0, 1, 40, 55, 56, 63, 64, 65, 119, 120, 200):
        msg = bytes((7 * k + n) & 255 for k in range(n))
        out = (C.c_uint8 * 32)()
        chk.p29c_sha256(msg, C.c_uint64(n), out)
        assert bytes(out) == hashlib.sha256(msg).digest(), n
    # 0 is replaced by 1 (no seed is known to reach it: the rule is exercised on a made-up digest)
    out = (C.c_uint8 * 16)()
    chk.p29c_coefficient_from_digest(bytes(16) + b"\x55" * 16, out)
    assert int.from_bytes(bytes(out), "little") == 1
    chk.p29c_coefficient_from_digest(bytes(15) + b"\x80" + b"\x55" * 16, out)
    assert int.from_bytes(bytes(out), "little") == 1 << 127


def test_library_exports_the_same_coefficients(K):
    seed = hashlib.sha256(b"library").digest()
    assert K.verify_combined_coefficients(seed, 0, 6) == [_z(seed, i) for i in range(6)]
    assert K.verify_combined_coefficients(seed, (1 << 40) + 5, 3) == [_z(seed, (1 << 40) + 5 + i) for i in range(3)]
    assert all(0 < z < 1 << 128 for z in K.verify_combined_coefficients(bytes(32), 0, 50))
