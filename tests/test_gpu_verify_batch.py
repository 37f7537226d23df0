"""Batched Groth16 verification on the GPU (groth16_verify_batch) and its pairing primitive (icicle_snark_pairing_batch):
bit-for-bit against the host pairing, verdict for verdict against the host verifier groth16_verify_json."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden, unhex

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R_ORDER = 21888242871839275222246405745257275088548364400416034343698204186575808495617

pytestmark = pytest.mark.gpu


def _arr(ints):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in ints), dtype=np.uint64).reshape(-1, 4).copy()


def _ints(a):
    return [int.from_bytes(r.tobytes(), "little") for r in np.asarray(a).reshape(-1, 4)]


def _host_verdict(K, pj, qj, vkj):
    return K.lib().groth16_verify_json(pj.encode(), qj.encode(), vkj.encode())


@pytest.fixture(scope="module")
def golden(S):
    from test_verify import _golden_vk_json
    g, vkj = _golden_vk_json(S)
    return g, vkj


# ---- group helpers on the host FFI (standard-form affine numpy arrays ↔ snarkjs JSON points) -------------------------------
def _g1_json(K, P):
    x, y = _ints(K.ec("g1", "to_affine", P))
    return [str(x), str(y), "1"] if (x or y) else ["0", "0", "0"]


def _g2_json(K, P):
    x0, x1, y0, y1 = _ints(K.ec("g2", "to_affine", P))
    return [[str(x0), str(x1)], [str(y0), str(y1)], ["1", "0"]]


def _g1_proj(K, pt):
    return K.ec("g1", "from_affine", _arr([int(pt[0]), int(pt[1])]))


def _g2_proj(K, pt):
    return K.ec("g2", "from_affine", _arr([int(pt[0][0]), int(pt[0][1]), int(pt[1][0]), int(pt[1][1])]))


def _rerandomise(K, proof, delta2, theta, rho):
    """A' = θ⁻¹·A, B' = θ·B + ρ·δ₂, C' = C + ρ·A': another valid proof of the same statement"""
    A, B, C = _g1_proj(K, proof["pi_a"]), _g2_proj(K, proof["pi_b"]), _g1_proj(K, proof["pi_c"])
    A2 = K.ec("g1", "mul_scalar", A, pow(theta, -1, R_ORDER))
    B2 = K.ec("g2", "ecadd", K.ec("g2", "mul_scalar", B, theta), K.ec("g2", "mul_scalar", delta2, rho))
    C2 = K.ec("g1", "ecadd", C, K.ec("g1", "mul_scalar", A2, rho))
    return dict(proof, pi_a=_g1_json(K, A2), pi_b=_g2_json(K, B2), pi_c=_g1_json(K, C2))


def _non_subgroup_twist_point():
    """a point ON the twist but outside the order-r subgroup (as tests/test_verify.py builds it)"""
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
            return [[str(x0), "0"], [str(y[0]), str(y[1])], ["1", "0"]]
    raise AssertionError("no twist point found")


# ---- pairing primitive ----------------------------------------------------------------------------------------------------
def test_pairing_batch_matches_host_pairing(gpu):
    K = gpu
    Ps, Qs = [], []
    for c in load_golden("pairing.json")["cases"]:
        Ps.append(unhex(c["p"], 2, 4))
        Qs.append(unhex(c["q"], 4, 4))
    rnd = random.Random(4242)
    g1, g2 = K.ec("g1", "generator"), K.ec("g2", "generator")
    sa = [rnd.randrange(1, R_ORDER) for _ in range(200)]
    sb = [rnd.randrange(1, R_ORDER) for _ in range(200)]
    Ps += list(K.generator_mul("g1", _arr(sa)).reshape(-1, 2, 4))
    Qs += list(K.generator_mul("g2", _arr(sb)).reshape(-1, 4, 4))
    zp, zq = np.zeros((2, 4), dtype=np.uint64), np.zeros((4, 4), dtype=np.uint64)
    for k in (3, 50, 120):  # identity pairs mixed in
        Ps.insert(k, zp)
        Qs.insert(k, Qs[k])
        Ps.insert(k + 1, Ps[k + 2])
        Qs.insert(k + 1, zq)
    P, Qa = np.stack(Ps), np.stack(Qs)
    got = K.pairing_batch(P, Qa)
    assert got.shape == (len(P), 12, 4)
    for i in range(len(P)):
        assert np.array_equal(got[i], K.pairing(P[i], Qa[i])), i
    assert np.array_equal(K.pairing_batch(P[:0], Qa[:0]), np.zeros((0, 12, 4), dtype=np.uint64))


# ---- verdicts -------------------------------------------------------------------------------------------------------------
def test_mixed_batch_verdicts_equal_host(gpu, golden, S):
    K = gpu
    g, vkj = golden
    vk = json.loads(vkj)
    delta2 = _g2_proj(K, vk["vk_delta_2"])
    c0, c1 = g["cases"]
    items = []
    rnd = random.Random(64)
    for c in (c0, c1):
        items.append((c["proof"], c["public"]))
        items.append((_rerandomise(K, c["proof"], delta2, rnd.randrange(1, R_ORDER), rnd.randrange(R_ORDER)), c["public"]))
    p, pub = c0["proof"], c0["public"]
    bad = json.loads(json.dumps(p)); bad["pi_a"][1] = str((int(bad["pi_a"][1]) + 1) % Q); items.append((bad, pub))      # off the curve
    bad = json.loads(json.dumps(p)); bad["pi_c"][0] = str(int(bad["pi_c"][0]) + Q); items.append((bad, pub))            # not canonical
    items.append((dict(p, pi_a=p["pi_c"], pi_c=p["pi_a"]), pub))                                                           # swapped A / C
    items.append((p, [str(int(pub[0]) ^ 1)] + pub[1:]))                                                                     # flipped signal
    items.append((p, [str(int(pub[0]) + R_ORDER)] + pub[1:]))                                                               # ≥ r (aliasing)
    bad = json.loads(json.dumps(p)); bad["pi_b"][0][0] = str((int(bad["pi_b"][0][0]) + 1) % Q); items.append((bad, pub))  # off the twist
    items.append((dict(p, pi_b=_non_subgroup_twist_point()), pub))                                                         # outside the subgroup
    items.append((dict(p, pi_a=["0", "0", "0"]), pub))                                                                      # identity A
    items.append((dict(p, pi_b=[["0", "0"], ["0", "0"], ["0", "0"]]), pub))                                                # identity B
    items.append((c0["proof"], c1["public"]))                                                                               # other case's signals
    texts = [(json.dumps(a), json.dumps(b)) for a, b in items]
    texts.append((json.dumps(p)[:-3], json.dumps(pub)))                                                                     # malformed JSON
    texts.append((json.dumps(p), "[1, 2"))
    texts.append((json.dumps(p), json.dumps([])))                                                                           # too few signals
    texts.append((json.dumps(p), json.dumps([int(pub[0])])))                                                               # not a string
    while len(texts) < 64:
        texts.append(texts[len(texts) % 17])
    want = [_host_verdict(K, a, b, vkj) for a, b in texts]
    got = K.groth16_verify_batch([a for a, _ in texts], [b for _, b in texts], vkj)
    assert got == want
    assert set(want) == {1, 0, -2}
    # a valid proof paired with another statement's public signals is rejected
    other = [str((int(pub[0]) * 7 + 5) % R_ORDER)] + pub[1:]
    assert K.groth16_verify_batch([json.dumps(p)], [json.dumps(other)], vkj) == [0] == [_host_verdict(K, json.dumps(p), json.dumps(other), vkj)]


def test_batch_of_4096_known_verdicts(gpu, golden):
    K = gpu
    g, vkj = golden
    vk = json.loads(vkj)
    delta2 = _g2_proj(K, vk["vk_delta_2"])
    rnd = random.Random(4096)
    distinct = []
    for k in range(256):
        c = g["cases"][k % 2]
        distinct.append((json.dumps(_rerandomise(K, c["proof"], delta2, rnd.randrange(1, R_ORDER), rnd.randrange(R_ORDER))), json.dumps(c["public"])))
    proofs = [distinct[i % 256][0] for i in range(4096)]
    publics = [distinct[i % 256][1] for i in range(4096)]
    want = [1] * 4096
    for i in rnd.sample(range(4096), 300):
        pr = json.loads(proofs[i])
        kind = i % 3
        if kind == 0:
            pu = json.loads(publics[i])
            publics[i] = json.dumps([str(int(pu[0]) ^ 2)] + pu[1:])
            want[i] = 0
        elif kind == 1:
            pr["pi_c"] = pr["pi_a"]
            proofs[i] = json.dumps(pr)
            want[i] = 0
        else:
            proofs[i] = proofs[i][:-1]
            want[i] = -2
    got = K.groth16_verify_batch(proofs, publics, vkj)
    assert got == want
    for i in rnd.sample(range(4096), 32):
        assert _host_verdict(K, proofs[i], publics[i], vkj) == want[i]
    parse_ms, dev_ms = K.groth16_verify_batch_last_timings()
    assert parse_ms > 0 and dev_ms > 0


def test_real_proofs_from_the_prover_accepted(gpu, S, O):
    K = gpu
    r1, w = S.squaring_chain(300)
    zkey, vk = S.setup(r1, lambda g, k: K.generator_mul(g, k), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
    wtns = S.write_wtns(w)
    cm = K.CacheManager()
    try:
        cm.load("vb", zkey)
        proofs = [cm.prove_mem("vb", wtns, 3 + i, 5 + 2 * i)[:2] for i in range(6)]
    finally:
        cm.close()
        K.release_domain()
    vkj = S.vk_to_json(vk)
    got = K.groth16_verify_batch([p for p, _ in proofs], [q for _, q in proofs], vkj)
    assert got == [1] * 6
    assert all(_host_verdict(K, p, q, vkj) == 1 for p, q in proofs)


def test_edges(gpu, golden, S):
    K = gpu
    g, vkj = golden
    p, pub = json.dumps(g["cases"][0]["proof"]), json.dumps(g["cases"][0]["public"])
    assert K.groth16_verify_batch([], [], vkj) == []
    assert K.groth16_verify_batch([p], [pub], vkj) == [1]
    assert K.groth16_verify_batch([p] * 70, [pub] * 70, vkj, device="HIP:0") == [1] * 70
    # a verification key with nPublic = 0: the golden key's IC₁·pub₀ folded into IC₀ gives a key that accepts with no signals
    vk = json.loads(vkj)
    ic0 = _g1_proj(K, vk["IC"][0])
    ic1 = _g1_proj(K, vk["IC"][1])
    folded = K.ec("g1", "ecadd", ic0, K.ec("g1", "mul_scalar", ic1, int(json.loads(pub)[0])))
    vk0 = dict(vk, IC=[_g1_json(K, folded)], nPublic=0)
    vk0j = json.dumps(vk0)
    assert len(json.loads(pub)) == 1
    assert K.groth16_verify_batch([p, p], ["[]", pub], vk0j) == [1, 1] == [_host_verdict(K, p, "[]", vk0j), _host_verdict(K, p, pub, vk0j)]
    # key errors: < 0 with the text in groth16_verify_last_error()
    with pytest.raises(K.ProverError, match="malformed JSON"):
        K.groth16_verify_batch([p], [pub], vkj[:-2])
    bad = dict(vk, nPublic="x")
    with pytest.raises(K.ProverError, match="nPublic"):
        K.groth16_verify_batch([p], [pub], json.dumps(bad))
    with pytest.raises(K.ProverError, match="one device"):
        K.groth16_verify_batch([p], [pub], vkj, device="HIP:0-1")


def test_cli_verify_batch(gpu, golden, tmp_path):
    g, vkj = golden
    exe = os.path.join(ROOT, "icicle-snark_amd", "lib", "prove")
    lines = []
    for k, c in enumerate(g["cases"]):
        (tmp_path / f"p{k}.json").write_text(json.dumps(c["proof"]))
        (tmp_path / f"q{k}.json").write_text(json.dumps(c["public"]))
        lines.append(f"{tmp_path}/p{k}.json {tmp_path}/q{k}.json")
    (tmp_path / "bad.json").write_text(json.dumps(["1"]))
    lines.append(f"{tmp_path}/p0.json {tmp_path}/bad.json")
    lines.append(f"{tmp_path}/p0.json {tmp_path}/missing.json")
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    (tmp_path / "vk.json").write_text(vkj)
    cmds = f"verify-batch --list {tmp_path}/list.txt --vk {tmp_path}/vk.json --device HIP\nexit\n"
    out = subprocess.run([exe], input=cmds, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = [ln.replace("> ", "") for ln in out.stdout.splitlines()]
    assert got[:6] == ["0 accepted", "1 accepted", "2 rejected", "3 error: cannot read input file",
                       "accepted 2 rejected 1 errors 1", "COMMAND_COMPLETED"], out.stdout
