"""Batched Groth16 verification on the GPU (groth16_verify_batch) and its pairing primitive (icicle_snark_pairing_batch):
bit-for-bit against the host pairing and against bilinearity, verdict for verdict against the host verifier groth16_verify_json
and a discrete-log model of the verification equation (tests/groth16_dlog_model.py)."""
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
    x0, x1, y0, y1 = M.twist_point_outside_subgroup()
    return [[str(x0), str(x1)], [str(y0), str(y1)], ["1", "0"]]


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


# ---- the discrete-log case table (tests/groth16_dlog_model.py; tests/test_pairing29.py runs it through the checked header) --------
@pytest.fixture(scope="module")
def dlog(O):
    table = M.case_table()
    pts = M.Points(O)
    pts.need_items([it for _, items in table for it in items])
    pts.resolve()
    texts = [(M.vk_json(pts, key), [(M.proof_json(pts, it.proof), M.public_json(it.signals)) for it in items]) for key, items in table]
    return table, pts, texts


def test_dlog_table_verdicts_equal_model_and_host(gpu, dlog):
    """every item of the table: groth16_verify_batch = model = groth16_verify_json, in batches of 1, 63, 64, 65 and 300 of one key
    whose items (edge cases, valid and rejected) are shuffled together"""
    K = gpu
    table, _, texts = dlog
    sizes = (1, 63, 64, 65, 300)
    rnd = random.Random(6365)
    bad = []
    for t, ((key, items), (vkj, pq)) in enumerate(zip(table, texts)):
        for it, (pj, qj) in zip(items, pq):
            if _host_verdict(K, pj, qj, vkj) != it.want:
                bad.append(("host", it.label, it.want))
        for size in (sizes[t % 5], sizes[(t + 2) % 5]):
            idx = list(range(len(items))) + [rnd.randrange(len(items)) for _ in range(size - len(items))]
            rnd.shuffle(idx)
            for b in ([[k] for k in idx] if size == 1 else [idx]):
                got = K.groth16_verify_batch([pq[k][0] for k in b], [pq[k][1] for k in b], vkj)
                bad += [("gpu", size, items[k].label, g, items[k].want) for k, g in zip(b, got) if g != items[k].want]
    assert not bad, bad[:20]
    assert {it.want for _, items in table for it in items} == {1, 0, -2}


def test_real_prover_key_with_five_signals(gpu, S, O):
    """a prover key with nPublic = 5: its proofs are accepted, and each signal changed in turn is rejected, on the GPU and the host"""
    K = gpu
    r1, w = S.random_circuit(200, 5, 10, seed=55)
    zkey, vk = S.setup(r1, lambda g, k: K.generator_mul(g, k), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
    wtns = S.write_wtns(w)
    cm = K.CacheManager()
    try:
        cm.load("vb5", zkey)
        proofs = [cm.prove_mem("vb5", wtns, 7 + i, 11 + 3 * i)[:2] for i in range(4)]
    finally:
        cm.close()
        K.release_domain()
    vkj = S.vk_to_json(vk)
    assert json.loads(vkj)["nPublic"] == 5
    pub = json.loads(proofs[0][1])
    assert len(pub) == 5
    items = list(proofs)
    for j in range(5):
        changed = list(pub)
        changed[j] = str((int(pub[j]) + 1 + j) % R_ORDER)
        items.append((proofs[j % 4][0], json.dumps(changed)))
    want = [1] * 4 + [0] * 5
    assert K.groth16_verify_batch([p for p, _ in items], [q for _, q in items], vkj) == want
    assert [_host_verdict(K, p, q, vkj) for p, q in items] == want


# ---- the chunk boundary of groth16_verify_batch (CHUNK live proofs per launch, verify_batch.hip) ------------------------------
CHUNK = 1 << 16


@pytest.fixture(scope="module")
def pool3(O):
    """a key with nPublic = 3 and 251 proofs of it, each with its own random signals; every fourth is invalid (c off by one)"""
    rnd = random.Random(3333)
    key = M.random_key(rnd, 3, "n=3")
    items = []
    for k in range(251):
        sig = [rnd.randrange(R_ORDER) for _ in range(3)]
        items.append(M.Item(key, M.prove(key, sig, rnd.randrange(1, R_ORDER), rnd.randrange(1, R_ORDER), e=int(k % 4 == 3)), sig, f"pool {k}"))
    pts = M.Points(O)
    pts.need_items(items)
    pts.resolve()
    texts = [(M.proof_json(pts, it.proof), M.public_json(it.signals)) for it in items]
    assert {it.want for it in items} == {0, 1}
    return M.vk_json(pts, key), items, texts


def _tiled_batch(pool3, n, errors):
    """n items tiled from the pool; at the indices in `errors` a parse error (−2) of one of three kinds"""
    vkj, items, texts = pool3
    proofs = [texts[i % 251][0] for i in range(n)]
    publics = [texts[i % 251][1] for i in range(n)]
    want = [items[i % 251].want for i in range(n)]
    for t, i in enumerate(errors):
        p, q = json.loads(publics[i]), proofs[i]
        if t % 3 == 0:
            proofs[i] = q[:-2]                                                   # malformed JSON
        elif t % 3 == 1:
            publics[i] = json.dumps([p[0], str(int(p[1]) + R_ORDER), p[2]])      # a signal ≥ r at j = 1
        else:
            publics[i] = json.dumps(p[:2])                                       # too few signals
        want[i] = -2
    return proofs, publics, want


def test_chunk_boundary_with_gaps_in_the_live_list(gpu, pool3):
    """CHUNK + 4097 items with ~1 % parse errors before the boundary: the first launch takes the first CHUNK live items, the second
    a short chunk (m < cap) of distinct signal vectors, so the per-chunk signal layout pub[j·m + k] is exercised with m ≠ cap"""
    K = gpu
    vkj, items, texts = pool3
    n = CHUNK + 4097
    errors = [i for i in range(0, CHUNK, 97)]
    proofs, publics, want = _tiled_batch(pool3, n, errors)
    live = [i for i in range(n) if want[i] != -2]
    last1, first2 = live[CHUNK - 1], live[CHUNK]
    assert last1 > CHUNK - 1 and len(live) - CHUNK < CHUNK
    bad = next(k for k in range(251) if items[k].want == 0)
    for i in (last1, first2):  # rejected proofs on both sides of the boundary
        proofs[i], publics[i], want[i] = texts[bad][0], texts[bad][1], 0
    assert len({publics[i] for i in live[CHUNK:CHUNK + 251]}) >= 250
    got = K.groth16_verify_batch(proofs, publics, vkj)
    wrong = [(i, got[i], want[i]) for i in range(n) if got[i] != want[i]]
    assert not wrong, (len(wrong), wrong[:10], last1, first2)
    assert got[last1] == got[first2] == 0 and got[last1 - 1] == want[last1 - 1]
    sample = [0, errors[1], last1 - 1, last1, first2, first2 + 1, n - 1] + random.Random(7).sample(range(n), 57)
    assert [_host_verdict(K, proofs[i], publics[i], vkj) for i in sample] == [want[i] for i in sample]


def test_batch_of_exactly_one_chunk_of_live_items(gpu, pool3):
    K = gpu
    vkj, _, _ = pool3
    errors = list(range(5, CHUNK, 1311))
    proofs, publics, want = _tiled_batch(pool3, CHUNK + len(errors), errors)
    assert sum(v != -2 for v in want) == CHUNK
    got = K.groth16_verify_batch(proofs, publics, vkj)
    assert got == want
    sample = [0, len(want) - 1] + random.Random(8).sample(range(len(want)), 30)
    assert [_host_verdict(K, proofs[i], publics[i], vkj) for i in sample] == [want[i] for i in sample]


# ---- pairing_batch against bilinearity (no host pairing involved) ----------------------------------------------------------------
def _conj(e):
    """f^(p⁶) in bn254_pairing's basis: the six c1 coefficients negated mod q (= f⁻¹ for a pairing value)"""
    out = np.array(e, copy=True)
    c1 = _ints(e[6:12])
    out[6:12] = _arr([(Q - v) % Q for v in c1])
    return out


def test_pairing_batch_is_bilinear(gpu, O):
    K = gpu
    rnd = random.Random(2025)
    pts = M.Points(O)
    ab = [(rnd.randrange(1, R_ORDER), rnd.randrange(1, R_ORDER)) for _ in range(21)]
    pts.need("g1", [1] + [a for a, _ in ab] + [a * b for a, b in ab])
    pts.need("g2", [1] + [b for _, b in ab] + [a * b for a, b in ab])
    pts.resolve()
    P = [pts.g1(a) for a, _ in ab] + [pts.g1(a * b) for a, b in ab] + [pts.g1(1)] * 21
    Qs = [pts.g2(b) for _, b in ab] + [pts.g2(1)] * 21 + [pts.g2(a * b) for a, b in ab]
    got = K.pairing_batch(_arr([v for p in P for v in p]), _arr([v for q in Qs for v in q]))  # 63 lanes
    assert np.array_equal(got[:21], got[21:42]) and np.array_equal(got[:21], got[42:])
    one = np.zeros((12, 4), dtype=np.uint64)
    one[0, 0] = 1
    assert len({got[i].tobytes() for i in range(21)} | {one.tobytes()}) == 22  # 21 distinct values, none of them 1
    # e(−P, Q) = conj(e(P, Q))
    negP = [(x, (Q - y) % Q) for x, y in P[:21]]
    neg = K.pairing_batch(_arr([v for p in negP for v in p]), _arr([v for q in Qs[:21] for v in q]))
    for i in range(21):
        assert np.array_equal(neg[i], _conj(got[i])), i


def test_pairing_batch_edge_coordinates(gpu, O):
    """G₁ = (1, 2), −G₁ = (1, q − 2) and −k·G₁ (y = q − y(k·G₁)), each against e(G₁, ∓k·b·G₂), in batches of 1, 63 and 65"""
    K = gpu
    rnd = random.Random(1265)
    ks = [1, 2, 3, 4, 5, 6, 7, 8, 1000, R_ORDER - 1, R_ORDER - 2]
    pts = M.Points(O)
    b = [rnd.randrange(1, R_ORDER) for _ in ks]
    pts.need("g1", [1] + ks)
    pts.need("g2", b + [k * bb for k, bb in zip(ks, b)] + [-k * bb for k, bb in zip(ks, b)])
    pts.resolve()
    assert pts.g1(1) == (1, 2) and pts.g1(-1) == (1, Q - 2)
    pairs, rel = [], []  # rel: (i, j, conj): e_i = e_j, or e_i = conj(e_j)
    for k, bb in zip(ks, b):
        x, y = pts.g1(k)
        base = len(pairs)
        pairs += [((x, y), pts.g2(bb)), ((x, (Q - y) % Q), pts.g2(bb)), ((1, 2), pts.g2(k * bb)), ((1, 2), pts.g2(-k * bb))]
        rel += [(base, base + 2, False), (base + 1, base + 3, False), (base + 1, base, True)]
    P = _arr([v for p, _ in pairs for v in p])
    Qa = _arr([v for _, q in pairs for v in q])
    for size in (1, 63, 65):
        if size == 1:
            got = np.stack([K.pairing_batch(P[2 * i:2 * i + 2], Qa[4 * i:4 * i + 4])[0] for i in range(len(pairs))])
        else:  # the pairs repeated to fill the batch; lanes past the first copy must agree with it
            idx = [i % len(pairs) for i in range(size)]
            full = K.pairing_batch(P.reshape(-1, 2, 4)[idx], Qa.reshape(-1, 4, 4)[idx])
            for lane in range(len(pairs), size):
                assert np.array_equal(full[lane], full[lane % len(pairs)]), (size, lane)
            got = full[:len(pairs)]
        for i, j, cj in rel:
            assert np.array_equal(got[i], _conj(got[j]) if cj else got[j]), (size, i, j)
        assert not np.array_equal(got[0], got[1])
