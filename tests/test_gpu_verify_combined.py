"""Randomised batch verification on the GPU (groth16_verify_batch_combined) and its pairing-product primitive
(icicle_snark_pairing_product): verdict for verdict against groth16_verify_batch, the discrete-log model
(tests/groth16_dlog_model.py) and, for samples, the host verifier; `path` against the model; cancellation cases that an
unweighted product would accept; the chunk boundary; the product bit for bit against the host pairing."""
import hashlib
import json
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import groth16_dlog_model as M
from test_gpu_verify_batch import (CHUNK, R_ORDER, _arr, _g2_proj, _host_verdict, _rerandomise, _tiled_batch, dlog, golden,  # noqa: F401
                                   pool3)

pytestmark = pytest.mark.gpu

SEEDS = [hashlib.sha256(b"combined %d" % k).digest() for k in range(3)]


def _both(K, proofs, publics, vkj, seed=SEEDS[0]):
    """(verdicts, path) of the combined call, after checking the verdicts against groth16_verify_batch's"""
    got, path = K.groth16_verify_batch_combined(proofs, publics, vkj, seed=seed)
    assert got == K.groth16_verify_batch(proofs, publics, vkj)
    return got, path


def test_dlog_table_verdicts_and_path_equal_the_model(gpu, dlog):
    """every item of the table in batches of 1, 63, 64, 65 and 300 of one key, shuffled together as the per-item test does; then
    the key's valid items alone, tiled to 63 and 65: path = 1 exactly when every live item's model verdict is 1"""
    K = gpu
    table, _, texts = dlog
    sizes = (1, 63, 64, 65, 300)
    rnd = random.Random(6365)
    bad, paths = [], set()
    for t, ((key, items), (vkj, pq)) in enumerate(zip(table, texts)):
        def run(b, seed):
            got, path = _both(K, [pq[k][0] for k in b], [pq[k][1] for k in b], vkj, seed)
            live = [items[k].want for k in b if not items[k].json_only]
            want_path = int(all(w == 1 for w in live))
            paths.add((want_path, len(b) > 1))
            out = [("verdict", len(b), items[k].label, g, items[k].want) for k, g in zip(b, got) if g != items[k].want]
            if path != want_path:
                out.append(("path", len(b), [items[k].label for k in b][:4], path, want_path))
            return out
        for size in (sizes[t % 5], sizes[(t + 2) % 5]):
            idx = list(range(len(items))) + [rnd.randrange(len(items)) for _ in range(size - len(items))]
            rnd.shuffle(idx)
            for b in ([[k] for k in idx] if size == 1 else [idx]):
                bad += run(b, SEEDS[t % 3])
        valid = [k for k, it in enumerate(items) if it.want == 1]
        for size in (63, 65):
            bad += run([valid[i % len(valid)] for i in range(size)], SEEDS[(t + 1) % 3])
        sample = rnd.sample(range(len(items)), 3)
        assert [_host_verdict(K, pq[k][0], pq[k][1], vkj) for k in sample] == [items[k].want for k in sample]
    assert not bad, bad[:20]
    assert paths == {(1, False), (0, False), (1, True), (0, True)}


def test_cancellations_an_unweighted_product_would_accept(gpu, O):
    """c + 1 with c − 1, and two valid proofs of different statements with their signal vectors exchanged: the errors cancel in
    Π e(A, B)⁻¹·e(cpub, γ)·e(C, δ) without weights, so only the coefficients reject them"""
    K = gpu
    rnd = random.Random(77)
    key = M.random_key(rnd, 3, "n=3")
    sig1 = [rnd.randrange(R_ORDER) for _ in range(3)]
    sig2 = [rnd.randrange(R_ORDER) for _ in range(3)]
    a, b = rnd.randrange(1, R_ORDER), rnd.randrange(1, R_ORDER)
    plus = M.Item(key, M.prove(key, sig1, a, b, e=1), sig1, "c+1")
    minus = M.Item(key, M.prove(key, sig1, a + 5, b + 9, e=R_ORDER - 1), sig1, "c-1")
    p1, p2 = M.prove(key, sig1, a, b), M.prove(key, sig2, a + 1, b + 1)
    x1, x2 = M.Item(key, p1, sig2, "p1 with sig2"), M.Item(key, p2, sig1, "p2 with sig1")
    ok1, ok2 = M.Item(key, p1, sig1, "valid 1"), M.Item(key, p2, sig2, "valid 2")
    assert [it.want for it in (plus, minus, x1, x2, ok1, ok2)] == [0, 0, 0, 0, 1, 1]
    # the unweighted sums do cancel: Σ (a·b − γ·cpub − δ·c − α·β) ≡ 0 over each pair
    for pair in ((plus, minus), (x1, x2)):
        assert sum(it.proof.a * it.proof.b - key.alpha * key.beta - key.gamma * M.cpub_dlog(key, it.signals) - key.delta * it.proof.c
                   for it in pair) % R_ORDER == 0
    pts = M.Points(O)
    pts.need_items([plus, minus, x1, x2, ok1, ok2])
    pts.resolve()
    vkj = M.vk_json(pts, key)
    text = lambda it: (M.proof_json(pts, it.proof), M.public_json(it.signals))
    for pair in ((plus, minus), (x1, x2)):
        for lead in ([], [ok1, ok2] * 35):
            batch = [text(it) for it in lead + list(pair)]
            for seed in SEEDS + [None]:
                got, path = K.groth16_verify_batch_combined([p for p, _ in batch], [q for _, q in batch], vkj, seed=seed)
                assert path == 0 and got == [1] * len(lead) + [0, 0], (pair[0].label, len(lead), seed)
    got, path = K.groth16_verify_batch_combined([text(ok1)[0], text(ok2)[0]], [text(ok1)[1], text(ok2)[1]], vkj, seed=None)
    assert (got, path) == ([1, 1], 1)


def test_batch_of_4096_all_valid_then_one_flipped(gpu, golden):
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
    for seed in (SEEDS[0], SEEDS[1], None):
        assert K.groth16_verify_batch_combined(proofs, publics, vkj, seed=seed) == ([1] * 4096, 1)
    parse_ms, dev_ms = K.groth16_verify_batch_last_timings()
    assert parse_ms > 0 and dev_ms > 0
    i = 2777
    pu = json.loads(publics[i])
    publics[i] = json.dumps([str(int(pu[0]) ^ 2)] + pu[1:])
    want = [1] * 4096
    want[i] = 0
    assert _host_verdict(K, proofs[i], publics[i], vkj) == 0
    for seed in (SEEDS[0], SEEDS[2]):  # two seeds: equal verdicts
        assert _both(K, proofs, publics, vkj, seed) == (want, 0)


def test_chunk_boundary_with_gaps_in_the_live_list(gpu, pool3):
    """CHUNK + 4097 items tiled from the pool's valid proofs only, with ~1 % parse errors before the boundary: two chunks whose
    partial products and partial sums are combined, coefficients taken from the caller's indices across the gaps → path 1.
    Then a rejected proof on each side of the boundary: the exact verdicts through the fallback."""
    K = gpu
    vkj, items, texts = pool3
    good = [k for k in range(251) if items[k].want == 1]
    only_valid = (vkj, [items[k] for k in good] * 2, [texts[k] for k in good] * 2)  # _tiled_batch tiles the first 251 entries
    assert len(only_valid[1]) >= 251
    n = CHUNK + 4097
    errors = [i for i in range(0, CHUNK, 97)]
    proofs, publics, want = _tiled_batch(only_valid, n, errors)
    assert set(want) == {1, -2}
    live = [i for i in range(n) if want[i] != -2]
    last1, first2 = live[CHUNK - 1], live[CHUNK]
    assert last1 > CHUNK - 1 and len(live) - CHUNK < CHUNK
    got, path = K.groth16_verify_batch_combined(proofs, publics, vkj, seed=SEEDS[1])
    wrong = [(i, got[i], want[i]) for i in range(n) if got[i] != want[i]]
    assert not wrong and path == 1, (path, len(wrong), wrong[:10])
    bad = next(k for k in range(251) if items[k].want == 0)
    for i in (last1, first2):
        proofs[i], publics[i], want[i] = texts[bad][0], texts[bad][1], 0
    got, path = K.groth16_verify_batch_combined(proofs, publics, vkj, seed=SEEDS[1])
    wrong = [(i, got[i], want[i]) for i in range(n) if got[i] != want[i]]
    assert not wrong and path == 0, (path, len(wrong), wrong[:10], last1, first2)
    sample = [0, errors[1], last1, first2, n - 1]
    assert [_host_verdict(K, proofs[i], publics[i], vkj) for i in sample] == [want[i] for i in sample]


def test_real_proofs_from_the_prover_accepted(gpu, S, O):
    K = gpu
    r1, w = S.squaring_chain(300)
    zkey, vk = S.setup(r1, lambda g, k: K.generator_mul(g, k), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
    wtns = S.write_wtns(w)
    cm = K.CacheManager()
    try:
        cm.load("vbc", zkey)
        proofs = [cm.prove_mem("vbc", wtns, 3 + i, 5 + 2 * i)[:2] for i in range(6)]
    finally:
        cm.close()
        K.release_domain()
    vkj = S.vk_to_json(vk)
    assert K.groth16_verify_batch_combined([p for p, _ in proofs], [q for _, q in proofs], vkj) == ([1] * 6, 1)
    assert all(_host_verdict(K, p, q, vkj) == 1 for p, q in proofs)


def test_pairing_product_matches_the_host_product(gpu, O):
    K = gpu
    rnd = random.Random(1212)
    pts = M.Points(O)
    ab = [(rnd.randrange(1, R_ORDER), rnd.randrange(1, R_ORDER)) for _ in range(130)]
    pts.need("g1", [a for a, _ in ab])
    pts.need("g2", [b for _, b in ab])
    pts.resolve()
    P = [pts.g1(a) for a, _ in ab]
    Qs = [pts.g2(b) for _, b in ab]
    for k in (3, 64):
        P[k] = (0, 0)
    for k in (4, 129):
        Qs[k] = (0, 0, 0, 0)
    Pa = _arr([v for p in P for v in p]).reshape(-1, 2, 4)
    Qa = _arr([v for q in Qs for v in q]).reshape(-1, 4, 4)
    one = np.zeros((12, 4), dtype=np.uint64)
    one[0, 0] = 1
    want = one
    for k in range(1, 131):
        want = K.gt_op("mul", want, K.pairing(Pa[k - 1], Qa[k - 1]))
        if k in (1, 2, 63, 64, 65, 130):
            assert np.array_equal(K.pairing_product(Pa[:k], Qa[:k]), want), k
    assert not np.array_equal(want, one)
    assert np.array_equal(K.pairing_product(Pa[:0], Qa[:0]), one)
    assert np.array_equal(K.pairing_product(Pa[[3, 3, 64]], Qa[[3, 4, 129]]), one)  # all-identity inputs
    # bilinearity: e(aG₁, bG₂)·e(−abG₁, G₂) = 1
    a, b = ab[0]
    pts.need("g1", [-a * b])
    pts.need("g2", [1])
    pts.resolve()
    assert np.array_equal(K.pairing_product(_arr(list(P[0]) + list(pts.g1(-a * b))), _arr(list(Qs[0]) + list(pts.g2(1)))), one)
    # more pairs than the product kernel has lanes: every lane folds several Miller values
    idx = [i % 130 for i in range((1 << 14) + 300)]
    big = K.pairing_product(Pa[idx], Qa[idx])
    reps = [len([i for i in idx if i == k]) for k in range(130)]
    want = one
    for k in range(130):
        want = K.gt_op("mul", want, K.gt_op("pow", K.pairing(Pa[k], Qa[k]), reps[k]))
    assert np.array_equal(big, want)


def test_edges(gpu, golden):
    K = gpu
    g, vkj = golden
    p, pub = json.dumps(g["cases"][0]["proof"]), json.dumps(g["cases"][0]["public"])
    assert K.groth16_verify_batch_combined([], [], vkj) == ([], 1)
    assert K.groth16_verify_batch_combined([p], [pub], vkj) == ([1], 1)
    assert K.groth16_verify_batch_combined([p] * 70, [pub] * 70, vkj, device="HIP:0") == ([1] * 70, 1)
    assert K.groth16_verify_batch_combined([p[:-3], p], ["[1", pub], vkj) == ([-2, 1], 1)
    assert K.groth16_verify_batch_combined([p[:-3]], [pub], vkj) == ([-2], 1)  # no live item: nothing left to decide
    with pytest.raises(K.ProverError, match="malformed JSON"):
        K.groth16_verify_batch_combined([p], [pub], vkj[:-2])
    with pytest.raises(K.ProverError, match="nPublic"):
        K.groth16_verify_batch_combined([p], [pub], json.dumps(dict(json.loads(vkj), nPublic="x")))
    with pytest.raises(K.ProverError, match="one device"):
        K.groth16_verify_batch_combined([p], [pub], vkj, device="HIP:0-1")
    with pytest.raises(ValueError):
        K.groth16_verify_batch_combined([p], [pub], vkj, seed=b"short")


def test_cli_verify_batch_combined(gpu, golden, tmp_path):
    g, vkj = golden
    exe = os.path.join(ROOT, "icicle-snark_amd", "lib", "prove")
    lines = []
    for k, c in enumerate(g["cases"]):
        (tmp_path / f"p{k}.json").write_text(json.dumps(c["proof"]))
        (tmp_path / f"q{k}.json").write_text(json.dumps(c["public"]))
        lines.append(f"{tmp_path}/p{k}.json {tmp_path}/q{k}.json")
    (tmp_path / "good.txt").write_text("\n".join(lines) + "\n")
    (tmp_path / "bad.json").write_text(json.dumps(["1"]))
    lines.append(f"{tmp_path}/p0.json {tmp_path}/bad.json")
    lines.append(f"{tmp_path}/p0.json {tmp_path}/missing.json")
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    (tmp_path / "vk.json").write_text(vkj)
    cmds = (f"verify-batch --list {tmp_path}/good.txt --vk {tmp_path}/vk.json --device HIP --combined\n"
            f"verify-batch --list {tmp_path}/list.txt --vk {tmp_path}/vk.json --combined\nexit\n")
    out = subprocess.run([exe], input=cmds, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = [ln.replace("> ", "") for ln in out.stdout.splitlines()]
    assert got[:12] == ["0 accepted", "1 accepted", "accepted 2 rejected 0 errors 0", "decided by: combined equation", "COMMAND_COMPLETED",
                        "0 accepted", "1 accepted", "2 rejected", "3 error: cannot read input file", "accepted 2 rejected 1 errors 1",
                        "decided by: per-item fallback", "COMMAND_COMPLETED"], out.stdout
