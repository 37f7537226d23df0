"""Proofs of many keys in one call (K.VkSet.verify → groth16_verify_batch_mixed): verdict for verdict against groth16_verify_batch
key by key, the discrete-log model (tests/groth16_dlog_model.py) and, for samples, the host verifier; `path` and `keys_fallback`
against the model; with one key against groth16_verify_batch_combined; a wrong key tag; errors that cancel across two keys in an
unweighted product; one bad tenant among five; the chunk boundary; the call's error cases."""
import hashlib
import json
import random
import threading

import pytest

import groth16_dlog_model as M
from test_gpu_verify_batch import CHUNK, R_ORDER, _host_verdict, dlog, pool3  # noqa: F401

pytestmark = pytest.mark.gpu

SEEDS = [hashlib.sha256(b"mixed %d" % k).digest() for k in range(3)]


def _per_key_verdicts(K, vkjs, proofs, publics, key_of):
    """what groth16_verify_batch says, one call per key"""
    out = [None] * len(proofs)
    for k, vkj in enumerate(vkjs):
        at = [i for i, t in enumerate(key_of) if t == k]
        if at:
            for i, v in zip(at, K.groth16_verify_batch([proofs[i] for i in at], [publics[i] for i in at], vkj)):
                out[i] = v
    return out


def _valid_texts(dlog, t, count):
    """`count` valid (proof, public) texts of table key t, its valid items repeated"""
    table, _, texts = dlog
    good = [texts[t][1][k] for k, it in enumerate(table[t][1]) if it.want == 1]
    return [good[i % len(good)] for i in range(count)]


def _first_text(dlog, t, pick):
    table, _, texts = dlog
    k = next(k for k, it in enumerate(table[t][1]) if pick(it))
    return texts[t][1][k]


def _named(dlog, *names):
    table = dlog[0]
    return [next(t for t, (key, _) in enumerate(table) if key.name == n) for n in names]


def test_whole_table_in_one_batch(gpu, dlog):
    """ONE set of all keys of the table (0 to 40 signals; γ₂, δ₂, α₁ or β₂ the identity), every item of every key shuffled together"""
    K = gpu
    table, _, texts = dlog
    vkjs = [vkj for vkj, _ in texts]
    every = [(t, k) for t, (_, items) in enumerate(table) for k in range(len(items))]
    random.Random(11).shuffle(every)
    proofs = [texts[t][1][k][0] for t, k in every]
    publics = [texts[t][1][k][1] for t, k in every]
    key_of = [t for t, _ in every]
    items = [table[t][1][k] for t, k in every]
    want = [it.want for it in items]
    live = [it for it in items if not it.json_only]
    bad_keys = {id(it.key) for it in live if it.want != 1}
    with K.VkSet(vkjs) as vs:
        assert vs.n_keys == len(table) and [vs.n_public(t) for t in range(len(table))] == [key.n_public for key, _ in table]
        got, rep = vs.verify(proofs, publics, key_of, seed=SEEDS[0])
    assert got == want
    assert got == _per_key_verdicts(K, vkjs, proofs, publics, key_of)
    assert rep.path == int(all(it.want == 1 for it in live)) == 0
    assert rep.keys_fallback == len(bad_keys) and rep.keys_live == len({id(it.key) for it in live})
    assert {0, 40} <= {it.key.n_public for it in live} and set(want) == {1, 0, -2}
    for i in random.Random(12).sample(range(len(every)), 3):
        assert _host_verdict(K, proofs[i], publics[i], vkjs[key_of[i]]) == want[i]


@pytest.mark.parametrize("names,counts", [(["n=3"], [257]), (["n=8", "gamma=0"], [64, 0]),
                                           (["n=0", "n=40", "delta=0", "alpha=0", "beta=0"], [1, 2, 63, 0, 65])])
def test_all_valid_subsets_take_the_combined_path(gpu, dlog, names, counts):
    """per-key item counts 0, 1, 2, 63, 64, 65, 257 over sets of 1, 2 and 5 keys; a key of the set without an item changes nothing"""
    K = gpu
    texts = dlog[2]
    ts = _named(dlog, *names)
    batch = [(j, pq) for j, (t, c) in enumerate(zip(ts, counts)) for pq in _valid_texts(dlog, t, c)]
    random.Random(sum(counts)).shuffle(batch)
    with K.VkSet([texts[t][0] for t in ts]) as vs:
        got, rep = vs.verify([pq[0] for _, pq in batch], [pq[1] for _, pq in batch], [j for j, _ in batch], seed=SEEDS[1])
    assert got == [1] * sum(counts)
    assert (rep.path, rep.keys_fallback, rep.keys_live) == (1, 0, sum(c > 0 for c in counts))


def test_one_key_equals_the_combined_call(gpu, dlog):
    K = gpu
    table, _, texts = dlog
    t = _named(dlog, "n=3")[0]
    vkj, pq = texts[t]
    valid = _valid_texts(dlog, t, 70)
    mixed = [pq[k] for k, it in enumerate(table[t][1])] + valid
    with K.VkSet([vkj]) as vs:
        for batch in (valid, mixed):
            p, q = [a for a, _ in batch], [b for _, b in batch]
            got, rep = vs.verify(p, q, [0] * len(batch), seed=SEEDS[2])
            assert (got, rep.path) == K.groth16_verify_batch_combined(p, q, vkj, seed=SEEDS[2])
        assert rep.path == 0 and rep.keys_fallback == 1


def test_a_wrong_key_tag_is_rejected(gpu, dlog):
    """a valid proof of key a tagged with key b of equal n_public gives the model's verdict under b (0); rightly tagged, 1"""
    K = gpu
    table, _, texts = dlog
    a, b = _named(dlog, "n=2", "ic0=sum")
    assert table[a][0].n_public == table[b][0].n_public
    k = next(k for k, it in enumerate(table[a][1]) if it.want == 1 and it.label.endswith("valid"))
    it = table[a][1][k]
    assert M.model_verdict(table[b][0], it.proof, it.signals) == 0
    pj, qj = texts[a][1][k]
    with K.VkSet([texts[a][0], texts[b][0]]) as vs:
        assert vs.verify([pj, pj], [qj, qj], [1, 0], seed=SEEDS[0])[0] == [0, 1]
        got, rep = vs.verify([pj], [qj], [0], seed=SEEDS[0])
        assert (got, rep.path) == ([1], 1)
    assert K.groth16_verify_batch([pj], [qj], texts[b][0]) == [0]


def test_errors_that_cancel_across_two_keys(gpu, O):
    """item 1 under key 1 has error e₁, item 2 under key 2 has e₂ = −δ₁·e₁·δ₂⁻¹: an unweighted product over both keys accepts them
    (asserted in integers); the call rejects both, and both keys fall back"""
    K = gpu
    rnd = random.Random(21)
    keys = [M.random_key(rnd, 2, "k1"), M.random_key(rnd, 3, "k2")]
    sig = [[rnd.randrange(R_ORDER) for _ in range(k.n_public)] for k in keys]
    e1 = rnd.randrange(1, R_ORDER)
    e2 = -keys[0].delta * e1 * pow(keys[1].delta, -1, R_ORDER) % R_ORDER
    items = [M.Item(keys[j], M.prove(keys[j], sig[j], rnd.randrange(1, R_ORDER), rnd.randrange(1, R_ORDER), e=e), sig[j], f"e{j}")
             for j, e in enumerate((e1, e2))]
    assert [it.want for it in items] == [0, 0]
    assert sum(it.proof.a * it.proof.b - it.key.alpha * it.key.beta - it.key.gamma * M.cpub_dlog(it.key, it.signals) - it.key.delta * it.proof.c
               for it in items) % R_ORDER == 0
    pts = M.Points(O)
    pts.need_items(items)
    pts.resolve()
    proofs = [M.proof_json(pts, it.proof) for it in items]
    publics = [M.public_json(it.signals) for it in items]
    with K.VkSet([M.vk_json(pts, k) for k in keys]) as vs:
        for seed in SEEDS:
            got, rep = vs.verify(proofs, publics, [0, 1], seed=seed)
            assert (got, rep.path, rep.keys_fallback) == ([0, 0], 0, 2)


def test_one_bad_tenant_among_five(gpu, dlog):
    """five keys with 64 valid items each: one invalid item in key 3 costs key 3 alone the per-item stage; so does a pi_b outside
    the subgroup in key 1, which gets −2"""
    K = gpu
    texts = dlog[2]
    ts = _named(dlog, "n=2", "n=8", "ic2=O", "n=3", "gamma=0")
    batch = [(j, pq) for j, t in enumerate(ts) for pq in _valid_texts(dlog, t, 64)]
    random.Random(5).shuffle(batch)
    rejected = _first_text(dlog, ts[3], lambda it: it.want == 0)
    outside = _first_text(dlog, ts[1], lambda it: it.proof.b_outside)
    with K.VkSet([texts[t][0] for t in ts]) as vs:
        for tag, text, verdict in ((3, rejected, 0), (1, outside, -2)):
            at = 100
            b = batch[:at] + [(tag, text)] + batch[at:]
            got, rep = vs.verify([pq[0] for _, pq in b], [pq[1] for _, pq in b], [j for j, _ in b], seed=SEEDS[tag % 3])
            assert got == [1] * at + [verdict] + [1] * (len(batch) - at)
            assert (rep.path, rep.keys_fallback, rep.keys_live) == (0, 1, 5)


def test_chunk_boundary_with_gaps_in_the_live_list(gpu, dlog, pool3):
    """CHUNK + 65 items tiled from three keys with parse errors before the boundary: two lane launches whose values share one
    product, coefficients from the caller's indices across the gaps → path 1; then a rejected proof on each side of the boundary"""
    K = gpu
    vk0, items0, texts0 = pool3
    good0 = [texts0[k] for k in range(251) if items0[k].want == 1]
    bad0 = next(texts0[k] for k in range(251) if items0[k].want == 0)
    t1, t2 = _named(dlog, "n=8", "delta=0")
    pools = [good0, _valid_texts(dlog, t1, 7), _valid_texts(dlog, t2, 5)]
    n = CHUNK + 65
    key_of = [i % 3 for i in range(n)]
    proofs = [pools[i % 3][(i // 3) % len(pools[i % 3])][0] for i in range(n)]
    publics = [pools[i % 3][(i // 3) % len(pools[i % 3])][1] for i in range(n)]
    want = [1] * n
    for e, i in enumerate(range(0, CHUNK, 2003)):                   # 33 gaps: CHUNK + 32 live items
        if e % 2:
            proofs[i] = proofs[i][:-2]                                     # malformed JSON
        else:
            publics[i] = json.dumps(json.loads(publics[i])[:1])            # too few signals (every key here wants two or more)
        want[i] = -2
    live = [i for i in range(n) if want[i] != -2]
    assert len(live) > CHUNK and live[CHUNK - 1] > CHUNK - 1
    with K.VkSet([vk0, dlog[2][t1][0], dlog[2][t2][0]]) as vs:
        got, rep = vs.verify(proofs, publics, key_of, seed=SEEDS[1])
        wrong = [(i, got[i], want[i]) for i in range(n) if got[i] != want[i]]
        assert not wrong and (rep.path, rep.keys_live) == (1, 3), (rep.path, len(wrong), wrong[:10])
        last1 = next(i for i in reversed(live[:CHUNK]) if key_of[i] == 0)   # key 0's live items nearest to the boundary, one on each side
        first2 = next(i for i in live[CHUNK:] if key_of[i] == 0)
        for i in (last1, first2):
            proofs[i], publics[i], want[i] = bad0[0], bad0[1], 0
        got, rep = vs.verify(proofs, publics, key_of, seed=SEEDS[1])
        wrong = [(i, got[i], want[i]) for i in range(n) if got[i] != want[i]]
        assert not wrong and (rep.path, rep.keys_fallback) == (0, 1), (rep.path, rep.keys_fallback, len(wrong), wrong[:10], last1, first2)
    for i in (0, last1, first2, n - 1):
        assert _host_verdict(K, proofs[i], publics[i], [vk0, dlog[2][t1][0], dlog[2][t2][0]][key_of[i]]) == want[i]


def test_errors_and_threads(gpu, dlog):
    K = gpu
    texts = dlog[2]
    ts = _named(dlog, "n=2", "n=8")
    a, b = _valid_texts(dlog, ts[0], 1)[0], _valid_texts(dlog, ts[1], 1)[0]
    vs = K.VkSet([texts[t][0] for t in ts])
    try:
        got, rep = vs.verify([a[0], b[0], a[0], b[0]], [a[1], b[1], a[1], b[1]], [-1, 1, 0, 2], seed=SEEDS[0])
        assert got == [-2, 1, 1, -2] and rep.path == 1
        assert "key index" in K.lib().groth16_verify_last_error().decode()
        got, rep = vs.verify([], [], [])
        assert got == [] and rep.path == 1
        assert vs.verify([a[0], b[0]], [a[1], a[1]], [0, 1])[0] == [1, -2]          # too few signals for the tagged key
        assert vs.verify([a[0]], [a[1]], [5])[0] == [-2]                            # no live item at all
        with pytest.raises(ValueError):
            vs.verify([a[0]], [a[1]], [0], seed=b"short")
        with pytest.raises(K.ProverError, match="one device"):
            K.VkSet([texts[ts[0]][0]], device="HIP:0-1")
        # two threads on one set: the verdicts of serial calls
        batch = [(j, pq) for j, t in enumerate(ts) for pq in _valid_texts(dlog, t, 40)]
        batch.insert(17, (0, _first_text(dlog, ts[0], lambda it: it.want == 0)))
        args = ([pq[0] for _, pq in batch], [pq[1] for _, pq in batch], [j for j, _ in batch])
        serial = vs.verify(*args, seed=SEEDS[2])[0]
        assert serial == [1] * 17 + [0] + [1] * 63
        out = [None, None]

        def work(slot):
            out[slot] = vs.verify(*args, seed=SEEDS[slot])[0]
        threads = [threading.Thread(target=work, args=(s,)) for s in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert out == [serial, serial]
    finally:
        vs.free()
    with pytest.raises(K.ProverError, match="freed"):
        vs.verify([a[0]], [a[1]], [0])
    with pytest.raises(K.ProverError, match="freed"):
        vs.n_keys
    vs.free()   # a second free is harmless
