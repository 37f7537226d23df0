"""End-to-end parity (needs an MI355X): proofs from the HIP prover host are bit-identical — as parsed JSON
values, and here also as text — to the oracle pipeline (restated src/proof_helper.rs) on the same
zkey / witness / (r, s), equal the committed golden proof, and are accepted by the reference pairing check
when oracle/_ref is present."""
import base64
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, unhex, unhex_int

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cm(gpu):
    c = gpu.CacheManager()
    yield c
    c.close()
    gpu.release_domain()


def _fbm(K):
    return lambda g, sc: K.generator_mul(g, sc)


def test_golden_proof(gpu, cm):
    g = load_golden("groth16.json")
    zkey, wtns = base64.b64decode(g["zkey"]), base64.b64decode(g["wtns"])
    cm.load("golden", zkey)
    info = cm.info("golden")
    assert (info.n_vars, info.n_public, info.domain_size, info.n_coef) == (8, 1, 8, 14)
    for c in g["cases"]:
        pj, qj, _ = cm.prove_mem("golden", wtns, unhex_int(c["r"]), unhex_int(c["s"]))
        assert json.loads(pj) == c["proof"] and json.loads(qj) == c["public"]
        # serde_json::to_writer_pretty layout: sorted keys, two-space indent
        assert pj == json.dumps(c["proof"], indent=2, sort_keys=True)
        assert qj == json.dumps(c["public"], indent=2)


@pytest.mark.parametrize("N", [50, 3000, 40000])
def test_squaring_chain_vs_oracle(gpu, cm, O, S, N):
    K = gpu
    r1, w = S.squaring_chain(N)
    zkey, vk = S.setup(r1, _fbm(K), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
    wtns = S.write_wtns(w)
    key = f"sq{N}"
    cm.load(key, zkey)
    cache = O.build_cache(O.parse_zkey(zkey))
    for (r, s) in ((1, 1), (0x1234567890ABCDEF << 100, 987654321)):
        pj, qj, tm = cm.prove_mem(key, wtns, r, s)
        proof, public = O.groth16_prove(zkey, wtns, r, s, cache=cache)
        assert json.loads(pj) == proof and json.loads(qj) == public
    assert json.loads(qj) == [str(pow(3, 1 << N, O.R_MOD))]
    # random blinding: a different but valid proof each time
    p1, _, _ = cm.prove_mem(key, wtns)
    p2, _, _ = cm.prove_mem(key, wtns)
    assert p1 != p2
    vkj = S.vk_to_json(dict(vk, n_public=len(vk["IC"]) - 1))
    assert K.groth16_verify_json(pj, qj, vkj) and K.groth16_verify_json(p1, qj, vkj)
    import ref as R
    if R.available():
        assert R.groth16_verify(json.loads(pj), json.loads(qj), vk)
        assert R.groth16_verify(json.loads(p1), json.loads(qj), vk)
    cm.evict(key)


def test_bit_heavy_random_circuit_vs_oracle(gpu, cm, O, S):
    """stand-in for the RSA/SHA-style circuits: sparse random R1CS, witness dominated by 0/1 wires."""
    K = gpu
    r1, w = S.random_circuit(6000, 3, 40, bit_fraction=0.8)
    zkey, vk = S.setup(r1, _fbm(K), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
    wtns = S.write_wtns(w)
    cm.load("rand", zkey)
    pj, qj, _ = cm.prove_mem("rand", wtns, 5, 7)
    proof, public = O.groth16_prove(zkey, wtns, 5, 7)
    assert json.loads(pj) == proof and json.loads(qj) == public
    assert K.groth16_verify_json(pj, qj, S.vk_to_json(dict(vk, n_public=len(vk["IC"]) - 1)))
    import ref as R
    if R.available():
        assert R.groth16_verify(proof, public, vk)
    cm.evict("rand")


def test_sharded_commitments_sum_to_the_unsharded_proof(gpu, cm, O, S):
    """multi-GPU decomposition on one device: 3 point-range shards, partial commitments summed like the
    gathered blocks of the RCCL path."""
    K = gpu
    r1, w = S.squaring_chain(1000)
    zkey, _ = S.setup(r1, _fbm(K), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
    wtns = S.write_wtns(w)
    cm.load("full", zkey)
    want, _, _ = cm.prove_mem("full", wtns, 11, 13)
    blocks = b""
    for rank in range(3):
        cm.load(f"shard{rank}", zkey, shard_rank=rank, shard_count=3)
        blk, _ = cm.commitments(f"shard{rank}", wtns)
        blocks += blk
    total = K.sum_commitments(blocks, 3)
    got, _ = cm.assemble("full", wtns, total, 11, 13)
    assert got == want


@pytest.mark.parametrize("count", [2, 4, 8])
def test_power_of_two_shards_use_residue_classes_of_h(gpu, cm, O, S, count):
    """power-of-two shard counts: H is split by k mod count and every rank runs the folded forward transform
    (qap_coset_fold3 + a size-n/count NTT) instead of the full one; the partial commitments still sum to the unsharded
    proof, which equals the oracle's."""
    K = gpu
    N = 20000                                         # domain 2^15: n / count >= 1024 for every count tested
    r1, w = S.squaring_chain(N)
    zkey, _ = S.setup(r1, _fbm(K), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
    wtns = S.write_wtns(w)
    key = f"full{count}"
    cm.load(key, zkey)
    want, public, _ = cm.prove_mem(key, wtns, 21, 34)
    proof, pub = O.groth16_prove(zkey, wtns, 21, 34)
    assert json.loads(want) == proof and json.loads(public) == pub
    blocks = b""
    for rank in range(count):
        cm.load(f"p2shard{count}_{rank}", zkey, shard_rank=rank, shard_count=count)
        blk, _ = cm.commitments(f"p2shard{count}_{rank}", wtns)
        blocks += blk
        cm.evict(f"p2shard{count}_{rank}")
    got, _ = cm.assemble(key, wtns, K.sum_commitments(blocks, count), 21, 34)
    assert got == want
    cm.evict(key)


def test_cli_repl_protocol(gpu, O, S, tmp_path):
    """the `prove` worker: same stdin protocol and sentinels as src/main.rs:121-186."""
    K = gpu
    r1, w = S.squaring_chain(64)
    zkey, vk = S.setup(r1, _fbm(K))
    (tmp_path / "c.zkey").write_bytes(zkey)
    (tmp_path / "w.wtns").write_bytes(S.write_wtns(w))
    exe = os.path.join(ROOT, "icicle-snark_amd", "lib", "prove")
    cmd = f"prove --witness {tmp_path}/w.wtns --zkey {tmp_path}/c.zkey --proof {tmp_path}/p.json --public {tmp_path}/q.json --device HIP\n"
    out = subprocess.run([exe], input="\n" + cmd + cmd + "exit\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.count("COMMAND_COMPLETED") == 4 and "COMMAND_EMPTY" in out.stdout and "COMMAND_EXIT" in out.stdout
    assert out.stdout.count("proof took") == 2
    proof = json.loads((tmp_path / "p.json").read_text())
    assert json.loads((tmp_path / "q.json").read_text()) == [str(pow(3, 1 << 64, O.R_MOD))]
    assert proof["protocol"] == "groth16" and proof["curve"] == "bn128"
    import ref as R
    if R.available():
        assert R.groth16_verify(proof, json.loads((tmp_path / "q.json").read_text()), vk)


def test_prover_errors(gpu, cm, S, O):
    K = gpu
    with pytest.raises(K.ProverError):
        cm.load("bad", b"nope" + bytes(100))
    r1, w = S.squaring_chain(10)
    zkey, _ = S.setup(r1, _fbm(K))
    cm.load("ten", zkey)
    with pytest.raises(K.ProverError):      # wrong witness length (src/proof_helper.rs:257-262)
        cm.prove_mem("ten", S.write_wtns(w[:-1]), 1, 1)
    with pytest.raises(K.ProverError):
        cm.prove_mem("missing", S.write_wtns(w), 1, 1)
    with pytest.raises(K.ProverError):      # no CPU fallback
        cm.prove("w", "z", "p", "q", device="CPU")
    # a coefficient record that points outside the domain is rejected by the device-side CSR build
    (off, _), = O.read_sections(zkey, b"zkey")[4]
    bad = bytearray(zkey)
    bad[off + 4 + 3 * 44 + 4: off + 4 + 3 * 44 + 8] = (1 << 20).to_bytes(4, "little")   # record 3: c = 2^20 ≥ n
    with pytest.raises(K.ProverError, match="coefficient 3 out of range"):
        cm.load("bad-coef", bytes(bad))


def test_repeated_and_opposite_points_in_one_bucket(gpu, cm, O, S):
    """the exceptional cases of the bucket accumulation on the prover's table path: a run of equal witness values
    over base points that are copies of one point (P + P: the doubling branch) or alternate P, −P (sum = identity,
    then identity + P), in the G1 sections A / B1 / C and the G2 section B2.  Same modified zkey and witness for
    the oracle; such a witness does not satisfy the circuit, the commitments are compared all the same."""
    K = gpu
    N = 600
    r1, w = S.squaring_chain(N)
    zkey, _ = S.setup(r1, _fbm(K), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
    sec = O.read_sections(zkey, b"zkey")
    z = bytearray(zkey)
    q = O.Q_MOD

    def neg(pt, coord):          # Montgomery form of −y is q − (Montgomery form of y); G2: both components of y
        half = len(pt) // 2
        out = bytearray(pt)
        for k in range(half, len(pt), coord):
            y = int.from_bytes(pt[k:k + coord], "little")
            out[k:k + coord] = ((q - y) % q).to_bytes(coord, "little")
        return bytes(out)
    for sid, size, first in ((5, 64, 0), (6, 64, 0), (7, 128, 0), (8, 64, 2)):   # C starts at wire n_public + 1 = 2
        (off, _), = sec[sid]
        base = bytes(z[off + (20 - first) * size: off + (21 - first) * size])
        for i in range(21, 200):      # alternate P, −P
            z[off + (i - first) * size: off + (i - first + 1) * size] = base if i % 2 == 0 else neg(base, 32)
        for i in range(300, 420):     # copies of P
            z[off + (i - first) * size: off + (i - first + 1) * size] = base
    w = list(w)
    for i in range(20, 200):
        w[i] = w[20]
    for i in range(300, 420):
        w[i] = w[300]
    zkey2, wtns = bytes(z), S.write_wtns(w)
    cm.load("degenerate", zkey2)
    pj, qj, _ = cm.prove_mem("degenerate", wtns, 3, 9)
    proof, public = O.groth16_prove(zkey2, wtns, 3, 9)
    assert json.loads(pj) == proof and json.loads(qj) == public
    cm.evict("degenerate")


def test_edge_scalars_in_the_witness(gpu, cm, O, S):
    """signed-digit recoding at its limits on the prover's table path (the windows tile the 254 bits exactly there):
    witness values around (r − 1)/2 — the negation threshold —, around 2^253, r − 1, and values whose low bits are all
    ones (carries through every window).  Not a satisfying witness; the proof is compared with the oracle's."""
    K = gpu
    r1, w = S.squaring_chain(400)
    zkey, _ = S.setup(r1, _fbm(K), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
    R = O.R_MOD
    half = (R - 1) // 2
    edge = [half, half + 1, half - 1, half + 2, (1 << 253) - 1, 1 << 253, (1 << 253) + 1, R - 1, R - 2, 1, 2,
            half - (half % (1 << 200)) - 1, (half >> 230 << 230) - 1, (1 << 252) - 1, (1 << 240) - 1, ((1 << 253) - 1) ^ (1 << 19)]
    w = list(w)
    for k, v in enumerate(edge):
        w[5 + k] = v % R
        w[100 + k] = (R - v) % R
    wtns = S.write_wtns(w)
    cm.load("edge", zkey)
    pj, qj, _ = cm.prove_mem("edge", wtns, 7, 11)
    proof, public = O.groth16_prove(zkey, wtns, 7, 11)
    assert json.loads(pj) == proof and json.loads(qj) == public
    cm.evict("edge")


@pytest.mark.parametrize("N", [33_000, 262_200])
def test_edge_scalars_in_the_witness_tables(gpu, cm, O, S, N):
    """The same on the witness tables of keys large enough for them (witness_table_geometry, csrc/prover/cache.cpp): 33 002 wires
    run c = 16 / 16 windows, the last two narrowed, on the LDS-staged sort; 262 202 wires run c = 18 / 15 windows with EVERY window
    one bit narrow (wide = 0: 15 × 17 bits ≥ 254), the width the rule narrows to from 19 because a bucket would hold fewer than 28
    entries.  Squaring chains whose witness is overwritten in place — wire 0 and the public wires stay — with the edge list of
    tests/msm_inputs.py for the geometry that runs (each window's digit 1, its negative extreme with the carry, all-ones below,
    r − v of each, the negation threshold, 2^253): from wire n_public + 1 on, the first wire of the C MSM (its skip_below), whose
    other side is the public wires; across wires 1023 | 1024, the sort's tile border; and at the last wires.  Not a satisfying
    witness; proof and publics are the oracle's, and the four witness MSMs report the geometry named here."""
    import msm_inputs as MI
    K = gpu
    O.calibrate_threads()
    wires = N + 2
    c, W, wide = MI.WITNESS_GEOMS[wires]
    zkey, wtns = importlib.import_module("bench").make_inputs(K, S, N)
    key = f"edge{N}"
    cm.load(key, zkey)                                              # dense tables built inside the load
    info = cm.info(key)
    assert info.n_vars == wires
    E = MI.ints_to_arr(MI.edge_list((c, W, wide)))
    n = len(E)
    wb = np.frombuffer(wtns, dtype=np.uint8).copy()
    body = wb[len(wb) - 32 * wires:].view(np.uint64).reshape(-1, 4)
    first = info.n_public + 1
    starts = [first, 1024 - n // 2, wires - n]
    assert first + n <= starts[1] and starts[1] + n <= starts[2]
    for k, s in enumerate(starts):
        body[s:s + n] = np.roll(E, -k * (n // 3), axis=0)
    edged = wb.tobytes()
    pj, qj, _ = cm.prove_mem(key, edged, 7, 11)
    geoms = [K.msm_profile(back)[1] for back in (4, 3, 2, 1)]       # A, B1, B2, C
    cm.evict(key)
    assert [(g["c"], g["W"], g["nbuckets"]) for g in geoms] == [(c, W, 1 << (c - 1))] * 4, geoms
    assert [g["is_g2"] for g in geoms] == [False, False, True, False]
    proof, public = O.groth16_prove(zkey, edged, 7, 11)
    assert json.loads(pj) == proof and json.loads(qj) == public


def test_identity_b_bases_and_table_free_layout(gpu, O, S, tmp_path):
    """Wires without a B-side occurrence have the identity as their B1/B2 base (snarkjs writes all-zero bytes): the bucket
    kernels skip them.  Same proof as the oracle's with the fixed-base tables (default) and with the classic layout of a
    memory-constrained host (ICICLE_SNARK_TABLES=0, read at cache build: its own process), and through three point-range shards."""
    import subprocess
    import sys
    K = gpu
    r1, w = S.random_circuit(3000, 3, 40, bit_fraction=0.7)
    zkey, _ = S.setup(r1, _fbm(K), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
    wtns = S.write_wtns(w)
    r, s = 0x1234567, 0x7654321
    proof, public = O.groth16_prove(zkey, wtns, r, s)
    c = K.CacheManager()
    c.load("k", zkey)
    pj, qj, _ = c.prove_mem("k", wtns, r, s)
    assert json.loads(pj) == proof and json.loads(qj) == public
    blocks = []
    for rank in range(3):
        c.load(f"s{rank}", zkey, shard_rank=rank, shard_count=3)
        blocks.append(c.commitments(f"s{rank}", wtns)[0])
    assert c.assemble("k", wtns, K.sum_commitments(b"".join(blocks), 3), r, s)[:2] == (pj, qj)
    c.close()
    (tmp_path / "c.zkey").write_bytes(zkey)
    (tmp_path / "w.wtns").write_bytes(wtns)
    code = (
        "import importlib, json, sys; sys.path.insert(0, %r)\n"
        "K = importlib.import_module('icicle-snark_amd'); K.set_device('HIP', 0)\n"
        "cm = K.CacheManager(); cm.load('k', open(%r, 'rb').read())\n"
        "pj, qj, _ = cm.prove_mem('k', open(%r, 'rb').read(), %d, %d); print(json.dumps([json.loads(pj), json.loads(qj)]))\n"
    ) % (ROOT, str(tmp_path / "c.zkey"), str(tmp_path / "w.wtns"), r, s)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, ICICLE_SNARK_TABLES="0"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == [proof, public]


def test_mutated_witness_files_never_crash(gpu, cm):
    """400 random mutations of the golden .wtns (truncations, bit flips, overwritten length fields, insertions) through the
    prover: each either proves (the mutation hit value bytes) or is refused with an error — none takes the process down or
    wedges the cache entry (the golden proof still comes out afterwards)."""
    import random
    g = load_golden("groth16.json")
    zkey, wtns = base64.b64decode(g["zkey"]), base64.b64decode(g["wtns"])
    cm.load("fuzz", zkey)
    rng = random.Random(7)
    proved = refused = 0
    for _ in range(400):
        b = bytearray(wtns)
        k = rng.randrange(5)
        if k == 0:
            del b[rng.randrange(len(b)):]
        elif k == 1:
            for _ in range(rng.randrange(1, 6)):
                b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
        elif k == 2:
            i = rng.randrange(0, len(b) - 8)
            b[i:i + 8] = rng.choice([b"\xff" * 8, b"\0" * 8, (2 ** 63).to_bytes(8, "little"), (len(b) * 3).to_bytes(8, "little")])
        elif k == 3:
            i = rng.randrange(len(b))
            b[i:i] = bytes(rng.randrange(256) for _ in range(rng.randrange(1, 40)))
        else:
            i = rng.randrange(0, len(b) - 4)
            b[i:i + 4] = rng.choice([b"\xff\xff\xff\xff", b"\0\0\0\0", b"\x01\0\0\x80"])
        try:
            cm.prove_mem("fuzz", bytes(b), 3, 5)
            proved += 1
        except gpu.ProverError:
            refused += 1
    assert proved + refused == 400 and refused > 100
    c = g["cases"][0]
    pj, qj, _ = cm.prove_mem("fuzz", wtns, unhex_int(c["r"]), unhex_int(c["s"]))
    assert json.loads(pj) == c["proof"] and json.loads(qj) == c["public"]
    cm.evict("fuzz")


def test_mutated_zkey_files_never_crash(gpu):
    """200 random mutations of the golden .zkey through cache build + prove on the device: a mutated key is refused, or builds
    and proves (bit flips inside point or coefficient bytes give a different, meaningless proof) — no crash, no hang, and the
    untouched key still yields the golden proof afterwards."""
    import random
    K = gpu
    g = load_golden("groth16.json")
    zkey, wtns = base64.b64decode(g["zkey"]), base64.b64decode(g["wtns"])
    rng = random.Random(11)
    built = refused = 0
    c = K.CacheManager()
    for it in range(200):
        b = bytearray(zkey)
        k = rng.randrange(5)
        if k == 0:
            del b[rng.randrange(len(b)):]
        elif k == 1:
            for _ in range(rng.randrange(1, 6)):
                b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
        elif k == 2:
            i = rng.randrange(0, len(b) - 8)
            b[i:i + 8] = rng.choice([b"\xff" * 8, b"\0" * 8, (2 ** 63).to_bytes(8, "little"), (len(b) * 3).to_bytes(8, "little")])
        elif k == 3:
            i = rng.randrange(len(b))
            b[i:i] = bytes(rng.randrange(256) for _ in range(rng.randrange(1, 40)))
        else:
            i = rng.randrange(0, len(b) - 4)
            b[i:i + 4] = rng.choice([b"\xff\xff\xff\xff", b"\0\0\0\0", b"\x01\0\0\x80", b"\x09\0\0\0"])
        key = f"m{it}"
        try:
            c.load(key, bytes(b))
            c.prove_mem(key, wtns, 3, 5)
            built += 1
        except K.ProverError:
            refused += 1
        c.evict(key)
    assert built + refused == 200 and refused > 20 and built > 20, (built, refused)
    c.load("ok", zkey)
    case = g["cases"][0]
    pj, qj, _ = c.prove_mem("ok", wtns, unhex_int(case["r"]), unhex_int(case["s"]))
    assert json.loads(pj) == case["proof"] and json.loads(qj) == case["public"]
    c.close()


def test_pinned_witness_buffer_takes_the_direct_dma_path(gpu, cm):
    """a witness handed over in pinned host memory (hipHostMalloc) is copied by one DMA in stream order instead of through the
    staging workers: same proof as from a pageable buffer"""
    import ctypes as C
    g = load_golden("groth16.json")
    zkey, wtns = base64.b64decode(g["zkey"]), base64.b64decode(g["wtns"])
    cm.load("pin", zkey)
    c = g["cases"][0]
    r, s = unhex_int(c["r"]), unhex_int(c["s"])
    want = cm.prove_mem("pin", wtns, r, s)[:2]
    hip = C.CDLL("libamdhip64.so")
    p = C.c_void_p()
    assert hip.hipHostMalloc(C.byref(p), C.c_size_t(len(wtns)), 0) == 0
    try:
        C.memmove(p, wtns, len(wtns))
        pinned = (C.c_char * len(wtns)).from_address(p.value)
        pj, qj = C.create_string_buffer(1 << 14), C.create_string_buffer(1 << 16)
        for _ in range(3):
            rc = gpu.lib().groth16_prove_mem(cm._h, b"pin", pinned, C.c_size_t(len(wtns)), int(r).to_bytes(32, "little"), int(s).to_bytes(32, "little"),
                                             pj, C.c_size_t(len(pj)), qj, C.c_size_t(len(qj)), None)
            assert rc == 0
            assert (pj.value.decode(), qj.value.decode()) == want
    finally:
        hip.hipHostFree(p)
    assert json.loads(want[0]) == c["proof"]
    cm.evict("pin")


def test_cache_budget_evicts_least_recently_used_keys(gpu, O, S):
    """groth16_cache_set_budget (the reference's CacheManager never evicts, src/cache.rs:110-114; the fixed-base tables make an entry
    ≈ 10× its size): with a budget that holds two of three keys, loading the third evicts the least recently USED one; proofs
    of the surviving keys are unchanged, and the evicted key simply builds again."""
    K = gpu
    keys = {}
    for name, n in (("a", 2500), ("b", 2600), ("c", 2700)):
        r1, w = S.squaring_chain(n)
        zkey, _ = S.setup(r1, _fbm(K), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
        keys[name] = (zkey, S.write_wtns(w))
    c = K.CacheManager()
    c.load("a", keys["a"][0])
    c.load("b", keys["b"][0])
    pa = c.prove_mem("a", keys["a"][1], 3, 4)[0]
    pb = c.prove_mem("b", keys["b"][1], 3, 4)[0]
    size_a, size_b = c.info("a").device_bytes, c.info("b").device_bytes
    need_c = 11 * len(keys["c"][0])                           # the size estimate of a new entry: 11 × its zkey
    c.set_budget(max(size_a, size_b) + need_c + (1 << 20))    # room for "c" next to ONE of the two
    assert size_a + size_b + need_c > max(size_a, size_b) + need_c + (1 << 20)
    c.prove_mem("a", keys["a"][1], 3, 4)                      # "a" is now more recently used than "b"
    c.load("c", keys["c"][0])
    assert c.contains("a") and c.contains("c") and not c.contains("b")
    assert c.prove_mem("a", keys["a"][1], 3, 4)[0] == pa
    c.set_budget(0)
    c.load("b", keys["b"][0])
    assert c.prove_mem("b", keys["b"][1], 3, 4)[0] == pb
    c.close()


def test_cache_info_sized_respects_the_callers_struct_size(gpu, cm):
    """groth16_cache_info_sized writes no more than the caller's sizeof(Groth16CircuitInfo): a binary built against an older,
    shorter struct is not overrun when the struct grows (round-2 advisor finding)."""
    import ctypes as C
    K = gpu
    if not cm.contains("g"):
        cm.load("g", base64.b64decode(load_golden("groth16.json")["zkey"]))
    full = cm.info("g")
    buf = (C.c_uint8 * 64)(*([0xAB] * 64))
    lib = K.lib()
    assert lib.groth16_cache_info_sized(cm._h, b"g", buf, C.c_size_t(24)) == 0
    raw = bytes(buf)
    assert raw[24:] == b"\xab" * 40                                     # nothing beyond the 24 bytes the caller has
    assert int.from_bytes(raw[0:4], "little") == full.n_vars and int.from_bytes(raw[16:24], "little") == full.device_bytes
    assert lib.groth16_cache_info_sized(cm._h, b"g", buf, C.c_size_t(64)) == 0
    assert int.from_bytes(bytes(buf)[24:28], "little") == full.b_bases
    assert lib.groth16_cache_info_sized(cm._h, b"nokey", buf, C.c_size_t(64)) != 0
    assert bytes(buf)[28:32] == (0).to_bytes(4, "little")                # one shard: not a device group


@pytest.mark.parametrize("pct", [35, 60])
def test_witness_head_and_tail_accumulate_into_the_same_buckets(gpu, pct):
    """A witness on its way in is split (csrc/prover/prover.cpp): the head is sorted and accumulated into the four bucket arrays
    while the tail is still being uploaded, the tail's accumulation continues those buckets (`into`).  Forced here on circuits
    the oracle proves in seconds (ICICLE_SNARK_HEAD_MIN=0; in production only witnesses of ≥ 2^19 wires are split): dense and
    bit-heavy witnesses (large buckets with `into`), pageable buffer, file and pinned buffer, each equal to the proof of the
    SAME witness resident on the device — the single-sort path — for the same (r, s), to the oracle's, and accepted by the
    pairing check."""
    code = r'''
import ctypes as C, importlib, json, os, sys, tempfile
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "oracle"))
import oracle as O
K = importlib.import_module("icicle-snark_amd"); S = importlib.import_module("icicle-snark_amd.synth")
bench = importlib.import_module("bench")
K.set_device("HIP", 0)
hip = C.CDLL("libamdhip64.so")
tmp = tempfile.mkdtemp()
for name in ("chain", "bits"):
    if name == "chain":
        zkey, wtns = bench.make_inputs(K, S, 200000)
        vk = None
    else:
        zkey, wtns, vk, nc = bench.make_standin_inputs(K, S, "aadhaar_standin", scale=0.22)
    cm = K.CacheManager(); cm.load(name, zkey)
    for rep in range(3):                                   # (the stand-in key rebuilds its tables after the first prove)
        split = cm.prove_mem(name, wtns, 11 + rep, 5)[:2]  # pageable buffer in: head / tail
        whole = cm.prove_mem(name, wtns, 11 + rep, 5, resident=True)[:2]
        assert split == whole, (name, rep)
    proof, public = O.groth16_prove(zkey, wtns, 13, 5)
    assert json.loads(split[0]) == proof and json.loads(split[1]) == public, name
    if vk is not None:
        assert K.groth16_verify_json(split[0], split[1], S.vk_to_json(vk))
    # pinned buffer in: two DMAs with an event between them
    p = C.c_void_p()
    assert hip.hipHostMalloc(C.byref(p), C.c_size_t(len(wtns)), 0) == 0
    C.memmove(p, wtns, len(wtns))
    pinned = (C.c_char * len(wtns)).from_address(p.value)
    pj, qj = C.create_string_buffer(1 << 14), C.create_string_buffer(1 << 20)
    rc = K.lib().groth16_prove_mem(cm._h, name.encode(), pinned, C.c_size_t(len(wtns)), (13).to_bytes(32, "little"), (5).to_bytes(32, "little"), pj, C.c_size_t(len(pj)), qj, C.c_size_t(len(qj)), None)
    assert rc == 0 and (pj.value.decode(), qj.value.decode()) == split, name
    # files in, files out (random r, s): same public signals, valid proof
    zp, wp = os.path.join(tmp, name + ".zkey"), os.path.join(tmp, name + ".wtns")
    open(zp, "wb").write(zkey); open(wp, "wb").write(wtns)
    cm.prove_files(wp, zp, os.path.join(tmp, "proof.json"), os.path.join(tmp, "public.json"))
    assert open(os.path.join(tmp, "public.json")).read() == split[1]
    if vk is not None:
        assert K.groth16_verify_json(open(os.path.join(tmp, "proof.json")).read(), split[1], S.vk_to_json(vk))
    cm.close()
print("HEAD_TAIL_OK")
''' % (ROOT, ROOT)
    env = dict(os.environ, ICICLE_SNARK_HEAD_MIN="0", ICICLE_SNARK_HEAD_PCT=str(pct), ICICLE_SNARK_QUIET="1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=1500, env=env)
    assert "HEAD_TAIL_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_proofs_across_the_deferred_table_build(gpu, O, S, tmp_path):
    """groth16_cache_load returns once the key can prove in the classic layout; the fixed-base tables are built behind its first
    proof and adopted by a later prove (csrc/prover/cache.cpp: TableBuild).  Every proof of a loop that crosses the swap —
    host buffer, resident witness and the file entry point — equals the oracle's; an evict in the middle of a build is clean;
    ICICLE_SNARK_DEFER_TABLES=0 builds the tables inside the load."""
    K = gpu
    N = 100_000
    zkey, wtns = importlib.import_module("bench").make_inputs(K, S, N)
    cache = O.build_cache(O.parse_zkey(zkey))
    want = {rs: O.groth16_prove(zkey, wtns, *rs, cache=cache) for rs in ((1, 1), (9, 4))}
    cm = K.CacheManager()
    cm.load("d", zkey, wait_tables=False)
    assert not cm.tables_ready("d")
    seen, after = [], 0
    for i in range(400):
        rs = list(want)[i % 2]
        rdy = cm.tables_ready("d")
        pj, qj, _ = cm.prove_mem("d", wtns, *rs, resident=(i % 3 == 2))
        assert json.loads(pj) == want[rs][0] and json.loads(qj) == want[rs][1], (i, rdy)
        seen.append(rdy)
        after += 1 if rdy else 0
        if after >= 3:
            break
    assert seen[0] is False and seen[-1] is True
    assert cm.tables_ready("d", wait=True)
    # evicted while the build is (most likely) under way: the worker stops at its next slice and the entry goes away cleanly
    cm.load("e", zkey, wait_tables=False)
    cm.prove_mem("e", wtns, 1, 1)                                # releases the build
    cm.evict("e")
    # the file entry point on a fresh key, then again after the tables have been adopted
    zp, wp = tmp_path / "c.zkey", tmp_path / "w.wtns"
    zp.write_bytes(zkey)
    wp.write_bytes(wtns)
    for rep in range(2):
        cm.prove_files(str(wp), str(zp), str(tmp_path / "p.json"), str(tmp_path / "q.json"))
        assert json.loads((tmp_path / "q.json").read_text()) == want[(1, 1)][1]
        assert cm.tables_ready(f"{zp}_HIP", wait=True)
    # a witness of 0 / 1 wires and small values: the first (classic) prove counts its non-zero digits and the deferred build gives the
    # four witness tables the narrower digits such a witness wants AT ONCE (no dense tables first, no rebuild inside a later prove)
    rng = np.random.default_rng(3)
    wb = np.frombuffer(wtns, dtype=np.uint8).copy()
    body = wb[len(wb) - 32 * (N + 2):].view(np.uint64).reshape(-1, 4)
    kind = rng.random(N + 2)
    bits = kind < 0.7
    body[bits] = 0
    body[bits, 0] = rng.integers(0, 2, size=int(bits.sum()), dtype=np.uint64)
    small = (kind >= 0.7) & (kind < 0.8)
    body[small, 1:] = 0
    body[0] = 0
    body[0, 0] = 1
    light = wb.tobytes()
    want_light = O.groth16_prove(zkey, light, 3, 8, cache=cache)
    cm.load("light", zkey, wait_tables=False)
    pj, qj, _ = cm.prove_mem("light", light, 3, 8)                # classic layout; releases the build
    assert json.loads(pj) == want_light[0] and json.loads(qj) == want_light[1]
    assert cm.tables_ready("light", wait=True)
    t0 = __import__("time").perf_counter()
    pj, qj, _ = cm.prove_mem("light", light, 3, 8)                # first prove on the tables: no rebuild inside it
    first_tab_ms = (__import__("time").perf_counter() - t0) * 1e3
    assert json.loads(pj) == want_light[0]
    c_light = K.msm_profile(4)[1]["c"]                            # A's geometry (back = 4)
    cm.load("dense", zkey)
    cm.prove_mem("dense", wtns, 3, 8)
    c_dense = K.msm_profile(4)[1]["c"]
    assert c_light <= c_dense - 2, (c_light, c_dense)
    assert first_tab_ms < 60, first_tab_ms                        # (a rebuild of four tables inside the prove takes > 100 ms)
    pj, qj, _ = cm.prove_mem("light", wtns, 1, 1)                 # … and a dense witness on the narrow tables is still right
    assert json.loads(pj) == want[(1, 1)][0]
    # a key that HAS its dense tables follows a light witness too: the prove that counted the digits starts the worker at its end, so one
    # prove + a wait is enough for the next prove to run on the narrow tables (what bench.py does before its warm timings)
    cm.load("follow", zkey)                                       # dense tables built in the load
    pj, qj, _ = cm.prove_mem("follow", light, 3, 8)
    assert json.loads(pj) == want_light[0] and K.msm_profile(4)[1]["c"] == c_dense
    assert cm.tables_ready("follow", wait=True)
    pj, qj, _ = cm.prove_mem("follow", light, 3, 8)
    assert json.loads(pj) == want_light[0] and K.msm_profile(4)[1]["c"] <= c_dense - 2
    cm.evict("light"); cm.evict("dense"); cm.evict("follow")
    # tables inside the load when deferral is switched off
    os.environ["ICICLE_SNARK_DEFER_TABLES"] = "0"
    try:
        cm.load("n", zkey, wait_tables=False)
        assert cm.tables_ready("n")
        pj, qj, _ = cm.prove_mem("n", wtns, 9, 4)
        assert json.loads(pj) == want[(9, 4)][0]
    finally:
        del os.environ["ICICLE_SNARK_DEFER_TABLES"]
    cm.close()
    K.release_domain()


def test_cold_pipeline_first_proof_while_the_key_uploads(gpu, O, S, tmp_path):
    """groth16_prove on a key that is not cached (one device): the cache entry is built with its sections still crossing PCIe and the
    first proof is enqueued behind the stages of that upload (csrc/prover/prover.cpp: cold_prove; prover_internal.h: ColdFeed).
    The proof is valid, public.json is the oracle's, the entry the pipeline left behind proves bit-identically to the oracle at
    fixed (r, s) in both layouts, ICICLE_SNARK_COLD_PIPELINE=0 (load, then prove) gives the same, a witness that does not fit
    and a coefficient record outside the domain are diagnosed as before, and a key whose upload failed is not left in the cache."""
    K = gpu
    B = importlib.import_module("bench")
    N = 100_000
    n = 1 << 17
    K.release_domain()
    K.initialize_domain(K.get_root_of_unity(n))
    zkey, vk = S.setup_squaring_chain(N, B.GpuVec(K), _fbm(K), points_to_mont=B._to_mont(K))
    K.release_domain()
    wtns = S.write_wtns(S.squaring_chain_witness(N))
    vkj = S.vk_to_json(vk)
    cache = O.build_cache(O.parse_zkey(zkey))
    want = O.groth16_prove(zkey, wtns, 5, 6, cache=cache)
    wp = tmp_path / "w.wtns"
    wp.write_bytes(wtns)
    pp, qp = tmp_path / "proof.json", tmp_path / "public.json"
    cm = K.CacheManager()
    for rep, env in enumerate(({}, {"ICICLE_SNARK_COLD_PIPELINE": "0"}, {"ICICLE_SNARK_TABLES": "0"})):
        zp = tmp_path / f"c{rep}.zkey"
        zp.write_bytes(zkey)
        key = f"{zp}_HIP"
        os.environ.update(env)
        try:
            assert not cm.contains(key)
            cm.prove_files(str(wp), str(zp), str(pp), str(qp))            # nothing cached: upload and first proof overlap
        finally:
            for k in env:
                del os.environ[k]
        assert cm.contains(key)
        assert json.loads(qp.read_text()) == want[1]
        assert K.groth16_verify_json(pp.read_text(), qp.read_text(), vkj), rep
        pj, qj, _ = cm.prove_mem(key, wtns, 5, 6)                         # classic layout, on what the pipeline uploaded
        assert json.loads(pj) == want[0] and json.loads(qj) == want[1], rep
        if "ICICLE_SNARK_TABLES" not in env:
            assert cm.tables_ready(key, wait=True)
            pj, qj, _ = cm.prove_mem(key, wtns, 5, 6)                     # … and on the tables built from it
            assert json.loads(pj) == want[0], rep
        cm.prove_files(str(wp), str(zp), str(pp), str(qp))                # cached now
        assert K.groth16_verify_json(pp.read_text(), qp.read_text(), vkj), rep
        cm.evict(key)
    # a witness that does not fit the key: refused with the reference's message, before or after the key is loaded
    zp = tmp_path / "short.zkey"
    zp.write_bytes(zkey)
    short = tmp_path / "short.wtns"
    short.write_bytes(S.write_wtns(S.squaring_chain_witness(N)[:-1]))
    for rep in range(2):
        with pytest.raises(K.ProverError, match="witness"):
            cm.prove_files(str(short), str(zp), str(pp), str(qp))
    cm.prove_files(str(wp), str(zp), str(pp), str(qp))
    assert K.groth16_verify_json(pp.read_text(), qp.read_text(), vkj)
    cm.evict(f"{zp}_HIP")
    # a coefficient record that points outside the domain is found by the CSR build INSIDE the upload task: the prove fails with
    # that message and the half-uploaded key does not stay in the cache
    (off, _), = O.read_sections(zkey, b"zkey")[4]
    bad = bytearray(zkey)
    bad[off + 4 + 3 * 44 + 4: off + 4 + 3 * 44 + 8] = (1 << 20).to_bytes(4, "little")
    bp = tmp_path / "bad.zkey"
    bp.write_bytes(bytes(bad))
    for rep in range(2):
        with pytest.raises(K.ProverError, match="coefficient 3 out of range"):
            cm.prove_files(str(wp), str(bp), str(pp), str(qp))
        assert not cm.contains(f"{bp}_HIP")
    # a key cut short inside its last section, and one that is not a key at all
    cut = tmp_path / "cut.zkey"
    cut.write_bytes(zkey[:len(zkey) - 4096])
    junk = tmp_path / "junk.zkey"
    junk.write_bytes(b"zkey" + bytes(4096))
    for p in (cut, junk):
        with pytest.raises(K.ProverError):
            cm.prove_files(str(wp), str(p), str(pp), str(qp))
        assert not cm.contains(f"{p}_HIP")
    # the golden key (eight wires) through the same entry point
    g = load_golden("groth16.json")
    gz, gw = tmp_path / "g.zkey", tmp_path / "g.wtns"
    gz.write_bytes(base64.b64decode(g["zkey"]))
    gw.write_bytes(base64.b64decode(g["wtns"]))
    cm.prove_files(str(gw), str(gz), str(pp), str(qp))
    assert json.loads(qp.read_text()) == g["cases"][0]["public"]
    v = g["vk"]
    gvk = dict(vk_alpha_1=unhex(v["vk_alpha_1"], 2, 4), vk_beta_2=unhex(v["vk_beta_2"], 4, 4), vk_gamma_2=unhex(v["vk_gamma_2"], 4, 4),
               vk_delta_2=unhex(v["vk_delta_2"], 4, 4), IC=[unhex(p, 2, 4) for p in v["IC"]], n_public=len(v["IC"]) - 1)
    assert K.groth16_verify_json(pp.read_text(), qp.read_text(), S.vk_to_json(gvk))
    # and the good key still proves after all of that
    zp = tmp_path / "again.zkey"
    zp.write_bytes(zkey)
    cm.prove_files(str(wp), str(zp), str(pp), str(qp))
    assert K.groth16_verify_json(pp.read_text(), qp.read_text(), vkj)
    cm.close()
    K.release_domain()


def test_two_threads_prove_uncached_keys_through_one_manager(gpu, S, tmp_path):
    """Two host threads call groth16_prove for DIFFERENT keys that are not cached, through one CacheManager, again and again
    (evicting in between): cold pipelines, deferred table builds and adoptions of two keys interleave — every proof verifies and
    every public.json is its key's."""
    import threading
    K = gpu
    B = importlib.import_module("bench")
    keys = []
    for N in (40_000, 90_000):
        n = 1
        while n < N + 2:
            n <<= 1
        K.release_domain()
        K.initialize_domain(K.get_root_of_unity(n))
        zkey, vk = S.setup_squaring_chain(N, B.GpuVec(K), _fbm(K), points_to_mont=B._to_mont(K))
        K.release_domain()
        zp, wp = tmp_path / f"k{N}.zkey", tmp_path / f"k{N}.wtns"
        zp.write_bytes(zkey)
        wp.write_bytes(S.write_wtns(S.squaring_chain_witness(N)))
        keys.append((N, str(zp), str(wp), S.vk_to_json(vk), [str(pow(3, 1 << N, S.R_MOD))]))
    cm = K.CacheManager()
    errors = []

    def run(k):
        N, zp, wp, vkj, public = keys[k]
        pp, qp = str(tmp_path / f"p{k}.json"), str(tmp_path / f"q{k}.json")
        try:
            for it in range(6):
                cm.prove_files(wp, zp, pp, qp)
                pj, qj = open(pp).read(), open(qp).read()
                if json.loads(qj) != public or not K.groth16_verify_json(pj, qj, vkj):
                    errors.append((k, it, "bad proof"))
                if it % 3 == 1:
                    cm.evict(f"{zp}_HIP")           # (possibly in the middle of its table build)
        except Exception as e:                      # noqa: BLE001 — collected, the main thread asserts
            errors.append((k, repr(e)))

    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors

    # … and the SAME uncached key from two threads at once: one of them runs the cold pipeline, the other finds the entry afterwards
    def same(i):
        N, zp, wp, vkj, public = keys[1]
        pp, qp = str(tmp_path / f"sp{i}.json"), str(tmp_path / f"sq{i}.json")
        try:
            for it in range(3):
                cm.prove_files(wp, zp, pp, qp)
                if json.loads(open(qp).read()) != public or not K.groth16_verify_json(open(pp).read(), open(qp).read(), vkj):
                    errors.append(("same", i, it))
        except Exception as e:                      # noqa: BLE001
            errors.append(("same", i, repr(e)))

    for rnd in range(3):
        cm.evict(f"{keys[1][1]}_HIP")
        ts = [threading.Thread(target=same, args=(i,)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    assert not errors, errors
    cm.close()
    K.release_domain()


def test_deferred_table_build_waits_for_the_cold_upload(gpu, S, tmp_path):
    """The worker that builds a key's fixed-base tables reads the base arrays: inside a cold prove (sections still crossing PCIe) it
    must not start before they have landed, whatever its grace time says.  ICICLE_SNARK_TABLE_GRACE_MS=0 makes it want to start at
    once; 800 k constraints make the upload (≈ 15 ms) outlast the worker's start-up.  Every proof — the cold one, the ones on the
    adopted tables — passes the pairing check (a build from half-uploaded bases gave tables, and proofs, that do not)."""
    K = gpu
    B = importlib.import_module("bench")
    N = 800_000
    K.release_domain()
    K.initialize_domain(K.get_root_of_unity(1 << 20))
    zkey, vk = S.setup_squaring_chain(N, B.GpuVec(K), _fbm(K), points_to_mont=B._to_mont(K))
    K.release_domain()
    vkj = S.vk_to_json(vk)
    zp, wp, pp, qp = (str(tmp_path / x) for x in ("c.zkey", "w.wtns", "proof.json", "public.json"))
    open(zp, "wb").write(zkey)
    open(wp, "wb").write(S.write_wtns(S.squaring_chain_witness(N)))
    del zkey
    public = [str(pow(3, 1 << N, S.R_MOD))]
    cm = K.CacheManager()
    os.environ["ICICLE_SNARK_TABLE_GRACE_MS"] = "0"
    try:
        for rep in range(3):
            cm.prove_files(wp, zp, pp, qp)                               # cold: upload, first proof and (held back) table worker
            assert json.loads(open(qp).read()) == public
            assert K.groth16_verify_json(open(pp).read(), open(qp).read(), vkj), rep
            assert cm.tables_ready(f"{zp}_HIP", wait=True)
            for _ in range(2):
                cm.prove_files(wp, zp, pp, qp)                           # on the adopted tables
                assert K.groth16_verify_json(open(pp).read(), open(qp).read(), vkj), rep
            cm.evict(f"{zp}_HIP")
    finally:
        del os.environ["ICICLE_SNARK_TABLE_GRACE_MS"]
    cm.close()
    K.release_domain()


def test_two_threads_prove_with_one_cached_key(gpu, cm, O, S):
    """Two host threads call groth16_prove_mem on the SAME cached key at once (BASELINE config 5 is a repeated-prove loop; round-5
    verdict item 5): the manager admits one prove at a time — the key has one set of streams and work buffers — so the calls must
    neither deadlock nor mix their witnesses: every proof with fixed (r, s) is the oracle's for THAT thread's witness."""
    import threading
    K = gpu
    N = 6000
    r1, w_a = S.squaring_chain(N)
    zkey, _ = S.setup(r1, _fbm(K), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
    _, w_b = S.squaring_chain(N, a=5)           # the same circuit on another input
    wt = [S.write_wtns(w_a), S.write_wtns(w_b)]
    cm.load("twothreads", zkey)
    cache = O.build_cache(O.parse_zkey(zkey))
    want = [[O.groth16_prove(zkey, wt[t], 3 + t, 5 + i, cache=cache) for i in range(2)] for t in range(2)]
    errs = []

    def loop(t):
        try:
            K.set_device("HIP", 0)
            for rep in range(6):
                i = rep % 2
                pj, qj, _ = cm.prove_mem("twothreads", wt[t], 3 + t, 5 + i)
                if json.loads(pj) != want[t][i][0] or json.loads(qj) != want[t][i][1]:
                    errs.append((t, rep))
                cm.prove_mem("twothreads", wt[t])   # a randomly blinded one in between
        except Exception as e:   # noqa: BLE001
            errs.append((t, repr(e)))
    th = [threading.Thread(target=loop, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=300)
    assert not any(x.is_alive() for x in th), "a prove call did not return"
    assert not errs, errs
    cm.evict("twothreads")
