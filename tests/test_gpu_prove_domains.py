"""The QAP front end at EVERY domain size (needs an MI355X): proofs bit-identical to the oracle pipeline for domain logs 2 … 22.

csrc/prover/prover.cpp: enqueue_front_end switches on the domain size n — below 2^12 it runs bn254_ntt, the coset sweep,
bn254_ntt and the final sweep; from 2^12 on (ntt_fusable) the inverse transform carries 1/n and the coset keys in its last pass
and the forward transform ends in the A·B − C' epilogue — and every n has its own pass plan and bound plan underneath
(csrc/ntt.hip, table in DESIGN.md §6).  A strided H shard runs the same choice on m = n / count.  Squaring chains at the fullest
fill of the domain (N = 2^k − 2 constraints) and at the emptiest (N = 2^(k−1) − 1: the padding rows of the spmv and the all-zero
tail of the transforms meet), stand-in circuits with rows of 1 – 8 entries, the same front end on the 8×32-bit kernels, and
the strided H shards at and below the fusable size."""
import importlib
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
RS = (0x1234567890ABCDEF << 100, 987654321)      # fixed blinding: a value above 2^160 and a small one


@pytest.fixture(scope="module")
def cm(gpu, O):
    O.calibrate_threads()
    gpu.release_domain()
    c = gpu.CacheManager()
    yield c
    c.close()
    gpu.release_domain()


def _chain_key(K, S, O, N):
    """(zkey, wtns) of the squaring chain with N constraints, built the way the other tests build theirs: the generic Python
    setup for small N, the vectorised one on the device for large"""
    if N + 2 <= 1 << 13:
        r1, w = S.squaring_chain(N)
        zkey, _ = S.setup(r1, lambda g, sc: K.generator_mul(g, sc), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
        return zkey, S.write_wtns(w)
    return importlib.import_module("bench").make_inputs(K, S, N)


def _prove_equals_oracle(K, cm, O, zkey, wtns, k, key):
    cm.load(key, zkey)
    assert cm.info(key).domain_size == 1 << k
    pj, qj, _ = cm.prove_mem(key, wtns, *RS)
    cm.evict(key)
    proof, public = O.groth16_prove(zkey, wtns, *RS)
    assert json.loads(pj) == proof and json.loads(qj) == public, key


def _chain_fills(K, cm, O, S, k):
    """fullest fill for every k; emptiest fill too up to 2^19; emptiest alone at 2^21 and 2^22 (the oracle's time)"""
    fills = []
    if k <= 20:
        fills.append(("full", (1 << k) - 2))
    if k <= 19 or k >= 21:
        fills.append(("empty", (1 << (k - 1)) - 1))
    for name, N in fills:
        zkey, wtns = _chain_key(K, S, O, N)
        _prove_equals_oracle(K, cm, O, zkey, wtns, k, f"chain{k}{name}")


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7, 8, 9, 10, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22], ids=lambda v: f"log{v:02d}")
def test_front_end_at_every_domain_size(gpu, cm, O, S, k):
    """8×32-bit transforms up to 2^10; fused radix-2^29 front end from 2^13: 13 [8,5], 14 [8,6] (xcd_batch), 15 [8,7] and
    16 [8,8] (shrink_last), 17 [6,6,5] … 22 [8,8,6] (3-pass)"""
    _chain_fills(gpu, cm, O, S, k)


def test_front_end_at_2p11_the_last_size_that_is_not_fused(gpu, cm, O, S):
    """first radix-2^29 plan ([6,5], one tile per row); transforms, coset sweep and final sweep as separate launches"""
    _chain_fills(gpu, cm, O, S, 11)


def test_front_end_at_2p12_the_first_fused_size(gpu, cm, O, S):
    """ntt_fusable: [6,6], two tiles per row; scale_tab in the inverse's last pass, the A·B − C' epilogue in the forward's"""
    _chain_fills(gpu, cm, O, S, 12)


def _standin_key(K, S, k):
    """a synth.standin_circuit key of domain 2^k (7/8 full): rows of 1 – 8 entries, coefficients −1 and up to 2^16"""
    B = importlib.import_module("bench")
    nc = (1 << k) - (1 << (k - 3))
    r, w = S.standin_circuit(nc, 2, 40, seed=k)
    K.release_domain()
    K.initialize_domain(K.get_root_of_unity(1 << k))
    zkey, _ = S.setup_sparse(r, B.GpuVec(K), lambda g, sc: K.generator_mul(g, sc), points_to_mont=B._to_mont(K))
    K.release_domain()
    return zkey, S.write_wtns(w)


@pytest.mark.parametrize("k", [11, 12, 14, 18], ids=lambda v: f"log{v:02d}")
def test_front_end_standin_circuit(gpu, cm, O, S, k):
    zkey, wtns = _standin_key(gpu, S, k)
    _prove_equals_oracle(gpu, cm, O, zkey, wtns, k, f"standin{k}")


def test_front_end_on_the_8x32_kernels_behind_the_switch(gpu):
    """ICICLE_SNARK_NTT29=0 (read once per process) — and a domain whose Montgomery-261 twiddle table could not be allocated —
    puts the prover's transforms on the 8×32-bit kernels: ntt_pass_kernel<true> (the A·B − C' epilogue) and `scale_tab` on that
    path run nowhere else.  One child process proves the domain logs 11 (not fused), 12, 13, 16 (2-pass), 18 (the last 2-pass
    size of that plan), 19 and 20 (3-pass) and compares each proof with the oracle's."""
    code = r'''
import importlib, json, os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "oracle"))
import oracle as O
K = importlib.import_module("icicle-snark_amd"); S = importlib.import_module("icicle-snark_amd.synth")
bench = importlib.import_module("bench")
assert os.environ["ICICLE_SNARK_NTT29"] == "0"
K.set_device("HIP", 0)
O.calibrate_threads()
cm = K.CacheManager()
for k in (11, 12, 13, 16, 18, 19, 20):
    zkey, wtns = bench.make_inputs(K, S, (1 << k) - 2)
    cm.load("k", zkey)
    assert cm.info("k").domain_size == 1 << k
    pj, qj, _ = cm.prove_mem("k", wtns, %d, %d)
    cm.evict("k")
    proof, public = O.groth16_prove(zkey, wtns, %d, %d)
    assert json.loads(pj) == proof and json.loads(qj) == public, k
    print("ok", k, flush=True)
cm.close()
K.release_domain()
print("FRONT_END_8X32_OK")
''' % (ROOT, ROOT, RS[0], RS[1], RS[0], RS[1])
    env = dict(os.environ, ICICLE_SNARK_NTT29="0", ICICLE_SNARK_QUIET="1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=1500, env=env)
    assert out.returncode == 0 and "FRONT_END_8X32_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


@pytest.mark.parametrize("k,count", [(13, 8), (13, 4), (12, 2), (12, 8), (14, 4)],
                         ids=["m1024_2p13_over_8", "m2048_2p13_over_4", "m2048_2p12_over_2", "m512_2p12_over_8_range_sharded", "m4096_2p14_over_4_fused"])
def test_strided_h_shards_at_and_below_the_fusable_size(gpu, cm, O, S, k, count):
    """h_strided (csrc/prover/cache.cpp) holds when m = n / count ≥ 1024.  With m = 1024 or 2048 the shard's forward transform is
    not fusable: bn254_ntt + qap_final on d_fold.  m = 512 falls back to range shards of H; m = 4096 takes the fused transform
    (the control).  In every case the summed partial commitments, assembled with the full key, are the unsharded proof, and that
    proof is the oracle's."""
    K = gpu
    N = (1 << k) - (1 << (k - 2))
    zkey, wtns = _chain_key(K, S, O, N)
    key = f"h{k}_{count}"
    cm.load(key, zkey)
    assert cm.info(key).domain_size == 1 << k
    want, public, _ = cm.prove_mem(key, wtns, 21, 34)
    proof, pub = O.groth16_prove(zkey, wtns, 21, 34)
    assert json.loads(want) == proof and json.loads(public) == pub
    blocks = b""
    for rank in range(count):
        cm.load(f"{key}_{rank}", zkey, shard_rank=rank, shard_count=count)
        blk, _ = cm.commitments(f"{key}_{rank}", wtns)
        blocks += blk
        cm.evict(f"{key}_{rank}")
    got, _ = cm.assemble(key, wtns, K.sum_commitments(blocks, count), 21, 34)
    assert got == want
    cm.evict(key)
