"""Distributed QAP front end (tests/dist_qap_model.py): the three-stage decomposition with two all-to-alls equals the
oracle's construct_r1cs, (a) simulated in one process for G = 2, 4, 8 and (b) run by two gloo processes that really exchange
their blocks; the model's spmv, its tabulated stage 2 and its buffer codecs; and the row-shape circuit of tests/dist_shapes.py.
CPU only — the HIP kernels of the same stages are compared with this model buffer by buffer in tests/test_gpu_dist_shapes.py and
with the single-GPU prover in tests/test_gpu_dist.py."""
import importlib
import json
import os
import random
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import dist_qap_model as D
import dist_shapes as M


def _reference_h(O, rows, logn):
    """d = NTT(coset(iNTT(A))) ∘ NTT(coset(iNTT(B))) − NTT(coset(iNTT(C'))) with the oracle's transforms (domain 2n)"""
    R, n = O.R_MOD, 1 << logn
    w2n = O.fr_omega(logn + 1)
    ev = []
    for x in rows:
        a = O.arr_to_ints(O.fr_ntt(O.ints_to_arr(x), True, domain_log=logn + 1))
        a = [v * pow(w2n, k, R) % R for k, v in enumerate(a)]
        ev.append(O.arr_to_ints(O.fr_ntt(O.ints_to_arr(a), False, domain_log=logn + 1)))
    return [(a * b - c) % R for b, a, c in zip(*ev)]


def _ntt_fns(O, logm, logn):
    inv = lambda v: O.arr_to_ints(O.fr_ntt(O.ints_to_arr(v), True, domain_log=logn + 1)) if logm else list(v)
    fwd = lambda v: O.arr_to_ints(O.fr_ntt(O.ints_to_arr(v), False, domain_log=logn + 1)) if logm else list(v)
    return inv, fwd


@pytest.mark.parametrize("logn,G", [(5, 2), (6, 4), (7, 8), (6, 8)])
def test_three_stage_decomposition_equals_construct_r1cs(O, logn, G):
    n, m, mb = 1 << logn, (1 << logn) // G, (1 << logn) // (G * G)
    rnd = random.Random(7 * logn + G)
    rows = [[rnd.randrange(O.R_MOD) for _ in range(n)] for _ in range(3)]     # [B | A | C'] evaluations on the domain
    want = _reference_h(O, rows, logn)
    wn, w2n = O.fr_omega(logn), O.fr_omega(logn + 1)
    inv, fwd = _ntt_fns(O, m.bit_length() - 1, logn)
    Y = [D.stage1([x[r::G] for x in rows], r, G, n, wn, inv) for r in range(G)]
    Z = []
    for b in range(G):      # exchange 1: rank b receives block b of every source
        recv = [[Y[j1][row][b * mb:(b + 1) * mb] for j1 in range(G)] for row in range(3)]
        Z.append(D.stage2(recv, b, G, n, wn, w2n))
    for r in range(G):      # exchange 2: rank r receives its Z_r block from every rank b, in block order
        z_rows = [sum((Z[b][row][r] for b in range(G)), []) for row in range(3)]
        assert D.stage3(z_rows, fwd) == want[r::G], (logn, G, r)


_WORKER = r'''
import importlib, os, random, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "oracle")); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import torch, torch.distributed as dist
import oracle as O
from test_dist_qap import _reference_h, _ntt_fns
import dist_qap_model as D
dist.init_process_group("gloo")
r, G = dist.get_rank(), dist.get_world_size()
logn = 6; n, m, mb = 1 << logn, (1 << logn) // G, (1 << logn) // (G * G)
rnd = random.Random(99)
rows = [[rnd.randrange(O.R_MOD) for _ in range(n)] for _ in range(3)]     # same on every rank (the witness is)
inv, fwd = _ntt_fns(O, m.bit_length() - 1, logn)
wn, w2n = O.fr_omega(logn), O.fr_omega(logn + 1)
def a2a(chunks):   # chunks[peer] = list of ints for that peer; returns what every peer sent to this rank (gloo has no all_to_all: gather + pick)
    mine = torch.from_numpy(O.ints_to_arr([v for c in chunks for v in c]).view("int64").copy())
    outs = [torch.empty_like(mine) for _ in range(G)]
    dist.all_gather(outs, mine)
    per = len(chunks[0])
    return [O.arr_to_ints(o.numpy().view("uint64").reshape(-1, 4))[r * per:(r + 1) * per] for o in outs]
Y = D.stage1([x[r::G] for x in rows], r, G, n, wn, inv)
recv = [a2a([Y[row][b * mb:(b + 1) * mb] for b in range(G)]) for row in range(3)]          # recv[row][j1]
Z = D.stage2(recv, r, G, n, wn, w2n)                                                          # Z[row][i1]
z_rows = [sum(a2a([Z[row][i1] for i1 in range(G)]), []) for row in range(3)]                  # blocks in source order
got = D.stage3(z_rows, fwd)
assert got == _reference_h(O, rows, logn)[r::G]
dist.barrier(); dist.destroy_process_group()
print("DIST_QAP_OK", r)
'''


def test_two_gloo_ranks_exchange_their_blocks():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-c", _WORKER % {"root": ROOT}]
    # torch.distributed.run has no -c: run the worker from a temp file
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".py", delete=False) as f:
        f.write(_WORKER % {"root": ROOT})
        path = f.name
    try:
        cmd = cmd[:-2] + [path]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="2"))
        assert out.returncode == 0 and out.stdout.count("DIST_QAP_OK") == 2, out.stdout[-2000:] + out.stderr[-3000:]
    finally:
        os.unlink(path)


def test_spmv_rows_through_the_three_stages_equal_construct_r1cs(O, S):
    """the model additions on a random small R1CS (domain 2^6, G = 4): spmv_rows → stage 1 → exchange → tabulated stage 2 →
    exchange → stage 3 (dist_shapes.model_round) gives A·B − C' of the same rows on the coset, residue class by residue class"""
    logn, G = 6, 4
    r1, w = S.random_circuit(55, 3, 6, bit_fraction=0.3)
    ks = S.key_scalars(r1)
    assert ks["n"] == 1 << logn
    rows = D.spmv_rows(ks["coeffs"], w, ks["n"])
    # the rows are what they claim to be: row j of A (of B) applied to the witness, the public-binding rows included
    a = [0] * ks["n"]
    for (j, i, v) in r1.A:
        a[j] = (a[j] + v * w[i]) % O.R_MOD
    for s in range(r1.n_public + 1):
        a[r1.n_constraints + s] = w[s]
    assert rows[1] == a and rows[2] == [x * y % O.R_MOD for x, y in zip(rows[1], rows[0])] and any(rows[0]) and rows[0] != rows[1]
    want = _reference_h(O, rows, logn)
    _, _, E = M.model_round(O, rows, logn, G)
    for r in range(G):
        assert E[r] == want[r::G], r
    # a record given twice adds twice
    dup = D.spmv_rows([(0, 1, 2, 5), (1, 1, 0, 3), (0, 1, 2, O.R_MOD - 1)], [1, 0, 7], 2)
    assert dup == [[0, 3], [0, 4 * 7], [0, 3 * 4 * 7]]


@pytest.mark.parametrize("logn,G", [(5, 2), (6, 4), (7, 8), (6, 8)])
def test_tabulated_stage2_equals_the_pow_per_term_one(O, logn, G):
    n, mb = 1 << logn, (1 << logn) // (G * G)
    rnd = random.Random(31 * logn + G)
    wn, w2n = O.fr_omega(logn), O.fr_omega(logn + 1)
    pw = D.power_table(w2n, 2 * n)
    assert pw[1] == w2n and pw[2] == wn and pw[n] == O.R_MOD - 1 and pw[-1] * w2n % O.R_MOD == 1
    for b in range(G):
        recv = [[[rnd.randrange(O.R_MOD) for _ in range(mb)] for _ in range(G)] for _ in range(3)]
        assert D.stage2_tab(recv, b, G, n, pw) == D.stage2(recv, b, G, n, wn, w2n), b


def test_buffer_codecs_round_trip(O):
    xs = [0, 1, O.R_MOD - 1, (1 << 253) + 1, 0x0123456789ABCDEF << 64]
    raw = D.ints_to_fe_bytes(xs)
    assert len(raw) == 32 * len(xs) and raw == O.ints_to_arr(xs).tobytes() and D.fe_bytes_to_ints(raw) == xs
    R2 = (1 << 512) % O.R_MOD
    rec = D.section4_records([0, 1], [7, 8], [3, 4], O.ints_to_arr([5 * R2 % O.R_MOD, (O.R_MOD - 2) * R2 % O.R_MOD]))
    assert rec == [(0, 7, 3, 5), (1, 8, 4, O.R_MOD - 2)]


@pytest.fixture(scope="module")
def shapes(S):
    r1, w, starts = M.row_shape_circuit(S)
    return r1, w, starts, S.key_scalars(r1)


def test_row_shape_circuit_holds_every_shape_in_every_residue_class(S, shapes):
    """the builder of tests/dist_shapes.py, read back from what setup() writes into section 4 (key_scalars' coeffs)"""
    r1, w, starts, ks = shapes
    R, nc, n = S.R_MOD, r1.n_constraints, ks["n"]
    assert n == 1 << 13 and nc + r1.n_public + 1 <= n and nc % 8 == 0
    per = {}                                                  # (matrix, row) → [(wire, value)]
    for (mat, row, wire, v) in ks["coeffs"]:
        per.setdefault((mat, row), []).append((wire, v))
    lens = lambda j: (len(per.get((0, j), [])), len(per.get((1, j), [])))
    mult = lambda j, mat: sorted(sum(1 for x, _ in per.get((mat, j), []) if x == y) for y in {x for x, _ in per.get((mat, j), [])})
    for c in range(8):
        rows = [j for j in range(c, nc, 8)]
        have = {lens(j) for j in rows}
        for L in M.LONG:
            assert (L, 1) in have and (1, L) in have, (c, L)
        assert (0, 2) in have and (2, 0) in have and (0, 0) in have, c
        twice = [j for j in rows if mult(j, 0) == [1, 1, 2]]
        thrice = [j for j in rows if mult(j, 1) == [1, 3]]
        assert twice and thrice, c
        for j, mat in ((twice[0], 0), (thrice[0], 1)):      # the repeated record carries different values
            x = max({x for x, _ in per[mat, j]}, key=lambda y: sum(1 for z, _ in per[mat, j] if z == y))
            vals = [v for z, v in per[mat, j] if z == x]
            assert len(set(vals)) == len(vals) > 1, (j, vals)
        coeffs = {v for j in rows for mat in (0, 1) for _, v in per.get((mat, j), [])}
        assert {1, R - 1, R - 2, (1 << 253) + 1} <= coeffs, c
        long_rows = [j for j in rows if max(lens(j)) >= 63]
        for j in long_rows:
            side = per[0, j] if lens(j)[0] >= 63 else per[1, j]
            assert side[0][0] == 0 and side[-1][0] == r1.n_vars - 1 and len({x for x, _ in side}) == len(side), j
    assert lens(0) == (300, 1) and lens(nc - 1) == (1, 300)
    # A and B differ on almost every row: swapping the two slots changes far more than the public-binding rows
    rows3 = D.spmv_rows(ks["coeffs"], w, n)
    assert sum(1 for x, y in zip(rows3[0], rows3[1]) if x != y) > nc // 2
    assert [lens(nc + s) for s in range(r1.n_public + 1)] == [(1, 0)] * (r1.n_public + 1)
    # and the witness satisfies the system: C's wire of row j is the product of the two rows
    first_out = 1 + r1.n_public
    assert all(w[first_out + j] == rows3[2][j] for j in range(nc)) and sum(1 for j in range(nc) if rows3[2][j]) > nc // 2


def test_row_shape_circuit_proof_verifies(K, S, O, shapes):
    """the oracle's proof of the row-shape circuit passes the pairing check (the oracle has no verifier of its own: the library's
    host check, and the reference's where oracle/_ref is built)"""
    r1, w, _, _ = shapes
    Gaff = {g: O.ec_to_affine(g, O.ec_generator(g)) for g in ("g1", "g2")}
    zkey, vk = S.setup(r1, lambda g, sc: O.fixed_base_mul(g, Gaff[g], sc), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
    proof, public = O.groth16_prove(zkey, S.write_wtns(w), 21, 34)
    assert public == [str(v) for v in w[1:1 + r1.n_public]]
    assert K.groth16_verify_json(json.dumps(proof), json.dumps(public), S.vk_to_json(vk)) is True
    bad = [str(int(public[0]) ^ 1)] + public[1:]
    assert K.groth16_verify_json(json.dumps(proof), json.dumps(bad), S.vk_to_json(vk)) is False
    import ref
    if ref.available():
        assert ref.groth16_verify(proof, public, vk) and not ref.groth16_verify(proof, bad, vk)
