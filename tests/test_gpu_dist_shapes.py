"""The SHARDED QAP front end at every size, shard count and row shape (needs an MI355X; shard caches in one process play the
ranks, as in tests/test_gpu_dist.py).  Every comparison is of exact integers or bytes.

n = 2^k is the key's domain, G the shard count, m = n / G what one rank transforms, N the resident NTT domain.  "stride" below
is what the kernels multiply a twiddle index by: N / 2n for qap_coset_fold3 (tw_scale) and the scaled keys, N / n and N / 2n for
qap_dist_tw1 and qap_dist_mid (sn, sn / 2).  With N = 2n, the only case the suite had, they are 1, 2 and 1.

Which test runs which kernel (csrc/prover/qap.hip; call sites in csrc/prover/prover.cpp shard_dist_stage1 / shard_dist_stage2 /
enqueue_front_end and csrc/prover/cache.cpp build_cache):

  qap_spmv_strided     test_stages_equal_the_integer_model: (m, G) = (2^12, 2) on the row-shape circuit (rows of 0 – 300 entries,
                       A ≠ B, repeated records, coefficients r − 1, r − 2, 2^253 + 1), (2^13, 2), (2^12, 4), (2^13, 4), (2^12, 8)
                       on stand-in circuits (rows of 1 – 8 entries) — its output is compared through stage 1, element by element;
                       test_matrix_end_to_end: squaring chains, m = 2^12 … 2^16 with G = 2, 4, 8 and (2^17, 2);
                       test_standin_circuit_end_to_end (2^13, 8)
  qap_dist_tw1         the same tests (the table is built by a shard's first stage 1) at N / n = 2;
                       test_resident_domain_larger_than_2n[13-2]: fresh shard caches under N = 16n, N / n = 16
  qap_dist_mid<2|4|8>  test_stages_equal_the_integer_model: <2> at m = 2^12, 2^13; <4> at 2^12, 2^13; <8> at 2^12 — every element of
                       every rank's send buffer; test_matrix_end_to_end: each of <2>, <4>, <8> at m = 2^12 … 2^16, <2> at 2^17;
                       sn = 2 throughout, sn = 16 (sn / 2 = 8) in test_resident_domain_larger_than_2n[13-2]
  size-m ntt_fused     inverse with the scale table of qap_dist_tw1, batch 3, and forward with the A·B − C' epilogue: m = 2^12 [6,6],
                       2^13 [8,5] (both also stage by stage), 2^14, 2^15, 2^16 (two passes) and 2^17 (three passes) in
                       test_matrix_end_to_end; m = 2^12 inside a domain of 2^17 = 32m in test_resident_domain_larger_than_2n[13-2]
  qap_coset_fold3      replicated path of test_matrix_end_to_end (every (m, G) above, tw_scale 1); G = 2, 4, 8 on the row-shape
                       circuit in test_row_shapes_replicated_fold; G = 16 at m = 2^10 (stand-in; bn254_ntt + qap_final follow) and
                       m = 2^12 (chain; fused) in test_strided_fold_beyond_eight_shards; tw_scale 8 in
                       test_resident_domain_larger_than_2n[13-2]; after another witness's Z rows in test_stale_state_between_witnesses
  qap_gather_strided   every strided shard load above: stride 2, 4, 8 and 16, every first < stride
  qap_spmv             the row-shape circuit unsharded (the same da / db lock-step loop), against the oracle
  qap_coset_mul3       test_resident_domain_larger_than_2n[10-1]: key_stride 8 (n = 2^10, N = 2^14)
  ntt_build_scaled_keys  test_resident_domain_larger_than_2n[13-1]: tw_stride 8 (a key loaded under N = 16n)
"""
import importlib
import json

import pytest

import dist_qap_model as D
import dist_shapes as M

pytestmark = pytest.mark.gpu
RS = (0x1234567890ABCDEF << 100, 987654321)      # fixed blinding: a value above 2^160 and a small one
ROW_NAMES = ("B", "A", "A∘B")


class _Key:
    """one proving key with a witness: the bytes, and lazily the single-device proof, the oracle's, and the integer model"""

    def __init__(self, K, O, cm, name, k, zkey, wtns):
        self.K, self.O, self.cm, self.name, self.k, self.zkey, self.wtns = K, O, cm, name, k, zkey, wtns
        cm.load(name, zkey)
        assert cm.info(name).domain_size == 1 << k, (name, cm.info(name).domain_size)
        self.want, self.public, _ = cm.prove_mem(name, wtns, *RS)
        self._oracle = False
        self._rows = None
        self._model = {}

    def check_oracle(self):
        if not self._oracle:
            proof, public = self.O.groth16_prove(self.zkey, self.wtns, *RS)
            assert json.loads(self.want) == proof and json.loads(self.public) == public, self.name
            self._oracle = True

    def model(self, G):
        """(Y, Z) of dist_shapes.model_round for this key's section 4 and witness"""
        if G not in self._model:
            if self._rows is None:
                z = self.O.parse_zkey(self.zkey)
                w = self.O.arr_to_ints(self.O.parse_wtns(self.wtns)["witness"])
                self._rows = D.spmv_rows(D.section4_records(z["m"], z["c"], z["s"], z["coef"]), w, 1 << self.k)
            self._model[G] = M.model_round(self.O, self._rows, self.k, G)[:2]
        return self._model[G]

    def assemble(self, blocks, count, wtns=None):
        return self.cm.assemble(self.name, wtns or self.wtns, self.K.sum_commitments(blocks, count), *RS)[0]

    def drop(self):
        self.cm.evict(self.name)


class _Keys:
    """the keys of this module, built on first use: up to 2^16 they stay (a few tens of MB each), above that only the latest"""

    def __init__(self, K, O, S, cm):
        self.K, self.O, self.S, self.cm = K, O, S, cm
        self.small, self.big = {}, None

    def get(self, kind, k):
        name = f"{kind}{k}"
        if name in self.small:
            return self.small[name]
        if self.big is not None and self.big.name == name:
            return self.big
        K, O, S = self.K, self.O, self.S
        P = importlib.import_module("test_gpu_prove_domains")
        if kind == "chain":                                   # 7/8 fill of the domain
            zkey, wtns = P._chain_key(K, S, O, (1 << k) - (1 << (k - 3)))
        elif kind == "standin":
            zkey, wtns = P._standin_key(K, S, k)
        else:
            assert (kind, k) == ("shapes", 13)
            r1, w, _ = M.row_shape_circuit(S)
            zkey, _ = S.setup(r1, lambda g, sc: K.generator_mul(g, sc), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
            wtns = S.write_wtns(w)
        if k > 16 and self.big is not None:
            self.big.drop()
            self.big = None
        e = _Key(K, O, self.cm, name, k, zkey, wtns)
        if k <= 16:
            self.small[name] = e
        else:
            self.big = e
        return e


@pytest.fixture(scope="module")
def cm(gpu, O):
    O.calibrate_threads()
    gpu.release_domain()
    c = gpu.CacheManager()
    yield c
    c.close()
    gpu.release_domain()


@pytest.fixture(scope="module")
def keys(gpu, O, S, cm):
    return _Keys(gpu, O, S, cm)


def _load_shards(cm, e, G, tag=""):
    names = [f"{e.name}{tag}/{r}of{G}" for r in range(G)]
    for r, nm in enumerate(names):
        cm.load(nm, e.zkey, shard_rank=r, shard_count=G)
    return names


def _evict(cm, names):
    for nm in names:
        cm.evict(nm)


def _assert_rows(raw, want_rows, where):
    """raw = 3·len(row) elements of a device buffer; want_rows = the model's three rows.  On a mismatch the message names the
    case, the stage, the rank, the row and the first differing index."""
    ln = len(want_rows[0])
    assert len(raw) == 3 * ln * 32, (where, len(raw), ln)
    for row, want in enumerate(want_rows):
        part = raw[row * ln * 32:(row + 1) * ln * 32]
        if part == D.ints_to_fe_bytes(want):
            continue
        got = D.fe_bytes_to_ints(part)
        i = next(i for i in range(ln) if got[i] != want[i])
        bad = sum(1 for x, y in zip(got, want) if x != y)
        raise AssertionError(f"{where} row {row} ({ROW_NAMES[row]}): first differing index {i} of {ln} ({bad} differ): "
                             f"device {got[i]:#066x}, model {want[i]:#066x}")


def _dist_round(K, cm, e, names, wtns, model=None, note=""):
    """one complete distributed round on the shard caches `names` → the concatenated commitment blocks.  With `model` = (Y, Z)
    every element of every rank's two send buffers is compared with it before the exchange that ships it."""
    G = len(names)
    st = [cm.dist_stage1(nm, wtns) for nm in names]
    rows, rb, cb = st[0][2:]
    m = (1 << e.k) // G
    assert rows == 3 and rb == m * 32 and cb == (m // G) * 32 and all(s[2:] == st[0][2:] for s in st)
    if model:
        for r, s in enumerate(st):
            _assert_rows(K.raw_to_host(s[0], rows * rb), model[0][r], f"k={e.k} G={G}{note} stage 1 rank {r}")
    M.exchange(K, [(s[0], s[1]) for s in st], rows, rb, cb)
    st2 = [cm.dist_stage2(nm) for nm in names]
    if model:
        for b, s in enumerate(st2):
            want = [sum(model[1][b][row], []) for row in range(3)]                 # [row][peer i1][m/G], as the buffer lies
            _assert_rows(K.raw_to_host(s[0], rows * rb), want, f"k={e.k} G={G}{note} stage 2 rank {b}")
    M.exchange(K, st2, rows, rb, cb)
    for nm in names:
        cm.dist_exchange_done(nm)
    return b"".join(cm.commitments(nm, None)[0] for nm in names)


def _replicated(cm, names, wtns):
    return b"".join(cm.commitments(nm, wtns)[0] for nm in names)


# ---- 1 (and the stage-by-stage half of 3): every stage buffer against the integer model --------------------------------------------
@pytest.mark.parametrize("k,G,kind", [(13, 2, "shapes"), (14, 2, "standin"), (14, 4, "standin"), (15, 4, "standin"), (15, 8, "standin")],
                         ids=lambda v: str(v))
def test_stages_equal_the_integer_model(gpu, cm, keys, k, G, kind):
    """m = 2^12 ([6,6]) with G = 2, 4, 8 and m = 2^13 ([8,5]) with G = 2, 4: all 3·m elements of every rank's stage-1 and stage-2
    send buffers equal tests/dist_qap_model.py applied to the spmv of the key's section 4 (a plain scatter-add), and the round's
    proof is the single-device one and the oracle's.  The 2^13 key is the row-shape circuit of tests/dist_shapes.py, the others
    stand-in circuits (rows of 1 – 8 entries, A ≠ B)."""
    e = keys.get(kind, k)
    e.check_oracle()
    names = _load_shards(cm, e, G)
    assert all(cm.dist_supported(nm) for nm in names)
    blocks = _dist_round(gpu, cm, e, names, e.wtns, e.model(G))
    assert e.assemble(blocks, G) == e.want, (k, G)
    _evict(cm, names)


# ---- 2: the (m, G) matrix end to end ------------------------------------------------------------------------------------------------
_MATRIX = sorted({(lm + lg, 1 << lg) for lm in range(12, 17) for lg in (1, 2, 3)} | {(18, 2)})
_MATRIX = [c for c in _MATRIX if c not in ((17, 2), (17, 4), (17, 8), (19, 8))]      # tests/test_gpu_dist.py runs these four


@pytest.mark.parametrize("k,G", _MATRIX, ids=lambda v: str(v))
def test_matrix_end_to_end(gpu, cm, keys, k, G):
    """squaring chain at 7/8 fill; m = n / G from 2^12 to 2^16 for G = 2, 4, 8, and (2^17, 2): the distributed path and the
    replicated path, twice each on the same shard caches, sum and assemble to the single-device proof (the oracle's up to 2^16;
    above that tests/test_gpu_prove_domains.py pins the single-device prover to the oracle at the same k)"""
    e = keys.get("chain", k)
    if k <= 16:
        e.check_oracle()
    names = _load_shards(cm, e, G)
    assert all(cm.dist_supported(nm) for nm in names)
    for rep in range(2):
        assert e.assemble(_dist_round(gpu, cm, e, names, e.wtns), G) == e.want, (k, G, "distributed", rep)
    for rep in range(2):
        assert e.assemble(_replicated(cm, names, e.wtns), G) == e.want, (k, G, "replicated", rep)
    _evict(cm, names)


# ---- 3: row shapes ------------------------------------------------------------------------------------------------------------------
def test_row_shapes_unsharded_equal_the_oracle(keys):
    """the row-shape circuit through qap_spmv (the same lock-step loop as qap_spmv_strided) on one device"""
    keys.get("shapes", 13).check_oracle()


@pytest.mark.parametrize("count", [2, 4, 8])
def test_row_shapes_replicated_fold(gpu, cm, keys, count):
    e = keys.get("shapes", 13)
    e.check_oracle()
    names = _load_shards(cm, e, count)
    assert e.assemble(_replicated(cm, names, e.wtns), count) == e.want, count
    _evict(cm, names)


def test_standin_circuit_end_to_end(gpu, cm, keys):
    """(k, G) = (16, 8): rows of 1 – 8 entries at m = 2^13"""
    e = keys.get("standin", 16)
    e.check_oracle()
    names = _load_shards(cm, e, 8)
    assert e.assemble(_dist_round(gpu, cm, e, names, e.wtns), 8) == e.want
    assert e.assemble(_replicated(cm, names, e.wtns), 8) == e.want
    _evict(cm, names)


# ---- 4: strided fold beyond eight shards --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,kind", [(14, "standin"), (16, "chain")], ids=lambda v: str(v))
def test_strided_fold_beyond_eight_shards(gpu, cm, keys, k, kind):
    """sixteen strided shards: m = 2^10 (forward transform not fusable: bn254_ntt + qap_final) and m = 2^12 (fused).  The
    distributed stages stop at eight, so every rank takes the replicated path: qap_coset_fold3 with G = 16."""
    e = keys.get(kind, k)
    e.check_oracle()
    names = _load_shards(cm, e, 16)
    for nm in names:
        assert not cm.dist_supported(nm)
    with pytest.raises(gpu.ProverError, match="not a strided shard of 2, 4 or 8"):
        cm.dist_stage1(names[3], e.wtns)
    assert e.assemble(_replicated(cm, names, e.wtns), 16) == e.want, k
    _evict(cm, names)


# ---- 5: a resident domain larger than 2n --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,G", [(10, 1), (13, 2), (13, 1)], ids=lambda v: str(v))
def test_resident_domain_larger_than_2n(gpu, O, S, keys, k, G):
    """the manager keeps a resident NTT domain that is larger than 2n once it has recorded the key's size: n = 2^10 (unfused:
    qap_coset_mul3), 2^13 unsharded (fused: the scaled keys) and 2^13 over two shards (distributed stages and the replicated fold)
    under N = 2^(k+4) = 8·2n, on entries loaded before the larger domain came (their tables are kept) and on entries loaded
    under it (their tables are built with the stride)"""
    K = gpu
    P = importlib.import_module("test_gpu_prove_domains")
    if k == 13:
        e0 = keys.get("shapes", 13)
        zkey, wtns = e0.zkey, e0.wtns
    else:
        zkey, wtns = P._chain_key(K, S, O, (1 << k) - (1 << (k - 3)))
    K.release_domain()
    c = K.CacheManager()                                       # its own manager: no size recorded yet
    e = _Key(K, O, c, "first", k, zkey, wtns)                  # loads and proves once under N = 2n
    e.check_oracle()
    model = e0.model(G) if G > 1 else None
    shards = _load_shards(c, e, G) if G > 1 else []
    if G > 1:
        assert e.assemble(_dist_round(K, c, e, shards, wtns, model, " N=2n"), G) == e.want
    K.release_domain()
    K.initialize_domain(K.get_root_of_unity(1 << (k + 4)))

    def large_domain_is_resident():
        # a transform of all 2^(k+4) points is refused by any smaller domain
        x = O.ints_to_arr([(i * i + 7) % O.R_MOD for i in range(1 << (k + 4))])
        assert K.ntt(x, False).tobytes() == O.fr_ntt(x, False).tobytes()

    large_domain_is_resident()
    assert c.prove_mem("first", wtns, *RS)[:2] == (e.want, e.public)
    c.load("second", zkey)                                     # d_skeys of this entry: built from the larger table
    assert c.prove_mem("second", wtns, *RS)[:2] == (e.want, e.public)
    if G > 1:
        fresh = _load_shards(c, e, G, tag="+")                 # d_tw1 of these: built from the larger table
        for names, note in ((shards, " N=16n"), (fresh, " N=16n, loaded under it")):
            assert e.assemble(_dist_round(K, c, e, names, wtns, model, note), G) == e.want, note
            assert e.assemble(_replicated(c, names, wtns), G) == e.want, note
    large_domain_is_resident()                                 # still: no path has rebuilt the domain for 2n
    c.close()
    K.release_domain()


# ---- 6: stale state between witnesses -----------------------------------------------------------------------------------------------
def test_stale_state_between_witnesses(gpu, cm, keys, S):
    """(k, G) = (13, 2): Z rows of one witness in d_fold must never finish another witness's proof"""
    K = gpu
    e = keys.get("chain", 13)
    N = (1 << 13) - (1 << 10)
    w1, w2 = e.wtns, S.write_wtns(S.squaring_chain_witness(N, 5))
    assert w1 == S.write_wtns(S.squaring_chain_witness(N, 3)) and w2 != w1
    want2 = cm.prove_mem(e.name, w2, *RS)[0]
    assert want2 != e.want
    names = _load_shards(cm, e, 2)
    assert e.assemble(_dist_round(K, cm, e, names, w1), 2) == e.want                  # 1: a complete round with W1
    for nm in names:                                                                  # 2: stage 1 alone with W2
        cm.dist_stage1(nm, w2)
    blocks = b"".join(cm.commitments(nm, None)[0] for nm in names)                    # 3: must not finish from W1's Z rows
    assert e.assemble(blocks, 2, w2) == want2
    assert e.assemble(_dist_round(K, cm, e, names, w2), 2, w2) == want2               # 4: a complete round with W2
    assert e.assemble(_replicated(cm, names, w1), 2) == e.want                        # 5: W1 again, replicated
    for nm in names:                                                                  # 6: no stage 2 since the fresh stage 1
        cm.dist_stage1(nm, w2)
        with pytest.raises(K.ProverError, match="groth16_dist_stage2 has not run for the resident witness"):
            cm.dist_exchange_done(nm)
    blocks = b"".join(cm.commitments(nm, None)[0] for nm in names)
    assert e.assemble(blocks, 2, w2) == want2
    _evict(cm, names)
