"""The device half of the packed witness (needs an MI355X): groth16_wtns_unpack's kernel against tests/wtns_pack_model.py's Python
integers at the smallest shapes where it can go wrong, groth16_prove_packed against groth16_prove_mem byte for byte, the witness
check from a packed witness, and the four REPL commands.  Every expected byte is the model's; every case is CONSTRUCTED."""
import base64
import json
import os
import random
import subprocess

import pytest

import wtns_pack_model as M
from conftest import ROOT, load_golden, unhex_int

pytestmark = pytest.mark.gpu

R = M.R_MOD
EDGES = M.edge_values()
FULL = R // 3                                                                # 32 significant bytes, its negation too


def mixed(n, seed=1):
    rng = random.Random(seed)
    pool = EDGES + [rng.randrange(R) for _ in range(8)] + [rng.randrange(1 << 64) for _ in range(4)] + [R - rng.randrange(1, 1 << 40) for _ in range(4)]
    return [rng.randrange(2) if rng.random() < 0.75 else rng.choice(pool) for _ in range(n)]


def _device_equals_model(K, values, image=None):
    image = M.pack(values) if image is None else image
    out, rep = K.wtns_unpack(image, device="HIP")
    assert out == M.write_wtns(values)
    assert (rep.n_witness, rep.in_bytes, rep.out_bytes, rep.fault_kind) == (len(values), len(image), 76 + 32 * len(values), 0)
    return rep


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_device_unpack_at_every_size(gpu, n):
    _device_equals_model(gpu, mixed(n, seed=n))
    _device_equals_model(gpu, (EDGES * (n // len(EDGES) + 1))[:n])


@pytest.mark.parametrize("name,values", [
    ("all zero: an empty payload", [0] * 600),
    ("all one", [1] * 600),
    ("all full-width: 8192-byte blocks, the LDS maximum", [FULL + k for k in range(513)]),
    ("all negated", [R - 1 - k * 251 for k in range(700)]),
    ("every length, positive and negated", [v for k in range(1, 32) for v in ((1 << (8 * k)) - 1, R - (1 << (8 * k)) + 1)] * 5),
])
def test_value_mixes(gpu, name, values):
    rep = _device_equals_model(gpu, values)
    if values[0] == FULL:
        assert M.pack_parts(values)[1][:3] == [0, 8192, 16384]
    assert rep.kernel_ms > 0 and rep.upload_ms > 0


def test_block_payloads_start_at_every_offset_mod_16(gpu):
    """block b's payload begins at the sum of the blocks before it: block b carries b + 1 one-byte values and full-width values
    otherwise 0, so the starts run through every residue; a second witness does the same with 31-byte values straddling the start"""
    values = []
    for b in range(34):
        values += [2 + b] * (b % 16 + 1) + [FULL] * (b % 3) + [0] * (256 - (b % 16 + 1) - b % 3)
    starts = M.pack_parts(values)[1]
    assert {s % 16 for s in starts[:-1]} == set(range(16))
    _device_equals_model(gpu, values)
    values = []
    for b in range(34):
        values += [0] * 200 + [(1 << 248) - 1 - b] * (b % 5 + 1) + [7] * (b % 16) + [1] * (56 - (b % 5 + 1) - b % 16)
    assert {s % 16 for s in M.pack_parts(values)[1][:-1]} == set(range(16))
    _device_equals_model(gpu, values)


def with_faults(values, faults):
    codes, payload, directory = bytearray(), bytearray(), []
    for i, v in enumerate(values):
        if i % M.BLOCK == 0:
            directory.append(len(payload))
        c, p = faults.get(i, None) or M.encode(v)
        codes.append(c)
        payload += p
    directory.append(len(payload))
    return M.container(len(values), bytes(codes), directory, bytes(payload))


FAULTS = {
    "CODE": [(0x21, b""), (0xa0, b"")],
    "NONCANONICAL-top-byte": [(0x02, b"\x05\x00"), (0x83, b"\x01\x02\x00")],
    "NONCANONICAL-one": [(0x01, b"\x01"), (0x01, b"\x01")],
    "NONCANONICAL-negation-shorter": [(0x20, (R - 1).to_bytes(32, "little")), (0x20, (R - (1 << 248) + 1).to_bytes(32, "little"))],
    "RANGE": [(0x20, R.to_bytes(32, "little")), (0x20, b"\xff" * 32)],
}


def _refused(K, image, element, kind, count):
    assert M.unpack(image)[1][0] == (element, kind) and len(M.unpack(image)[1]) == count
    with pytest.raises(K.WitnessFault, match=f"wtnz: element {element}: {M.KIND_TEXT[kind]}") as e:
        K.wtns_unpack(image, device="HIP")
    rep = e.value.report
    assert (rep.fault_kind, rep.fault_index, rep.fault_count) == (kind, element, count)


@pytest.mark.parametrize("name", sorted(FAULTS))
def test_each_fault_kind_twice_names_the_lower_and_counts_both(gpu, name):
    kind = getattr(M, name.split("-")[0])
    values = mixed(600, seed=7)
    _refused(gpu, with_faults(values, {259: FAULTS[name][0], 517: FAULTS[name][1]}), 259, kind, 2)
    # the first and the last element of the witness
    _refused(gpu, with_faults(values, {0: FAULTS[name][0], 599: FAULTS[name][1]}), 0, kind, 2)


def test_directory_fault_and_nothing_written(gpu, tmp_path):
    K = gpu
    values = mixed(800, seed=8)
    codes, directory, payload = M.pack_parts(values)
    moved = list(directory)
    moved[2] -= 1                                                            # one block boundary, one byte: host-valid
    image = M.container(800, codes, moved, payload)
    _refused(K, image, 256, M.DIRECTORY, 2)
    # a CODE fault below it is the one named; the directory faults are counted
    e = next(i for i in range(256) if codes[i] in (0x00, 0x40))              # (a code without payload: block 0's sum stays what it was)
    _refused(K, M.container(800, codes[:e] + b"\x60" + codes[e + 1:], moved, payload), e, M.CODE, 3)
    # the buffer entry: nothing written; the file entry: nothing left
    import ctypes as C
    rep, buf = K.WtnsPackReport(), C.create_string_buffer(b"\xaa" * (76 + 32 * 800), 76 + 32 * 800)
    assert K.lib().groth16_wtns_unpack(image, C.c_size_t(len(image)), buf, C.c_size_t(len(buf)), b"HIP", C.byref(rep)) == -2
    assert buf.raw == b"\xaa" * len(buf) and rep.fault_index == 256
    (tmp_path / "bad.wtnz").write_bytes(image)
    with pytest.raises(K.WitnessFault):
        K.wtns_unpack(str(tmp_path / "bad.wtnz"), out=str(tmp_path / "never.wtns"), device="HIP")
    assert os.listdir(tmp_path) == ["bad.wtnz"]
    # and the file entry of a sound witness
    (tmp_path / "ok.wtnz").write_bytes(M.pack(values))
    assert K.wtns_unpack(str(tmp_path / "ok.wtnz"), out=str(tmp_path / "ok.wtns"), device="HIP")[0] is None
    assert (tmp_path / "ok.wtns").read_bytes() == M.write_wtns(values)
    with pytest.raises(K.ProverError, match="does not name one HIP device"):
        K.wtns_unpack(M.pack(values), device="HIP:0-1")


# ---- prove_packed
@pytest.fixture(scope="module")
def cm(gpu):
    c = gpu.CacheManager()
    yield c
    c.close()
    gpu.release_domain()


class Key:
    """a circuit of several blocks: 520 wires, a bit-heavy witness, its key and its oracle proof"""

    def __init__(self, K, O, S):
        self.r1, self.w = S.random_circuit(500, 3, 16, bit_fraction=0.7, seed=21)
        self.zkey, self.vk = S.setup(self.r1, lambda g, sc: K.generator_mul(g, sc), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
        self.wtns = M.write_wtns(self.w)
        self.wtnz = M.pack(self.w)


@pytest.fixture(scope="module")
def key(gpu, O, S):
    return Key(gpu, O, S)


def test_prove_packed_on_the_golden_key(gpu, cm):
    g = load_golden("groth16.json")
    zkey, wtns = base64.b64decode(g["zkey"]), base64.b64decode(g["wtns"])
    values = M.wtns_values(wtns)
    assert M.write_wtns(values) == wtns
    cm.load("golden", zkey)
    for c in g["cases"]:
        pj, qj, _ = cm.prove_packed("golden", M.pack(values), unhex_int(c["r"]), unhex_int(c["s"]))
        assert pj == json.dumps(c["proof"], indent=2, sort_keys=True) and qj == json.dumps(c["public"], indent=2)
    cm.evict("golden")


def test_prove_packed_equals_prove_mem_byte_for_byte(gpu, cm, O, key):
    K = gpu
    assert len(key.w) > 2 * M.BLOCK and sum(1 for v in key.w if v < 2) > len(key.w) // 2
    cm.load("k", key.zkey)
    r, s = 0x1234567890ABCDEF << 100, 987654321
    want_p, want_q, _ = cm.prove_mem("k", key.wtns, r, s)
    # another witness in between, so that nothing of the first one is left on the device
    other = list(key.w)
    other[len(other) // 2] = (other[len(other) // 2] + 1) % R
    assert cm.prove_mem("k", M.write_wtns(other), r, s)[0] != want_p
    pj, qj, tm = cm.prove_packed("k", key.wtnz, r, s)
    assert (pj, qj) == (want_p, want_q) and tm.total_ms > 0
    # the witness is resident as after prove_mem
    assert cm.prove_mem("k", key.wtns, r, s, resident=True)[:2] == (want_p, want_q)
    # random blinding: valid proofs
    p1, q1, _ = cm.prove_packed("k", key.wtnz)
    assert p1 != want_p and q1 == want_q and K.groth16_verify_json(p1, q1, _vk(key))
    # an ordinary prove_mem afterwards still equals the oracle
    pj, qj, _ = cm.prove_mem("k", key.wtns, 3, 5)
    proof, public = O.groth16_prove(key.zkey, key.wtns, 3, 5)
    assert json.loads(pj) == proof and json.loads(qj) == public


def _vk(key):
    import importlib
    S = importlib.import_module("icicle-snark_amd.synth")
    return S.vk_to_json(dict(key.vk, n_public=len(key.vk["IC"]) - 1))


def test_a_faulty_packed_witness_proves_nothing_and_leaves_nothing_resident(gpu, cm, key):
    if not cm.contains("k"):
        cm.load("k", key.zkey)
    cm.prove_mem("k", key.wtns, 3, 5)                                       # a witness is resident
    bad = with_faults(key.w, {300: (0x20, R.to_bytes(32, "little"))})
    with pytest.raises(gpu.ProverError, match=r"\(-2\): wtnz: element 300: 32 bytes that are not below r"):
        cm.prove_packed("k", bad, 3, 5)
    with pytest.raises(gpu.ProverError, match="no witness given and none resident"):
        cm.prove_mem("k", key.wtns, 3, 5, resident=True)
    # the entries' own tests of a witness, with their messages; each reader refuses the other's magic
    with pytest.raises(gpu.ProverError, match="Invalid witness length. Circuit: %d, witness: %d" % (len(key.w), len(key.w) - 1)):
        cm.prove_packed("k", M.pack(key.w[:-1]), 3, 5)
    codes, directory, payload = M.pack_parts(key.w)
    with pytest.raises(gpu.ProverError, match="Curve of the witness does not match the curve of the proving key"):
        cm.prove_packed("k", M.container(len(key.w), codes, directory, payload, q=R + 2), 3, 5)
    with pytest.raises(gpu.ProverError, match=r"Invalid File format \(expected 'wtnz'\)"):
        cm.prove_packed("k", key.wtns, 3, 5)
    with pytest.raises(gpu.ProverError, match=r"Invalid File format \(expected 'wtns'\)"):
        cm.prove_mem("k", key.wtnz, 3, 5)
    assert cm.prove_packed("k", key.wtnz, 3, 5)[:2] == cm.prove_mem("k", key.wtns, 3, 5)[:2]


def test_a_shard_is_refused(gpu, cm, key):
    cm.load("shard0", key.zkey, shard_rank=0, shard_count=2)
    with pytest.raises(gpu.ProverError, match=r"\(-3\).*shard 0 of 2: groth16_prove_packed takes single-device keys"):
        cm.prove_packed("shard0", key.wtnz, 3, 5)
    cm.evict("shard0")
    with pytest.raises(gpu.ProverError, match=r"\(-4\)"):
        cm.prove_packed("absent", key.wtnz, 3, 5)


# ---- check_packed
def test_check_packed_gives_the_unpacked_verdict(gpu, S, key, tmp_path):
    K = gpu
    with K.R1cs(S.write_r1cs(key.r1)) as h:
        ok, rep = h.check(key.wtns)
        okz, repz = h.check_packed(key.wtnz)
        assert ok is True and okz is True and (repz.kind, repz.index, repz.noncanonical, repz.failed) == (rep.kind, rep.index, rep.noncanonical, rep.failed) == (0, 0, 0, 0)
        w = list(key.w)
        w[-1] = (w[-1] + 1) % R
        w[len(w) // 2] = (w[len(w) // 2] + 5) % R
        ok, rep = h.check(M.write_wtns(w))
        (tmp_path / "w.wtnz").write_bytes(M.pack(w))
        for okz, repz in (h.check_packed(M.pack(w)), h.check_packed(str(tmp_path / "w.wtnz"))):
            assert ok is False and okz is False and rep.failed > 0
            assert (repz.kind, repz.index, repz.noncanonical, repz.failed) == (rep.kind, rep.index, rep.noncanonical, rep.failed)
        w[0] = 2
        assert h.check_packed(M.pack(w))[1].kind == h.check(M.write_wtns(w))[1].kind != 0
        with pytest.raises(K.ProverError, match=r"\(-2\): wtnz: element 300: an undefined code byte"):
            h.check_packed(with_faults(key.w, {300: (0x41, b"")}))
        with pytest.raises(K.ProverError, match=r"\(-3\): the witness has %d values, the circuit %d wires" % (len(w) - 1, len(w))):
            h.check_packed(M.pack(w[:-1]))
        with pytest.raises(K.ProverError, match=r"Invalid File format \(expected 'wtnz'\)"):
            h.check_packed(key.wtns)
        with pytest.raises(K.ProverError, match=r"Invalid File format \(expected 'wtns'\)"):
            h.check(key.wtnz)
        assert h.check_packed(key.wtnz)[0] is True                          # the handle is as good as before


# ---- the REPL
def test_repl(gpu, O, S, key, tmp_path):
    t = tmp_path
    (t / "w.wtns").write_bytes(key.wtns)
    (t / "k.zkey").write_bytes(key.zkey)
    (t / "c.r1cs").write_bytes(S.write_r1cs(key.r1))
    (t / "bad.wtnz").write_bytes(with_faults(key.w, {300: (0x41, b""), 301: (0x41, b"")}))
    cmds = (f"wtns-pack --wtns {t}/w.wtns --out {t}/w.wtnz\n"
            f"wtns-unpack --packed {t}/w.wtnz --out {t}/host.wtns\n"
            f"wtns-unpack --packed {t}/w.wtnz --out {t}/dev.wtns --device HIP\n"
            f"wtns-unpack --packed {t}/bad.wtnz --out {t}/never.wtns --device HIP\n"
            f"prove-packed --witness {t}/w.wtnz --zkey {t}/k.zkey --proof {t}/proof.json --public {t}/public.json --device HIP\n"
            f"wtns-check --r1cs {t}/c.r1cs --wtnz {t}/w.wtnz\n"
            f"wtns-check --r1cs {t}/c.r1cs --wtnz {t}/bad.wtnz\nexit\n")
    run = subprocess.run([os.path.join(ROOT, "icicle-snark_amd", "lib", "prove")], input=cmds, capture_output=True, text=True, timeout=300, env=dict(os.environ, ICICLE_SNARK_QUIET="1"))
    assert run.returncode == 0, run.stderr
    lines = [ln.replace("> ", "") for ln in run.stdout.splitlines()]
    n, a, b = len(key.w), len(key.wtns), len(key.wtnz)
    assert lines[0].startswith(f"values {n} bytes {a} to {b} write ") and lines[1:3] == ["WTNS_WRITTEN", "COMMAND_COMPLETED"]
    assert lines[3].startswith(f"values {n} bytes {b} to {a} write ") and lines[4:6] == ["WTNS_WRITTEN", "COMMAND_COMPLETED"]
    assert lines[6].startswith(f"values {n} bytes {b} to {a}; upload ") and lines[7:9] == ["WTNS_WRITTEN", "COMMAND_COMPLETED"]
    assert lines[9:11] == ["WTNS_BAD VALUE 300 2", "COMMAND_COMPLETED"] and "wtns-unpack failed (-2): wtnz: element 300: an undefined code byte" in run.stderr
    assert lines[11] == "COMMAND_COMPLETED"
    assert lines[12:14] == ["satisfied", "COMMAND_COMPLETED"]
    assert lines[14] == "COMMAND_COMPLETED" and "wtns-check failed (-2): wtnz: element 300: an undefined code byte" in run.stderr
    assert (t / "w.wtnz").read_bytes() == key.wtnz and (t / "host.wtns").read_bytes() == key.wtns and (t / "dev.wtns").read_bytes() == key.wtns
    proof, public = json.loads((t / "proof.json").read_text()), (t / "public.json").read_text()
    assert json.loads(public) == [str(v) for v in key.w[1:1 + key.r1.n_public]]
    assert gpu.groth16_verify_json(json.dumps(proof), public, _vk(key))
    assert sorted(os.listdir(t)) == ["bad.wtnz", "c.r1cs", "dev.wtns", "host.wtns", "k.zkey", "proof.json", "public.json", "w.wtns", "w.wtnz"]
