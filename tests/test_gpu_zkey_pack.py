"""The device half of the packed proving key (needs an MI355X): the coefficient kernels of groth16_zkey_coefs_pack / _unpack against
tests/zkey_pack_model.py's Python integers at the smallest shapes where they can go wrong, groth16_zkey_pack / _unpack on whole keys
byte for byte, groth16_cache_load_packed against groth16_cache_load proof for proof, and the three REPL commands.  Every expected
byte is the model's (points: tests/point_pack_model.py) or the input's own; every case is CONSTRUCTED."""
import ctypes as C
import json
import os
import random
import struct
import subprocess

import pytest

import point_pack_model as PK
import test_gpu_ptau_pack as TP                                              # faulty points and words of every kind
import zkey_corpus as ZC
import zkey_pack_model as ZM
from conftest import ROOT

pytestmark = pytest.mark.gpu

R = ZM.R_MOD
FULL = R // 3                                                                # 32 significant bytes, its negation too
NONCANONICAL, OFF_CURVE, OFF_SUBGROUP = 1, 2, 3
# every rule and the lengths at which a path changes: zero, one, negated (1, 2 and 31 bytes), positive (1, 2, 31 and 32 bytes)
POOL = [0, 1, R - 1, R - 5, R - 256, R - (1 << 248) + 1, 2, 255, 256, 0xffff, (1 << 248) - 1, 1 << 248, FULL, R - FULL, (1 << 64) + 3]


def _same(got, want):
    first = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    assert len(got) == len(want) and got == want, "first difference at byte %d of %d" % (first, len(want))


def mixed(n, seed=1):
    rng = random.Random(seed)
    return [POOL[i % len(POOL)] if i < len(POOL) else rng.choice((1, R - 1)) if rng.random() < 0.75 else rng.choice(POOL + [rng.randrange(R)]) for i in range(n)]


def _codec_equals_model(K, values):
    records = ZM.records_of(values, triples=[(k & 1, (k * 7919) & 0xffffffff, 0xffffffff - k) for k in range(len(values))])
    want = ZM.coefs_body(records)
    assert ZM.unpack_body(want) == (records, [])
    got, rep = K.coefs_pack(records)
    _same(got, want)
    assert (rep.n, rep.in_bytes, rep.out_bytes, rep.fault_kind) == (len(values), len(records), len(want), 0)
    back, rep = K.coefs_unpack(want)
    _same(back, records)
    assert (rep.n, rep.in_bytes, rep.out_bytes, rep.fault_kind) == (len(values), len(want), len(records), 0)
    return want


# ---- the raw coefficient codec
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_codec_at_every_size(gpu, n):
    values = mixed(n, seed=n)
    body = _codec_equals_model(gpu, values)
    if n >= 63:
        codes = set(ZM.body_parts(body)[4])
        assert {0x00, 0x40} <= codes and {0x81, 0x82, 0x9f} <= codes and {0x01, 0x02, 0x1f, 0x20} <= codes   # every rule; lengths 1, 2, 31, 32
    _codec_equals_model(gpu, [1, R - 1] * (n // 2))                          # what a real key holds


@pytest.mark.parametrize("name,values", [
    ("all zero: an empty payload", [0] * 600),
    ("all full-width: 8192-byte blocks, the LDS maximum", [FULL + k for k in range(513)]),
    ("every length, positive and negated", [v for k in range(1, 32) for v in ((1 << (8 * k)) - 1, R - (1 << (8 * k)) + 1)] * 5),
])
def test_value_mixes(gpu, name, values):
    body = _codec_equals_model(gpu, values)
    if values[0] == FULL:
        assert ZM.body_parts(body)[5][:3] == [0, 8192, 16384]


def test_block_payloads_start_at_every_offset_mod_16(gpu):
    """block b's payload begins at the sum of the blocks before it: the starts run through every residue, once with one-byte values
    at the boundary and once with 31-byte values straddling it — the pack kernel's single bytes and whole vectors, the unpack
    kernel's aligned loads"""
    values = []
    for b in range(34):
        values += [2 + b] * (b % 16 + 1) + [FULL] * (b % 3) + [0] * (256 - (b % 16 + 1) - b % 3)
    assert {s % 16 for s in ZM.coefs_parts(ZM.records_of(values))[2][:-1]} == set(range(16))
    _codec_equals_model(gpu, values)
    values = []
    for b in range(34):
        values += [0] * 200 + [(1 << 248) - 1 - b] * (b % 5 + 1) + [7] * (b % 16) + [1] * (56 - (b % 5 + 1) - b % 16)
    assert {s % 16 for s in ZM.coefs_parts(ZM.records_of(values))[2][:-1]} == set(range(16))
    _codec_equals_model(gpu, values)
    # blocks shorter than one vector, so that several share it: no store may cover a neighbour's byte
    values = []
    for b in range(40):
        values += [3 + b] * (b % 7) + [1] * (256 - b % 7)
    _codec_equals_model(gpu, values)


# ---- faults
FAULTS = {
    "CODE": [(0x21, b""), (0xa0, b"")],
    "NONCANONICAL-top-byte": [(0x02, b"\x05\x00"), (0x83, b"\x01\x02\x00")],
    "NONCANONICAL-one": [(0x01, b"\x01"), (0x01, b"\x01")],
    "NONCANONICAL-negation-shorter": [(0x20, (R - 1).to_bytes(32, "little")), (0x20, (R - (1 << 248) + 1).to_bytes(32, "little"))],
    "RANGE": [(0x20, R.to_bytes(32, "little")), (0x20, b"\xff" * 32)],
}


def _body_refused(K, body, element, kind, count):
    records, faults = ZM.unpack_body(body)
    assert faults[0] == (element, kind) and len(faults) == count
    with pytest.raises(K.KeyFault, match=r"\(-2\): zkez: coefficient %d: %s" % (element, ZM.KIND_TEXT[kind])) as e:
        K.coefs_unpack(body)
    rep = e.value.report
    assert (rep.fault_kind, rep.fault_index, rep.fault_count) == (kind, element, count)
    # a filled buffer is as it was
    room = len(records)
    rep, buf = K.ZkeyCoefsReport(), C.create_string_buffer(b"\xaa" * room, room)
    assert K.lib().groth16_zkey_coefs_unpack(body, C.c_size_t(len(body)), buf, C.c_size_t(room), b"HIP", C.byref(rep)) == -2
    assert buf.raw == b"\xaa" * room and rep.fault_index == element


@pytest.mark.parametrize("name", sorted(FAULTS))
def test_each_fault_kind_twice_names_the_lower_and_counts_both(gpu, name):
    kind = getattr(ZM, name.split("-")[0])
    records = ZM.records_of(mixed(600, seed=7))
    _body_refused(gpu, ZM.coefs_body(records, replace={259: FAULTS[name][0], 517: FAULTS[name][1]}), 259, kind, 2)
    _body_refused(gpu, ZM.coefs_body(records, replace={0: FAULTS[name][0], 599: FAULTS[name][1]}), 0, kind, 2)   # the first and the last


def test_directory_faults(gpu):
    K = gpu
    records = ZM.records_of(mixed(800, seed=8))
    triples, codes, directory, payload = ZM.coefs_parts(records)
    moved = list(directory)
    moved[2] -= 1                                                            # one block boundary, one byte: host-valid
    _body_refused(K, ZM.body(800, triples, codes, moved, payload), 256, ZM.DIRECTORY, 2)
    # a CODE fault below it is the one named; the directory faults are counted
    e = next(i for i in range(256) if codes[i] in (0x00, 0x40))              # (a code without payload: block 0's sum stays what it was)
    _body_refused(K, ZM.body(800, triples, codes[:e] + b"\x60" + codes[e + 1:], moved, payload), e, ZM.CODE, 3)
    # the first and the last block
    moved = list(directory)
    moved[1] += 1
    moved[3] += 1
    _body_refused(K, ZM.body(800, triples, codes, moved, payload), 0, ZM.DIRECTORY, 4)


def test_a_value_not_below_r_is_refused_when_packing(gpu):
    K = gpu
    records = bytearray(ZM.records_of(mixed(700, seed=9)))
    records[300 * 44 + 12:300 * 44 + 44] = R.to_bytes(32, "little")
    records[600 * 44 + 12:600 * 44 + 44] = b"\xff" * 32
    with pytest.raises(K.KeyFault, match=r"\(-2\): zkey: coefficient 300: not below r") as e:
        K.coefs_pack(bytes(records))
    rep = e.value.report
    assert (rep.fault_kind, rep.fault_index, rep.fault_count) == (ZM.RANGE, 300, 2)
    room = 24 + 45 * 700 + 8 * 3
    rep, buf = K.ZkeyCoefsReport(), C.create_string_buffer(b"\xaa" * room, room)
    assert K.lib().groth16_zkey_coefs_pack(bytes(records), C.c_uint64(700), buf, C.c_size_t(room), b"HIP", C.byref(rep)) == -2 and buf.raw == b"\xaa" * room
    # cap one byte short: −3, the report says what is needed, nothing is written
    good = ZM.records_of(mixed(700, seed=9))
    need = len(ZM.coefs_body(good))
    rep, buf = K.ZkeyCoefsReport(), C.create_string_buffer(need)
    assert K.lib().groth16_zkey_coefs_pack(good, C.c_uint64(700), buf, C.c_size_t(need - 1), b"HIP", C.byref(rep)) == -3
    assert rep.out_bytes == need and buf.raw == bytes(need)


# ---- files
class Key:
    """S.random_circuit(500, 3, 16): 520 wires — two G1 workgroups and eight G2 workgroups plus 8 lanes — and several partial
    coefficient blocks, with extra A and B terms of coefficients r − 1, r − 5 and a full-width value on a wire whose witness value is
    0: the circuit stays satisfied"""

    def __init__(self, K, O, S):
        self.r1, self.w = S.random_circuit(500, 3, 16, bit_fraction=0.7, seed=21)
        x = next(i for i in range(20, len(self.w)) if self.w[i] == 0)
        self.r1.A += [(7, x, R - 1), (300, x, R - 5)]
        self.r1.B += [(450, x, FULL)]
        self.zkey, self.vk = S.setup(self.r1, lambda g, sc: K.generator_mul(g, sc), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
        self.wtns = S.write_wtns(self.w)
        self.zkez = ZM.pack_file(self.zkey)
        self.vk_json = S.vk_to_json(dict(self.vk, n_public=len(self.vk["IC"]) - 1))


@pytest.fixture(scope="module")
def key(gpu, O, S):
    return Key(gpu, O, S)


def _round_trip(K, zkey, zkez):
    packed, rep = K.zkey_pack(zkey)
    _same(packed, zkez)
    secs = dict(ZM.sections(zkey))
    n_coef = (len(secs[4]) - 4) // 44
    g1, g2 = sum(len(secs[s]) for s in (3, 5, 6, 8, 9)) // 64, len(secs[7]) // 128
    assert (rep.n_coef, list(rep.points), rep.in_bytes, rep.out_bytes) == (n_coef, [g1, g2], len(zkey), len(zkez))
    assert (rep.point_bytes, rep.coef_bytes) == (32 * g1 + 64 * g2, len(ZM.payload(zkez, 4))) and (rep.fault_section, rep.fault_kind, rep.fault_count) == (0, 0, 0)
    assert rep.upload_ms > 0 and rep.device_ms > 0 and rep.download_ms > 0
    assert len(zkez) <= K.zkey_packed_bound(zkey) and K.zkey_unpacked_size(zkez) == len(zkey)
    back, rep = K.zkey_unpack(zkez)
    _same(back, zkey)
    assert (rep.n_coef, list(rep.points), rep.in_bytes, rep.out_bytes, rep.coef_bytes) == (n_coef, [g1, g2], len(zkez), len(zkey), len(ZM.payload(zkez, 4)))


def test_the_golden_key_round_trips_in_every_byte(gpu):
    zkey = ZC.golden_zkey()
    _round_trip(gpu, zkey, ZM.pack_file(zkey))


def test_a_key_of_several_workgroups_round_trips_in_every_byte(gpu, key, tmp_path):
    K = gpu
    words = {sid: ZM.payload(key.zkez, sid) for sid in ZM.POINT_BYTES}
    g1 = [words[s][i:i + 32] for s in (3, 5, 6, 8, 9) for i in range(0, len(words[s]), 32)]
    g2 = [words[7][i:i + 64] for i in range(0, len(words[7]), 64)]
    assert len(g2) == 520 and len(words[9]) // 32 == 512
    # identities and both signs, in G1 and in G2
    assert bytes(31) + b"\x40" in g1 and {w[31] >> 7 for w in g1 if w[31] != 0x40} == {0, 1}
    assert bytes(63) + b"\x40" in g2 and {w[63] >> 7 for w in g2 if w[63] != 0x40} == {0, 1}
    # the coefficients: ±1 for the most part, the appended terms, several partial blocks' worth
    _, n, _, _, codes, directory, _ = ZM.body_parts(ZM.payload(key.zkez, 4))
    values = ZM.record_values(ZM.payload(key.zkey, 4)[4:])
    assert n > 4 * 256 and n % 256 and {R - 1, R - 5, FULL} <= set(values) and {0x40, 0x81, 0x20, 0x02} <= set(codes)
    _round_trip(K, key.zkey, key.zkez)
    # the file entries write the same bytes and leave nothing else
    (tmp_path / "k.zkey").write_bytes(key.zkey)
    none, rep = K.zkey_pack(tmp_path / "k.zkey", out=tmp_path / "k.zkez")
    assert none is None and rep.write_ms > 0 and rep.out_bytes == len(key.zkez)
    _same((tmp_path / "k.zkez").read_bytes(), key.zkez)
    none, rep = K.zkey_unpack(tmp_path / "k.zkez", out=tmp_path / "back.zkey")
    assert none is None and rep.write_ms > 0
    _same((tmp_path / "back.zkey").read_bytes(), key.zkey)
    assert sorted(os.listdir(tmp_path)) == ["back.zkey", "k.zkey", "k.zkez"]
    for f in (K.zkey_pack, K.zkey_unpack):
        with pytest.raises(K.ProverError, match=r"\(-3\).*the output path is the input's"):
            f(tmp_path / "k.zkez", out=tmp_path / "k.zkez")
    # cap one byte short: −3, the report says what is needed, nothing is written
    for entry, image, need in ((K.lib().groth16_zkey_pack, key.zkey, len(key.zkez)), (K.lib().groth16_zkey_unpack, key.zkez, len(key.zkey))):
        rep, buf = K.ZkeyPackReport(), C.create_string_buffer(need)
        assert entry(image, C.c_size_t(len(image)), buf, C.c_size_t(need - 1), b"HIP", C.byref(rep)) == -3
        assert rep.out_bytes == need and buf.raw == bytes(need)


def test_section_order_unknown_sections_and_section_10_survive(gpu):
    K = gpu
    secs = ZM.sections(ZC.golden_zkey())
    by = dict(secs)
    order = [1, 9, 2, 77, 7, 4, 10, 3, 8, 6, 5, 78]
    by.update({77: b"in the middle" * 5, 78: bytes(range(77)), 10: struct.pack("<I", 1) + bytes(range(200))})
    zkey = ZM.container([(s, by[s]) for s in order], magic=b"zkey")
    zkez = ZM.pack_file(zkey)
    assert [s for s, _ in ZM.sections(zkez)] == order
    _round_trip(K, zkey, zkez)
    packed = K.zkey_pack(zkey)[0]
    for sid in (1, 2, 10, 77, 78):
        assert ZM.payload(packed, sid) == by[sid]
    # the unpacked key is the key: the loader takes it
    cm = K.CacheManager()
    try:
        cm.load("permuted", K.zkey_unpack(packed)[0])
        assert cm.contains("permuted")
    finally:
        cm.close()
        K.release_domain()


def _put(image, sid, element, elem_bytes, new):
    p = bytearray(ZM.payload(image, sid))
    p[element * elem_bytes:element * elem_bytes + len(new)] = new
    return ZM.with_section(image, sid, bytes(p))


@pytest.mark.parametrize("sid", [5, 7], ids=["g1", "g2"])
def test_a_faulty_point_of_each_kind_is_named_and_nothing_is_written(gpu, key, sid):
    """at the last index and at a lower one in another workgroup; the lower one is named and both are counted"""
    K = gpu
    g2, last, low = sid == 7, 519, 70
    for form, image, elem, bad, wrapper, entry, room in (("zkez", key.zkez, 64 if g2 else 32, TP._bad_words(g2), K.zkey_unpack, K.lib().groth16_zkey_unpack, len(key.zkey)),
                                                         ("zkey", key.zkey, 128 if g2 else 64, TP._bad_points(g2), K.zkey_pack, K.lib().groth16_zkey_pack, len(key.zkey))):
        assert sorted(bad) == ([NONCANONICAL, OFF_CURVE, OFF_SUBGROUP] if g2 else [NONCANONICAL, OFF_CURVE])
        for kind, b in bad.items():
            e = _put(_put(image, sid, last, elem, b), sid, low, elem, b)
            with pytest.raises(K.KeyFault, match=r"\(-2\): %s: section %d, element %d: %s" % (form, sid, low, PK.KIND_TEXT[kind])) as err:
                wrapper(e)
            rep = err.value.report
            assert (rep.fault_section, rep.fault_index, rep.fault_kind, rep.fault_count) == (sid, low, kind, 2), (form, kind)
        rep, buf = K.ZkeyPackReport(), C.create_string_buffer(b"\x5a" * room, room)
        assert entry(e, C.c_size_t(len(e)), buf, C.c_size_t(room), b"HIP", C.byref(rep)) == -2 and buf.raw == b"\x5a" * room
    # the lowest faulty SECTION is named: a coefficient (section 4) before section 5, section 3 before both
    two = _put(key.zkez, sid, low, 64 if g2 else 32, TP._bad_words(g2)[OFF_CURVE])
    two = ZM.with_section(two, 4, ZM.coefs_body(ZM.payload(key.zkey, 4)[4:], declared=struct.unpack_from("<I", ZM.payload(key.zkey, 4), 0)[0], replace={300: (0x21, b"")}))
    with pytest.raises(K.KeyFault, match=r"\(-2\): zkez: coefficient 300: an undefined code byte") as err:
        K.zkey_unpack(two)
    assert (err.value.report.fault_section, err.value.report.fault_kind, err.value.report.fault_count) == (4, ZM.CODE, 1)
    with pytest.raises(K.KeyFault, match=r"\(-2\): zkez: section 3, element 1: the point is not on the curve"):
        K.zkey_unpack(_put(two, 3, 1, 32, TP._bad_words(False)[OFF_CURVE]))


def test_a_faulty_packed_file_leaves_nothing_behind(gpu, key, tmp_path):
    K = gpu
    (tmp_path / "bad.zkez").write_bytes(_put(key.zkez, 9, 511, 32, TP._bad_words(False)[OFF_CURVE]))
    with pytest.raises(K.KeyFault, match=r"\(-2\): zkez: section 9, element 511"):
        K.zkey_unpack(tmp_path / "bad.zkez", out=tmp_path / "never.zkey")
    assert os.listdir(tmp_path) == ["bad.zkez"]
    records = bytearray(ZM.payload(key.zkey, 4))
    records[4 + 44 * 1000 + 12:4 + 44 * 1000 + 44] = R.to_bytes(32, "little")
    with pytest.raises(K.KeyFault, match=r"\(-2\): zkey: coefficient 1000: not below r") as err:
        K.zkey_pack(ZM.with_section(key.zkey, 4, bytes(records)))
    assert (err.value.report.fault_section, err.value.report.fault_kind) == (4, ZM.RANGE)


# ---- the packed load
@pytest.fixture(scope="module")
def cm(gpu):
    c = gpu.CacheManager()
    yield c
    c.close()
    gpu.release_domain()


def _info(cm, name):
    i = cm.info(name)
    return (i.n_vars, i.n_public, i.domain_size, i.n_coef, i.device_bytes, i.b_bases)


def test_the_packed_load_proves_what_the_load_proves(gpu, cm, O, key):
    r, s = 0x1234567890ABCDEF << 100, 987654321
    cm.load("a", key.zkey, wait_tables=False)
    cm.load_packed("b", key.zkez, wait_tables=False)
    proof, public = O.groth16_prove(key.zkey, key.wtns, r, s)
    for again in (False, True):
        if again:
            assert cm.tables_ready("a", wait=True) and cm.tables_ready("b", wait=True)
        pa, qa, _ = cm.prove_mem("a", key.wtns, r, s)
        pb, qb, _ = cm.prove_mem("b", key.wtns, r, s)
        assert (pa, qa) == (pb, qb) and json.loads(pb) == proof and json.loads(qb) == public
        assert _info(cm, "a") == _info(cm, "b")
    assert gpu.groth16_verify_json(pb, qb, key.vk_json)
    # a key the manager holds is not loaded again; a path loads like an image
    cm.load_packed("b", b"not looked at")
    cm.evict("a")
    cm.evict("b")


def test_the_packed_load_from_a_file_and_on_the_golden_key(gpu, cm, O, key, tmp_path):
    (tmp_path / "k.zkez").write_bytes(key.zkez)
    cm.load_packed("f", str(tmp_path / "k.zkez"))
    proof, public = O.groth16_prove(key.zkey, key.wtns, 3, 5)
    pj, qj, _ = cm.prove_mem("f", key.wtns, 3, 5)
    assert json.loads(pj) == proof and json.loads(qj) == public
    cm.evict("f")
    import base64
    from conftest import load_golden, unhex_int
    g = load_golden("groth16.json")
    cm.load_packed("golden", ZM.pack_file(base64.b64decode(g["zkey"])))
    for c in g["cases"]:
        pj, qj, _ = cm.prove_mem("golden", base64.b64decode(g["wtns"]), unhex_int(c["r"]), unhex_int(c["s"]))
        assert pj == json.dumps(c["proof"], indent=2, sort_keys=True) and qj == json.dumps(c["public"], indent=2)
    cm.evict("golden")


def test_a_faulty_packed_key_is_not_cached_and_a_sound_one_still_loads(gpu, cm, O, key):
    for sid, elem, word, text in ((5, 32, TP._bad_words(False)[OFF_CURVE], "zkez: section 5, element 519: the point is not on the curve"),
                                  (7, 64, TP.TWIST_OUTSIDE_WORD, "zkez: section 7, element 519: the point is outside the subgroup"),
                                  (9, 32, TP._bad_words(False)[NONCANONICAL], "zkez: section 9, element 511: a coordinate is not below q")):
        with pytest.raises(gpu.ProverError, match=r"\(-2\): " + text):
            cm.load_packed("k", _put(key.zkez, sid, 511 if sid == 9 else 519, elem, word))
        assert not cm.contains("k")
    body = ZM.coefs_body(ZM.payload(key.zkey, 4)[4:], replace={700: (0x20, R.to_bytes(32, "little"))})
    with pytest.raises(gpu.ProverError, match=r"\(-2\): zkez: coefficient 700: 32 bytes that are not below r"):
        cm.load_packed("k", ZM.with_section(key.zkez, 4, body))
    assert not cm.contains("k")
    cm.load_packed("k", key.zkez)
    pj, qj, _ = cm.prove_mem("k", key.wtns, 3, 5)
    proof, public = O.groth16_prove(key.zkey, key.wtns, 3, 5)
    assert json.loads(pj) == proof and json.loads(qj) == public
    cm.evict("k")
    # one device only
    with pytest.raises(gpu.ProverError, match=r"\(-3\): shard 0 of 2: groth16_cache_load_packed takes single-device keys"):
        cm.load_packed("shard0", key.zkez, shard_rank=0, shard_count=2)
    assert not cm.contains("shard0")


# ---- the REPL
def test_repl(gpu, key, tmp_path):
    t = tmp_path
    (t / "w.wtns").write_bytes(key.wtns)
    (t / "k.zkey").write_bytes(key.zkey)
    (t / "bad.zkez").write_bytes(_put(key.zkez, 7, 6, 64, TP.TWIST_OUTSIDE_WORD))
    cmds = (f"zkey-pack --zkey {t}/k.zkey --out {t}/k.zkez --device HIP\n"
            f"zkey-unpack --packed {t}/k.zkez --out {t}/back.zkey\n"
            f"zkey-unpack --packed {t}/bad.zkez --out {t}/never.zkey\n"
            f"prove --witness {t}/w.wtns --zkey {t}/k.zkez --proof {t}/never.json --public {t}/never_public.json --device HIP\n"
            f"prove-zkez --witness {t}/w.wtns --zkez {t}/k.zkez --proof {t}/proof_z.json --public {t}/public_z.json --device HIP\n"
            f"prove --witness {t}/w.wtns --zkey {t}/k.zkey --proof {t}/proof.json --public {t}/public.json --device HIP\nexit\n")
    run = subprocess.run([os.path.join(ROOT, "icicle-snark_amd", "lib", "prove")], input=cmds, capture_output=True, text=True, timeout=300, env=dict(os.environ, ICICLE_SNARK_QUIET="1"))
    assert run.returncode == 0, run.stderr
    lines = [ln.replace("> ", "") for ln in run.stdout.splitlines()]
    n_coef = (len(ZM.payload(key.zkey, 4)) - 4) // 44
    head = "wires 520 domain 512 coefficients %d points %d 520 bytes " % (n_coef, 4 + 520 + 520 + 516 + 512)
    assert lines[0].startswith(head + "%d to %d (packed points " % (len(key.zkey), len(key.zkez))) and lines[1:3] == ["ZKEY_WRITTEN", "COMMAND_COMPLETED"]
    assert lines[3].startswith(head + "%d to %d (packed points " % (len(key.zkez), len(key.zkey))) and lines[4:6] == ["ZKEY_WRITTEN", "COMMAND_COMPLETED"]
    assert lines[6:8] == ["ZKEY_BAD POINT 7 6 1", "COMMAND_COMPLETED"] and "zkey-unpack failed (-2): zkez: section 7, element 6: the point is outside the subgroup" in run.stderr
    assert lines[8:11] == ["COMMAND_COMPLETED"] * 3 and "prove failed (-2): Invalid File format (expected 'zkey')" in run.stderr
    _same((t / "k.zkez").read_bytes(), key.zkez)
    _same((t / "back.zkey").read_bytes(), key.zkey)
    # the blinding is random: both proofs verify, over the same public signals
    public = (t / "public.json").read_text()
    assert (t / "public_z.json").read_text() == public and json.loads(public) == [str(v) for v in key.w[1:1 + key.r1.n_public]]
    for name in ("proof.json", "proof_z.json"):
        assert gpu.groth16_verify_json((t / name).read_text(), public, key.vk_json)
    assert sorted(os.listdir(t)) == ["back.zkey", "bad.zkez", "k.zkey", "k.zkez", "proof.json", "proof_z.json", "public.json", "public_z.json", "w.wtns"]
