"""groth16_zkey_check on the GPU (needs an MI355X): a sound key passes; every fault below is CONSTRUCTED — an edit of the zkey's
bytes at a chosen section and index — and must be reported with its exact kind, section, index and counts.  One key serves the
module: 163 wires on a 256-point domain, so sections 5 to 9 cross two wave boundaries and end mid-wave."""
import base64
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
import groth16_dlog_model as M

pytestmark = pytest.mark.gpu

Q = M.Q
U64_MAX = (1 << 64) - 1
NONCANONICAL, OFF_CURVE, OFF_SUBGROUP, IDENTITY, PAIR_MISMATCH, COEFFICIENT = range(1, 7)
SEED = hashlib.sha256(b"zkey-check").digest()
SEEDS = [hashlib.sha256(b"zkey-check %d" % k).digest() for k in range(8)]
HEADER_SLOTS = [(0, 64), (64, 64), (128, 128), (256, 128), (384, 64), (448, 128)]  # α₁ β₁ β₂ γ₂ δ₁ δ₂: offset behind byte 84, size
ELEM = {3: 64, 5: 64, 6: 64, 7: 128, 8: 64, 9: 64}


def _sections(z):
    """{id: (offset of the payload, length)} of a snarkjs binary container: the small section walker of this test"""
    n = struct.unpack_from("<I", z, 8)[0]
    pos, out = 12, {}
    for _ in range(n):
        sid, ln = struct.unpack_from("<IQ", z, pos)
        out[sid] = (pos + 12, ln)
        pos += 12 + ln
    return out


class Key:
    def __init__(self, K, O, S):
        r1, w = S.random_circuit(150, 2, 10, seed=11)
        self.zkey, self.vk = S.setup(r1, lambda g, sc: K.generator_mul(g, sc), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
        self.wtns = S.write_wtns(w)
        self.sec = _sections(self.zkey)
        self.n_vars, self.n_public, self.domain = struct.unpack_from("<III", self.zkey, self.sec[2][0] + 72)
        self.O = O

    def count(self, s):
        return self.sec[s][1] // ELEM[s]

    def where(self, s, i):
        if s == 2:
            off, size = HEADER_SLOTS[i]
            return self.sec[2][0] + 84 + off, size
        return self.sec[s][0] + i * ELEM[s], ELEM[s]

    def words(self, z, s, i):
        """the point's coordinates as the file holds them (Montgomery residues)"""
        off, size = self.where(s, i)
        return [int.from_bytes(z[off + 32 * k:off + 32 * k + 32], "little") for k in range(size // 32)]

    def put_words(self, z, s, i, words):
        off, size = self.where(s, i)
        assert len(words) == size // 32
        z[off:off + size] = b"".join(int(v).to_bytes(32, "little") for v in words)

    def point(self, z, s, i):
        """standard-form coordinates"""
        return self.O.arr_to_ints(self.O.fq_convert_montgomery(self.O.ints_to_arr(self.words(z, s, i)), False))

    def put_point(self, z, s, i, coords):
        self.put_words(z, s, i, self.O.arr_to_ints(self.O.fq_convert_montgomery(self.O.ints_to_arr([c % Q for c in coords]), True)))

    def y_plus_one(self, z, s, i):
        """CONSTRUCTED fault: y ← y + 1 (first component of y for a G2 point) — off the curve"""
        p = self.point(z, s, i)
        p[len(p) // 2] = (p[len(p) // 2] + 1) % Q
        self.put_point(z, s, i, p)


@pytest.fixture(scope="module")
def key(gpu, O, S):
    return Key(gpu, O, S)


def _expect(rep, kind, section, index, faults):
    assert (rep.kind, rep.section, rep.index) == (kind, section, index), (rep.kind, rep.section, rep.index)
    assert list(rep.faults) == [faults.get(s, 0) for s in range(10)], list(rep.faults)


def test_the_key_has_the_shape_the_cases_need(key):
    """conditions on the inputs, checked against the synthesiser — not measurements"""
    assert 129 <= key.n_vars <= 191 and key.domain == 256 and key.n_public == 2
    assert [key.count(s) for s in (3, 5, 6, 7, 8, 9)] == [3, key.n_vars, key.n_vars, key.n_vars, key.n_vars - 3, 256]
    zero = [not any(key.words(key.zkey, 7, i)) for i in range(key.n_vars)]
    assert any(zero) and not all(zero)
    i, j = _swap_pair(key)
    assert i != j and any(key.words(key.zkey, 6, i)) and any(key.words(key.zkey, 6, j))
    assert key.words(key.zkey, 6, i) != key.words(key.zkey, 6, j)
    assert any(key.words(key.zkey, 7, i)) and any(key.words(key.zkey, 7, j))


def _swap_pair(key):
    live = [i for i in range(key.n_vars) if any(key.words(key.zkey, 7, i))]
    return live[0], live[-1]


def test_untouched_key_is_sound(gpu, key):
    ok, rep = gpu.zkey_check(key.zkey, seed=SEED)
    assert ok is True
    _expect(rep, 0, 0, 0, {})
    assert rep.device_ms > 0 and rep.upload_ms > 0 and rep.pairing_ms > 0
    ok, rep = gpu.zkey_check(key.zkey, slice_points=64, seed=SEED)
    assert ok is True
    _expect(rep, 0, 0, 0, {})
    for seed in SEEDS:
        ok, rep = gpu.zkey_check(key.zkey, seed=seed)
        assert ok is True, seed.hex()
    ok, rep = gpu.zkey_check(key.zkey)            # a seed from the operating system
    assert ok is True
    ok, rep = gpu.zkey_check(bytearray(key.zkey), device="HIP:0", seed=SEED)
    assert ok is True


@pytest.mark.parametrize("section", [3, 5, 6, 8, 9])
def test_one_damaged_point(gpu, key, section):
    last = key.count(section) - 1
    for index in sorted({i for i in (0, 63, 64, last) if i <= last}):
        z = bytearray(key.zkey)
        key.y_plus_one(z, section, index)
        for slice_points in (0, 64):
            ok, rep = gpu.zkey_check(z, slice_points=slice_points, seed=SEED)
            assert ok is False
            _expect(rep, OFF_CURVE, section, index, {section: 1})


def test_two_faults_in_one_section_and_one_in_each_of_two(gpu, key):
    z = bytearray(key.zkey)
    for i in (130, 70, 129):                      # CONSTRUCTED: three damaged points of section 5, out of order
        key.y_plus_one(z, 5, i)
    ok, rep = gpu.zkey_check(z, seed=SEED)
    assert ok is False
    _expect(rep, OFF_CURVE, 5, 70, {5: 3})
    ok, rep = gpu.zkey_check(z, slice_points=64, seed=SEED)
    _expect(rep, OFF_CURVE, 5, 70, {5: 3})
    z = bytearray(key.zkey)
    key.y_plus_one(z, 9, 5)                       # CONSTRUCTED: one fault in section 9, a later one in section 8
    key.y_plus_one(z, 8, 100)
    ok, rep = gpu.zkey_check(z, seed=SEED)
    assert ok is False
    _expect(rep, OFF_CURVE, 8, 100, {8: 1, 9: 1})


def test_non_canonical_coordinate(gpu, key):
    z = bytearray(key.zkey)
    w = key.words(z, 5, 77)
    key.put_words(z, 5, 77, [Q, w[1]])            # CONSTRUCTED: x := q, not a residue
    key.y_plus_one(z, 5, 78)                      # and an off-curve neighbour: the lower index and its kind win
    ok, rep = gpu.zkey_check(z, seed=SEED)
    assert ok is False
    _expect(rep, NONCANONICAL, 5, 77, {5: 2})
    z = bytearray(key.zkey)
    key.put_words(z, 7, 3, [0, 0, 0, (1 << 256) - 1])   # CONSTRUCTED: a G2 coordinate of all ones
    ok, rep = gpu.zkey_check(z, seed=SEED)
    _expect(rep, NONCANONICAL, 7, 3, {7: 1})


@pytest.mark.parametrize("slot", [0, 2, 5])
def test_identity_in_a_header_slot(gpu, key, slot):
    z = bytearray(key.zkey)
    key.put_words(z, 2, slot, [0] * (HEADER_SLOTS[slot][1] // 32))   # CONSTRUCTED: the point replaced by the identity
    ok, rep = gpu.zkey_check(z, seed=SEED)
    assert ok is False
    _expect(rep, IDENTITY, 2, slot, {2: 1})


def test_header_point_off_the_curve(gpu, key):
    z = bytearray(key.zkey)
    key.y_plus_one(z, 2, 3)                       # CONSTRUCTED: γ₂ with y + 1
    ok, rep = gpu.zkey_check(z, seed=SEED)
    assert ok is False
    _expect(rep, OFF_CURVE, 2, 3, {2: 1})


def test_section_7_subgroup_and_twist(gpu, key):
    i, _ = _swap_pair(key)
    z = bytearray(key.zkey)
    key.put_point(z, 7, i, M.twist_point_outside_subgroup())   # CONSTRUCTED: on the twist, outside the order-r subgroup
    ok, rep = gpu.zkey_check(z, seed=SEED)
    assert ok is False
    _expect(rep, OFF_SUBGROUP, 7, i, {7: 1})
    ok, rep = gpu.zkey_check(z, slice_points=64, seed=SEED)
    _expect(rep, OFF_SUBGROUP, 7, i, {7: 1})
    z = bytearray(key.zkey)
    key.y_plus_one(z, 7, 128)                     # CONSTRUCTED: off the twist
    ok, rep = gpu.zkey_check(z, seed=SEED)
    assert ok is False
    _expect(rep, OFF_CURVE, 7, 128, {7: 1})


def test_a_section_of_bad_points(gpu, key):
    z = bytearray(key.zkey)
    for i in range(256):                          # CONSTRUCTED: every y of section 9 zeroed
        w = key.words(z, 9, i)
        assert w[0], "an H point with x = 0 would become the identity"
        key.put_words(z, 9, i, [w[0], 0])
    for slice_points in (0, 64):
        ok, rep = gpu.zkey_check(z, slice_points=slice_points, seed=SEED)
        assert ok is False
        _expect(rep, OFF_CURVE, 9, 0, {9: 256})


def test_b1_b2_mismatch(gpu, key):
    i, j = _swap_pair(key)
    z = bytearray(key.zkey)
    wi, wj = key.words(z, 6, i), key.words(z, 6, j)
    key.put_words(z, 6, i, wj)                    # CONSTRUCTED: B1ᵢ and B1ⱼ swapped — both still on the curve
    key.put_words(z, 6, j, wi)
    for seed in SEEDS:
        ok, rep = gpu.zkey_check(z, seed=seed)
        assert ok is False, seed.hex()
        _expect(rep, PAIR_MISMATCH, 6, U64_MAX, {6: 1})
    ok, rep = gpu.zkey_check(z, slice_points=64, seed=SEED)
    _expect(rep, PAIR_MISMATCH, 6, U64_MAX, {6: 1})


def test_consistent_replacement_passes(gpu, key):
    """the control: B1ᵢ and B2ᵢ replaced TOGETHER by [k]G₁ and [k]G₂ — the check tests consistency, not a particular value"""
    K = gpu
    i, _ = _swap_pair(key)
    k = np.frombuffer((0x1234567890abcdef12345).to_bytes(32, "little"), dtype=np.uint64).reshape(1, 4)
    z = bytearray(key.zkey)
    key.put_point(z, 6, i, key.O.arr_to_ints(K.generator_mul("g1", k).reshape(-1, 4)))
    key.put_point(z, 7, i, key.O.arr_to_ints(K.generator_mul("g2", k).reshape(-1, 4)))
    assert bytes(z) != key.zkey
    ok, rep = K.zkey_check(z, seed=SEED)
    assert ok is True
    _expect(rep, 0, 0, 0, {})
    key.put_point(z, 7, i, key.O.arr_to_ints(K.generator_mul("g2", k + np.uint64(1)).reshape(-1, 4)))   # … and apart again
    ok, rep = K.zkey_check(z, seed=SEED)
    _expect(rep, PAIR_MISMATCH, 6, U64_MAX, {6: 1})


def test_header_pair_mismatch(gpu, key):
    K = gpu
    z = bytearray(key.zkey)
    beta1 = np.array(key.O.ints_to_arr(key.point(z, 2, 1)))
    two = K.ec("g1", "to_affine", K.ec("g1", "mul_scalar", K.ec("g1", "from_affine", beta1), 2))
    key.put_point(z, 2, 1, key.O.arr_to_ints(two))          # CONSTRUCTED: β₁ ← [2]β₁, a sound point that no longer matches β₂
    ok, rep = K.zkey_check(z, seed=SEED)
    assert ok is False
    _expect(rep, PAIR_MISMATCH, 2, 1, {2: 1})


def test_section_4(gpu, key):
    K = gpu
    off, ln = key.sec[4]
    n_coef = (ln - 4) // 44
    z = bytearray(key.zkey)
    rec = 17
    struct.pack_into("<I", z, off + 4 + 44 * rec + 8, key.n_vars)   # CONSTRUCTED: a wire index equal to n_vars
    ok, rep = K.zkey_check(z, seed=SEED)
    assert ok is False
    _expect(rep, COEFFICIENT, 4, rec, {4: 1})
    cm = K.CacheManager()
    try:
        with pytest.raises(K.ProverError, match="out of range"):
            cm.load("bad-wire", bytes(z))
    finally:
        cm.close()
    z = bytearray(key.zkey)
    last = n_coef - 1
    z[off + 4 + 44 * last + 12:off + 4 + 44 * last + 44] = M.R.to_bytes(32, "little")   # CONSTRUCTED: a value equal to r
    struct.pack_into("<I", z, off + 4 + 44 * 3 + 4, 256)                               # and a constraint index equal to the domain size
    ok, rep = K.zkey_check(z, slice_points=64, seed=SEED)
    _expect(rep, COEFFICIENT, 4, 3, {4: 2})


def test_malformed_files_are_errors_not_verdicts(gpu, key):
    K = gpu
    with pytest.raises(K.ProverError):
        K.zkey_check(key.zkey[:len(key.zkey) // 2], seed=SEED)
    with pytest.raises(K.ProverError):
        K.zkey_check(key.zkey, device="CPU", seed=SEED)
    with pytest.raises(K.ProverError, match="cannot open"):
        K.zkey_check_file("/nonexistent/key.zkey", seed=SEED)


def _devices(K):
    dev = K.Device()
    K.check(K.lib().icicle_get_active_device(C.byref(dev)), "get_active_device")
    hip = C.c_int(-1)
    C.CDLL("libamdhip64.so").hipGetDevice(C.byref(hip))
    return dev.type, dev.id, hip.value


def test_after_a_check_the_key_still_proves(gpu, key, O, tmp_path):
    K = gpu
    before = _devices(K)
    ok, _ = K.zkey_check(key.zkey, seed=SEED)
    assert ok is True
    path = tmp_path / "k.zkey"
    path.write_bytes(key.zkey)
    ok, rep = K.zkey_check_file(str(path), seed=SEED)
    assert ok is True
    _expect(rep, 0, 0, 0, {})
    assert _devices(K) == before                  # DeviceSession restored the thread's device
    cm = K.CacheManager()
    try:
        cm.load("checked", key.zkey)
        pj, qj, _ = cm.prove_mem("checked", key.wtns, 3, 5)
        proof, public = O.groth16_prove(key.zkey, key.wtns, 3, 5)
        assert json.loads(pj) == proof and json.loads(qj) == public
        assert K.groth16_verify_json(pj, qj, K.zkey_export_vk(key.zkey)) is True
    finally:
        cm.close()
        K.release_domain()


def test_repl_commands(gpu, tmp_path):
    K = gpu
    zkey = base64.b64decode(load_golden("groth16.json")["zkey"])
    (tmp_path / "g.zkey").write_bytes(zkey)
    bad = bytearray(zkey)
    sec = _sections(zkey)
    bad[sec[5][0] + 64 * 2 + 32] ^= 1             # CONSTRUCTED: one bit of A₂'s y
    (tmp_path / "bad.zkey").write_bytes(bad)
    exe = os.path.join(ROOT, "icicle-snark_amd", "lib", "prove")
    cmds = (f"zkey-check --zkey {tmp_path}/g.zkey --device HIP\n"
            f"zkey-export-vk --zkey {tmp_path}/g.zkey --vk {tmp_path}/vk.json\n"
            f"zkey-check --zkey {tmp_path}/bad.zkey\n"
            f"zkey-check --zkey {tmp_path}/missing.zkey\nexit\n")
    out = subprocess.run([exe], input=cmds, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.count("COMMAND_COMPLETED") == 5 and "COMMAND_EXIT" in out.stdout
    lines = [ln.replace("> ", "") for ln in out.stdout.splitlines()]
    assert lines.count("sound") == 1 and lines.count("unsound") == 1 and "VK_WRITTEN" in lines
    assert "section 5: 1 at fault, first: point off the curve at index 2" in lines
    assert "zkey-check failed (-1)" in out.stderr
    assert (tmp_path / "vk.json").read_text() == K.zkey_export_vk(zkey)
    help_text = subprocess.run([exe], input="nonsense\nexit\n", capture_output=True, text=True, timeout=300).stdout
    assert "zkey-check --zkey <file> [--device HIP]" in help_text and "zkey-export-vk --zkey <file> --vk <file>" in help_text
