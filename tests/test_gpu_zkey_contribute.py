"""groth16_zkey_contribute on the GPU (needs an MI355X): a phase-2 contribution δ′ applied to a proving key.  Expected bytes never
come from the library: sections 1 to 9 are the synthesiser's — contributing δ′ to setup(…, toxic=(τ, α, β, γ, δ)) must give exactly
setup(…, toxic=(τ, α, β, γ, δ·δ′)) — and section 10 is the Python model's (tests/zkey_contribute_model.py).  The circuits are
tests/zkey_new_circuits.py's over a power-8 ptau: `mixed` has 163 + 256 points in sections 8 and 9 (no multiple of the kernel's
64-lane blocks, an all-zero wire and a cancelling wire: identity points), `tiny` an empty section 8."""
import ctypes as C
import json
import os
import struct
import subprocess

import pytest

import zkey_contribute_model as ZM
import zkey_new_circuits as ZC

pytestmark = pytest.mark.gpu

R = ZM.R
SEED = bytes(range(32))
S1, S2 = bytes([0x51]) * 32, bytes(range(100, 132))
NAMES = [b"a", b"b"]
CIRCUITS = ["mixed", "chain7", "tiny"]
COPIED = [1, 2, 3, 5, 6, 7, 8, 9]          # compared as bytes; section 4 as records (zkey-new's stated order is not setup()'s)


class World:
    def __init__(self, K, O, S):
        self.K, self.S = K, S
        self.fbm = lambda g, sc: K.generator_mul(g, sc)
        self.to_mont = lambda a: O.fq_convert_montgomery(a, True)
        self.ptau = S.write_ptau(8, self.fbm, points_to_mont=self.to_mont)
        self.toxic = S.toxic_waste()
        self.g1 = ZM.G1Bytes(O)
        self.circuits = {n: r for n, r in ZC.circuits(S).items() if n in CIRCUITS}
        self.handles = {n: K.R1cs(S.write_r1cs(r)) for n, r in self.circuits.items()}
        self.d = [1, ZM.delta_of(S1), ZM.delta_of(S1) * ZM.delta_of(S2) % R]
        self._want, self._chain = {}, {}

    def want(self, name, delta, gamma=1):
        """the synthesiser's key of the circuit with this γ and δ over the ptau's τ, α, β"""
        if (name, delta, gamma) not in self._want:
            self._want[name, delta, gamma] = self.S.setup(self.circuits[name], self.fbm, points_to_mont=self.to_mont, toxic=self.toxic[:3] + (gamma, delta))[0]
        return self._want[name, delta, gamma]

    def chain(self, name):
        """[zkey-new's key, after S1 / "a", after S2 / "b"] and the two reports"""
        if name not in self._chain:
            k0, _ = self.handles[name].new_zkey(self.ptau)
            k1, r1 = self.K.zkey_contribute(k0, secret=S1, name="a")
            k2, r2 = self.K.zkey_contribute(k1, secret=S2, name="b")
            self._chain[name] = ([k0, k1, k2], [r1, r2])
        return self._chain[name]

    def close(self):
        for h in self.handles.values():
            h.close()


@pytest.fixture(scope="module")
def world(gpu, O, S):
    w = World(gpu, O, S)
    yield w
    w.close()


def _devices(K):
    dev = K.Device()
    K.check(K.lib().icicle_get_active_device(C.byref(dev)), "get_active_device")
    hip = C.c_int(-1)
    C.CDLL("libamdhip64.so").hipGetDevice(C.byref(hip))
    return dev.type, dev.id, hip.value


def _same_1_to_9(got, want, what):
    order = ZC.sections(got)[1]
    assert order == list(range(1, 11)) and got[:8] == want[:8], what
    for sid in COPIED:
        assert ZC.payload(got, sid) == ZC.payload(want, sid), (what, sid)
    assert sorted(ZC.records(got)) == sorted(ZC.records(want)), what


def test_the_inputs_have_the_shape_the_cases_need(world):
    """conditions, checked against the synthesiser — not measurements"""
    shape = lambda n: (len(ZC.payload(world.want(n, 1), 8)) // 64, len(ZC.payload(world.want(n, 1), 9)) // 64)
    assert shape("mixed") == (163, 256) and shape("chain7") == (7, 16) and shape("tiny") == (0, 8)
    assert (163 + 256) % 64 and 163 + 256 > 64                                     # a last block that is not full, more than one block
    c = ZC.payload(world.want("mixed", world.d[1]), 8)
    assert c[(165 - 3) * 64:(166 - 3) * 64] == bytes(64) and c[:64] != bytes(64)   # an identity point among the others
    assert 1 < world.d[1] < R and 1 < world.d[2] < R and world.d[1] != world.d[2]
    # δ only moves the header's δ₁, δ₂ and sections 8 and 9
    a, b = world.want("mixed", 1), world.want("mixed", world.d[1])
    assert [s for s in range(1, 11) if ZC.payload(a, s) != ZC.payload(b, s)] == [2, 8, 9]
    assert ZC.payload(a, 2)[:468] == ZC.payload(b, 2)[:468]


@pytest.mark.parametrize("name", CIRCUITS)
def test_every_byte_is_the_synthesisers_and_the_models(world, name, tmp_path):
    K = world.K
    before = _devices(K)
    keys, reps = world.chain(name)
    n8, n9 = (len(ZC.payload(keys[0], s)) // 64 for s in (8, 9))
    for i in (1, 2):
        _same_1_to_9(keys[i], world.want(name, world.d[i]), (name, i))
        assert ZC.payload(keys[i], 4) == ZC.payload(keys[0], 4)                      # copied, byte for byte
        model, delta = ZM.contribute(keys[i - 1], world.d[i - 1], (S1, S2)[i - 1], NAMES[i - 1], world.g1)
        assert ZC.payload(keys[i], 10) == model and delta == ZM.delta_of((S1, S2)[i - 1]), (name, i)
        rep = reps[i - 1]
        assert (rep.contribution, rep.points_c, rep.points_h, rep.zkey_bytes) == (i, n8, n9, len(keys[i]))
        assert len(keys[i]) == len(keys[i - 1]) + 164 + 1 and rep.faults == 0 and rep.device_ms > 0 and rep.download_ms > 0
    # the file entry writes the same bytes, and leaves nothing else behind
    src, out = tmp_path / "in.zkey", tmp_path / "out.zkey"
    src.write_bytes(keys[0])
    none, rep = K.zkey_contribute(str(src), secret=S1, name=b"a", out=out)
    assert none is None and out.read_bytes() == keys[1] and rep.write_ms > 0
    assert sorted(os.listdir(tmp_path)) == ["in.zkey", "out.zkey"]
    assert _devices(K) == before


def test_a_key_with_other_gamma_and_delta(world):
    """setup()'s default key: γ, δ ≠ 1.  Section 4 is setup()'s own here, so all of 1 to 9 are bytes."""
    K, S = world.K, world.S
    gamma, delta = world.toxic[3:]
    key = world.want("chain7", delta, gamma)
    assert key == S.setup(world.circuits["chain7"], world.fbm, points_to_mont=world.to_mont)[0] and gamma != 1 and delta != 1
    got, rep = K.zkey_contribute(key, secret=S1, name="a")
    want = world.want("chain7", delta * world.d[1] % R, gamma)
    for sid in range(1, 10):
        assert ZC.payload(got, sid) == ZC.payload(want, sid), sid
    assert ZC.payload(got, 10) == ZM.contribute(key, delta, S1, b"a", world.g1)[0] and rep.contribution == 1
    # the chain did not start from δ = 1: the audit says so at record 1
    ok, crep = K.zkey_contributions(got)
    assert (ok, crep.count, crep.kind, crep.index) == (False, 1, K.CONTRIB_POK, 1)
    # a key without section 10: the section is appended, with its header
    secs, order = ZC.sections(key)
    bare = key[:8] + struct.pack("<I", 9) + b"".join(key[secs[s][0] - 12:secs[s][0] + secs[s][1]] for s in order if s != 10)
    got2, rep2 = K.zkey_contribute(bare, secret=S1, name="a")
    assert got2 == got and rep2.zkey_bytes == len(bare) + 12 + 4 + 165


@pytest.mark.parametrize("inverse", [1, 2, R - 1, 3 << 252, (R + 1) // 2, ZM.FULL], ids=["1", "2", "r-1", "3*2^252", "(r+1)/2", "full"])
def test_edge_scalars_through_the_kernel(world, inverse):
    """δ′ chosen so that the kernel's scalar δ′⁻¹ is the edge: the shortest walks, −P, the 255-digit form, r/2, full width"""
    delta = pow(inverse, -1, R)
    assert delta * inverse % R == 1 and 0 < delta < R
    k0 = world.chain("chain7")[0][0]
    got, _ = world.K.zkey_contribute(k0, secret=S1, name="edge", delta=delta)
    _same_1_to_9(got, world.want("chain7", delta), hex(inverse))
    assert ZC.payload(got, 10) == ZM.contribute(k0, 1, S1, b"edge", world.g1, delta=delta)[0]
    if inverse == 1:                                                                  # δ′ = 1: nothing but section 10 moves
        assert all(ZC.payload(got, s) == ZC.payload(k0, s) for s in range(1, 10))


@pytest.mark.parametrize("name", CIRCUITS)
def test_the_librarys_own_judges_accept_the_key(world, name):
    K, h = world.K, world.handles[name]
    key = world.chain(name)[0][2]
    ok, rep = K.zkey_check(key, seed=SEED)
    assert ok is True and rep.kind == 0
    ok, rep = h.match_zkey(key, seed=SEED)
    assert ok is True and rep.kind == 0
    ok, rep = h.verify_zkey(key, world.ptau, seed=SEED)
    assert ok is True and (rep.kind, rep.failed_mask) == (0, 0)
    ok, rep = K.zkey_contributions(key)
    assert ok is True and (rep.count, rep.kind, rep.index) == (2, 0, 0) and [n for _, n in rep.records] == NAMES
    assert rep.records[1][0] == ZC.payload(key, 2)[468:532] == world.g1(world.d[2])


def _witnesses(S):
    """name → (a witness that satisfies the circuit, the wire to spoil)"""
    return {"mixed": (ZC.mixed(S)[1], 40), "chain7": (S.squaring_chain(7)[1], 3)}


@pytest.mark.parametrize("name", ["mixed", "chain7"])
def test_the_key_loads_proves_and_verifies(world, S, name):
    """(`tiny` has no private wire: its key has an empty section 8, which no prove of this suite has ever been given — the bytes
    and the judges above cover it, a prove of it would test the prover and not the contribution)"""
    K = world.K
    w, spoil = _witnesses(S)[name]
    r = world.circuits[name]
    assert ZC.check_r1cs(r, w)
    key = world.chain(name)[0][2]
    vk = K.zkey_export_vk(key)
    cm = K.CacheManager()
    try:
        cm.load("contributed", key)
        pj, qj, _ = cm.prove_mem("contributed", S.write_wtns(w), 3, 5)
        assert json.loads(qj) == [str(v) for v in w[1:1 + r.n_public]]
        assert K.groth16_verify_json(pj, qj, vk) is True
        bad = list(w)
        bad[spoil] = (bad[spoil] + 1) % R                               # CONSTRUCTED: one wire off by one
        assert not ZC.check_r1cs(r, bad)
        pj, qj, _ = cm.prove_mem("contributed", S.write_wtns(bad), 3, 5)
        assert K.groth16_verify_json(pj, qj, vk) is False
    finally:
        cm.close()


@pytest.mark.parametrize("stale, kind", [(9, "H"), (8, "C")])
def test_a_stale_half_fails(world, stale, kind):
    """CONSTRUCTED: the contributed key with one of the two scaled sections taken from the uncontributed key — both sections
    really were scaled, or verify_zkey names the one that was not, and that one alone"""
    K = world.K
    keys = world.chain("mixed")[0]
    key = ZM.with_section(keys[2], stale, ZC.payload(keys[0], stale))
    assert ZC.payload(key, stale) != ZC.payload(keys[2], stale) and len(key) == len(keys[2])
    ok, rep = world.handles["mixed"].verify_zkey(key, world.ptau, seed=SEED)
    k = K.VERIFY_KIND_NAMES.index(kind)
    assert ok is False and rep.kind == k and rep.failed_mask == 1 << (k - K.VERIFY_HEADER)
    assert K.zkey_contributions(key)[0] is True                         # the audit of section 10 does not look at 8 and 9


def _bump(image, offset):
    """the 32-byte little-endian coordinate at `offset`, plus one"""
    e = bytearray(image)
    e[offset:offset + 32] = ((int.from_bytes(e[offset:offset + 32], "little") + 1) % (1 << 256)).to_bytes(32, "little")
    return bytes(e)


def test_errors(world, tmp_path):
    K = world.K
    before = _devices(K)
    k0 = world.chain("mixed")[0][0]
    secs = ZC.sections(k0)[0]
    # CONSTRUCTED: one coordinate of one point, plus one — in the first block, in a middle block, in the last, not full, block
    for sid, elem, coord in ((8, 5, 0), (8, 162, 1), (9, 0, 1), (9, 200, 0), (9, 255, 1)):
        bad = _bump(k0, secs[sid][0] + 64 * elem + 32 * coord)
        with pytest.raises(K.ProverError, match=r"\(-2\).*section %d, element %d: the point is not on the curve \(1 points" % (sid, elem)):
            K.zkey_contribute(bad, secret=S1, name="a")
    bad = _bump(_bump(k0, secs[8][0] + 64 * 100), secs[9][0] + 64 * 7)
    with pytest.raises(K.ProverError, match=r"\(-2\).*section 8, element 100: .* \(2 points"):
        K.zkey_contribute(bad, secret=S1, name="a")
    path, out = tmp_path / "bad.zkey", tmp_path / "never.zkey"
    path.write_bytes(bad)
    with pytest.raises(K.ProverError, match=r"\(-2\).*section 8, element 100"):
        K.zkey_contribute(path, secret=S1, name="a", out=out)
    assert sorted(os.listdir(tmp_path)) == ["bad.zkey"]               # neither the key nor a temporary
    rep = K.ZkeyContributeReport()
    buf = C.create_string_buffer(len(k0) + 165)
    rc = K.lib().groth16_zkey_contribute(C.c_char_p(bad), C.c_size_t(len(bad)), S1, b"a", buf, C.c_size_t(len(buf)), b"HIP", None, C.byref(rep))
    assert rc == -2 and (rep.fault_section, rep.fault_index, rep.fault_kind, rep.faults) == (8, 100, K.ZKEY_OFF_CURVE, 2)
    # a coordinate not below q
    e = bytearray(k0)
    e[secs[9][0] + 64 * 3:secs[9][0] + 64 * 3 + 32] = ZM.Q.to_bytes(32, "little")
    with pytest.raises(K.ProverError, match=r"\(-2\).*section 9, element 3: a coordinate is not below q"):
        K.zkey_contribute(bytes(e), secret=S1, name="a")
    # a malformed section 10, and one that does not end in the header's δ₁
    k1 = world.chain("mixed")[0][1]
    for payload in (struct.pack("<I", 1), struct.pack("<I", 0) + b"\0", ZC.payload(k1, 10)[:-1], b"\0\0"):
        with pytest.raises(K.ProverError, match=r"\(-2\).*section 10 is malformed"):
            K.zkey_contribute(ZM.with_section(k0, 10, payload), secret=S1, name="a")
    with pytest.raises(K.ProverError, match=r"\(-2\).*last record is not the header's delta1"):
        K.zkey_contribute(ZM.with_section(k0, 10, ZC.payload(k1, 10)), secret=S1, name="a")
    # cap one byte short: −3, the report says what is needed, nothing is written
    need = len(k0) + 164 + 1
    buf = C.create_string_buffer(need)
    rc = K.lib().groth16_zkey_contribute(C.c_char_p(k0), C.c_size_t(len(k0)), S1, b"a", buf, C.c_size_t(need - 1), b"HIP", None, C.byref(rep))
    assert rc == -3 and rep.zkey_bytes == need and buf.raw == bytes(need)
    rc = K.lib().groth16_zkey_contribute(C.c_char_p(k0), C.c_size_t(len(k0)), S1, b"a", buf, C.c_size_t(need), b"HIP", None, C.byref(rep))
    assert rc == 0 and buf.raw == k1
    for delta in (0, R):
        with pytest.raises(K.ProverError, match=r"\(-3\).*fixed_delta"):
            K.zkey_contribute(k0, secret=S1, name="a", delta=delta)
    with pytest.raises(K.ProverError, match=r"\(-3\).*name has 256 bytes"):
        K.zkey_contribute(k0, secret=S1, name=b"n" * 256)
    assert len(K.zkey_contribute(k0, secret=S1, name=b"n" * 255)[0]) == len(k0) + 164 + 255
    with pytest.raises(K.ProverError, match=r"\(-1\).*cannot open"):
        K.zkey_contribute(tmp_path / "missing.zkey", secret=S1, name="a", out=tmp_path / "never.zkey")
    good = tmp_path / "good.zkey"
    good.write_bytes(k0)
    with pytest.raises(K.ProverError, match=r"\(-3\).*the output path is the input's"):
        K.zkey_contribute(good, secret=S1, name="a", out=good)
    assert good.read_bytes() == k0 and sorted(os.listdir(tmp_path)) == ["bad.zkey", "good.zkey"]
    assert _devices(K) == before
    # a following good call is as good as before; and without a secret the operating system's is drawn: two calls differ
    assert K.zkey_contribute(k0, secret=S1, name="a")[0] == k1
    a, b = K.zkey_contribute(k0, name="os")[0], K.zkey_contribute(k0, name="os")[0]
    assert a != b and ZC.payload(a, 4) == ZC.payload(b, 4) and K.zkey_contributions(a)[0] is True and K.zkey_contributions(b)[0] is True


def test_the_repl_contributes_and_audits(world, S, tmp_path):
    K = world.K
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    k0 = world.chain("chain7")[0][0]
    (tmp_path / "k0.zkey").write_bytes(k0)
    cmds = (f"zkey-contribute --zkey {tmp_path}/k0.zkey --out {tmp_path}/k1.zkey --name first --device HIP\n"
            f"zkey-contribute --zkey {tmp_path}/k1.zkey --out {tmp_path}/k2.zkey\n"
            f"zkey-contributions --zkey {tmp_path}/k2.zkey\n"
            f"zkey-contributions --zkey {tmp_path}/k0.zkey\n"
            f"zkey-contribute --zkey {tmp_path}/missing.zkey --out {tmp_path}/never.zkey\nnonsense\nexit\n")
    out = subprocess.run([os.path.join(root, "icicle-snark_amd", "lib", "prove")], input=cmds, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [ln.replace("> ", "") for ln in out.stdout.splitlines()]
    assert lines[0].startswith("contribution 1 points C 7 H 16 bytes %d; upload " % (len(k0) + 164 + 5))
    assert lines[1:3] == ["ZKEY_WRITTEN", "COMMAND_COMPLETED"]
    assert lines[3].startswith("contribution 2 points C 7 H 16 bytes %d; upload " % (len(k0) + 2 * 164 + 5)) and lines[4:6] == ["ZKEY_WRITTEN", "COMMAND_COMPLETED"]
    assert lines[6].startswith('contribution 1 name "first" delta1 ') and lines[7].startswith('contribution 2 name "" delta1 ')
    assert lines[8:12] == ["CHAIN_OK", "COMMAND_COMPLETED", "CHAIN_OK", "COMMAND_COMPLETED"]
    assert lines[12] == "COMMAND_COMPLETED" and "zkey-contribute failed (-1)" in out.stderr
    assert "zkey-contribute --zkey <file> --out <file> [--name <text>] [--device HIP]" in out.stdout and "zkey-contributions --zkey <file>" in out.stdout
    assert not (tmp_path / "never.zkey").exists()
    # δ′ was the operating system's: the structure, the library's judges and a proof — not bytes
    k2 = (tmp_path / "k2.zkey").read_bytes()
    assert ZC.sections(k2)[1] == list(range(1, 11)) and len(k2) == len(k0) + 2 * 164 + 5
    assert all(ZC.payload(k2, s) == ZC.payload(k0, s) for s in (1, 3, 4, 5, 6, 7)) and ZC.payload(k2, 2)[:468] == ZC.payload(k0, 2)[:468]
    assert all(ZC.payload(k2, s) != ZC.payload(k0, s) for s in (8, 9))
    ok, rep = K.zkey_contributions(k2)
    assert ok is True and rep.count == 2 and [n for _, n in rep.records] == [b"first", b""]
    ok, rep = world.handles["chain7"].verify_zkey(k2, world.ptau, seed=SEED)
    assert ok is True and (rep.kind, rep.failed_mask) == (0, 0)
    w = S.squaring_chain(7)[1]
    cm = K.CacheManager()
    try:
        cm.load("repl", k2)
        pj, qj, _ = cm.prove_mem("repl", S.write_wtns(w), 3, 5)
        assert K.groth16_verify_json(pj, qj, K.zkey_export_vk(k2)) is True
    finally:
        cm.close()
