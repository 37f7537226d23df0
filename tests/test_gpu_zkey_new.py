"""groth16_zkey_new on the GPU (needs an MI355X): the proving key of an .r1cs over a prepared .ptau, before any contribution.
The expected key is the synthesiser's: setup(r, …, toxic=(τ, α, β, 1, 1)) over the τ, α, β of write_ptau() writes, byte for byte,
what the library must write (affine points are canonical: the comparison is of bytes) — never anything the library computed.
The ptaus have power 8 and power 10 (the blocks that are read begin in the middle of their sections); the circuits are
tests/zkey_new_circuits.py's, at most a few hundred constraints each."""
import ctypes as C
import json
import os
import struct

import pytest

import zkey_new_circuits as ZC

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))
ALL = ["mixed", "fan", "chain6", "chain7", "tiny"]
POINT_SECTIONS = [1, 2, 3, 5, 6, 7, 8, 9, 10]


class World:
    def __init__(self, K, O, S):
        self.K, self.S = K, S
        self.fbm = lambda g, sc: K.generator_mul(g, sc)
        self.to_mont = lambda a: O.fq_convert_montgomery(a, True)
        self.ptau = {p: S.write_ptau(p, self.fbm, points_to_mont=self.to_mont) for p in (8, 10)}
        tau, alpha, beta = S.toxic_waste()[:3]
        self.circuits = ZC.circuits(S)
        self.want = {n: S.setup(r, self.fbm, points_to_mont=self.to_mont, toxic=(tau, alpha, beta, 1, 1))[0] for n, r in self.circuits.items()}
        self.handles = {n: K.R1cs(S.write_r1cs(r)) for n, r in self.circuits.items()}
        self.domain = {n: S.key_scalars(r)["n"] for n, r in self.circuits.items()}

    def powers(self, name):
        return [p for p in (8, 10) if (1 << p) >= self.domain[name]]

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


def _same_key(world, name, got, rep=None):
    want, r = world.want[name], world.circuits[name]
    assert ZC.sections(got)[1] == list(range(1, 11)) and got[:12] == want[:12]
    for sid in POINT_SECTIONS:
        assert ZC.payload(got, sid) == ZC.payload(want, sid), (name, sid)
    recs = ZC.records(got)
    assert len(recs) == len(ZC.records(want)) and sorted(recs) == sorted(ZC.records(want))
    assert recs == ZC.stated_records(r), name                       # the stated order: by constraint, A then B, then the binding rows
    assert len(got) == len(want)
    if rep is not None:
        assert (rep.n_vars, rep.n_public, rep.domain, rep.n_coeffs, rep.zkey_bytes) == (r.n_vars, r.n_public, world.domain[name], len(recs), len(want))
        longest = max(sum(1 for t in mat if t[1] == s) + (1 if k == 0 and s <= r.n_public else 0) for k, mat in enumerate((r.A, r.B, r.C)) for s in range(r.n_vars))
        assert rep.longest_column == longest and rep.device_ms > 0 and rep.upload_ms > 0 and rep.download_ms > 0


def test_the_inputs_have_the_shape_the_cases_need(world, S):
    """conditions, checked against the synthesiser — not measurements"""
    shape = lambda r: (r.n_vars, r.n_public, r.n_constraints)
    c, d = world.circuits, world.domain
    assert (shape(c["mixed"]), d["mixed"]) == ((166, 2, 158), 256)
    assert (shape(c["fan"]), d["fan"]) == ((303, 1, 300), 512)
    assert (shape(c["chain6"]), d["chain6"]) == ((8, 1, 6), 8) and (shape(c["chain7"]), d["chain7"]) == ((9, 1, 7), 16)
    assert (shape(c["tiny"]), d["tiny"]) == ((3, 2, 2), 8) and ZC.sections(world.want["tiny"])[0][8][1] == 0
    assert world.powers("fan") == [10] and all(world.powers(n) == [8, 10] for n in ALL if n != "fan")
    # γ = δ = 1: the header's δ₁ is G₁, γ₂ and δ₂ are G₂
    hdr = ZC.payload(world.want["mixed"], 2)
    g = world.to_mont(world.fbm("g1", S.ints_to_arr([1]))).tobytes(), world.to_mont(world.fbm("g2", S.ints_to_arr([1]))).tobytes()
    assert hdr[340:468] == g[1] and hdr[468:532] == g[0] and hdr[532:660] == g[1]
    for p in (8, 10):
        secs = ZC.sections(world.ptau[p])[0]
        assert hdr[84:148] == world.ptau[p][secs[4][0]:secs[4][0] + 64] and hdr[212:340] == world.ptau[p][secs[6][0]:secs[6][0] + 128]
    # a wire in no matrix is all-zero bytes in every section
    for sid, size in ((5, 64), (6, 64), (7, 128)):
        assert ZC.payload(world.want["mixed"], sid)[165 * size:166 * size] == bytes(size)
    assert ZC.payload(world.want["mixed"], 8)[(165 - 3) * 64:(166 - 3) * 64] == bytes(64)
    assert ZC.payload(world.want["mixed"], 5)[164 * 64:165 * 64] == bytes(64)     # the cancelling wire
    assert ZC.payload(world.want["mixed"], 5)[163 * 64:164 * 64] != bytes(64)


@pytest.mark.parametrize("name", ALL)
def test_the_key_is_the_synthesisers_byte_for_byte(world, name, tmp_path):
    h = world.handles[name]
    before = _devices(world.K)
    for p in world.powers(name):
        got, rep = h.new_zkey(world.ptau[p])
        _same_key(world, name, got, rep)
        ptau_path, out = tmp_path / f"pot{p}.ptau", tmp_path / f"out{p}.zkey"
        ptau_path.write_bytes(world.ptau[p])
        none, rep = h.new_zkey(str(ptau_path), out=out)
        assert none is None and rep.write_ms > 0
        _same_key(world, name, out.read_bytes(), rep)
        assert sorted(os.listdir(tmp_path)) == sorted(f"{k}{q}.{e}" for q in world.powers(name) if q <= p for k, e in (("pot", "ptau"), ("out", "zkey")))
    assert _devices(world.K) == before
    assert world.K.zkey_new_size(world.S.write_r1cs(world.circuits[name])) == (len(world.want[name]), len(ZC.records(world.want[name])))


@pytest.mark.parametrize("name", ["fan", "mixed"])
def test_heavy_column_threshold_does_not_change_a_byte(world, name):
    h, ptau = world.handles[name], world.ptau[10]
    reps = {}
    for thr in (0, 8, 64, 1 << 30):
        got, reps[thr] = h.new_zkey(ptau, heavy_column_terms=thr)
        assert got[:12] == world.want[name][:12]
        _same_key(world, name, got, reps[thr])
    assert reps[8].heavy_columns > 0 and reps[8].heavy_items >= 2 * reps[8].heavy_columns
    assert (reps[1 << 30].heavy_columns, reps[1 << 30].heavy_items) == (0, 0)
    if name == "fan":                                                # columns of 300 and 301 terms: cut at 64 as well
        assert reps[64].heavy_columns > 0 and reps[64].heavy_items > reps[64].heavy_columns


@pytest.mark.parametrize("name", ALL)
def test_the_librarys_own_checks_accept_the_key(world, name):
    K, h = world.K, world.handles[name]
    p = world.powers(name)[-1]
    key, _ = h.new_zkey(world.ptau[p])
    ok, rep = K.zkey_check(key, seed=SEED)
    assert ok is True and rep.kind == 0
    ok, rep = h.match_zkey(key, seed=SEED)
    assert ok is True and rep.kind == 0
    for q in world.powers(name):
        ok, rep = h.verify_zkey(key, world.ptau[q], seed=SEED)
        assert ok is True and (rep.kind, rep.failed_mask) == (0, 0)


def test_the_key_loads_proves_and_verifies(world, S):
    K = world.K
    r, w = ZC.mixed(S)
    key, _ = world.handles["mixed"].new_zkey(world.ptau[8])
    vk = K.zkey_export_vk(key)
    cm = K.CacheManager()
    try:
        cm.load("new", key)
        pj, qj, _ = cm.prove_mem("new", S.write_wtns(w), 3, 5)
        assert json.loads(qj) == [str(v) for v in w[1:3]]
        assert K.groth16_verify_json(pj, qj, vk) is True
        bad = list(w)
        bad[40] = (bad[40] + 1) % ZC.R                               # CONSTRUCTED: one private wire off by one
        assert not ZC.check_r1cs(r, bad)
        pj, qj, _ = cm.prove_mem("new", S.write_wtns(bad), 3, 5)
        assert K.groth16_verify_json(pj, qj, vk) is False
    finally:
        cm.close()


def _without_sections(image, drop):
    secs, order = ZC.sections(image)
    keep = [s for s in order if s not in drop]
    return image[:8] + struct.pack("<I", len(keep)) + b"".join(struct.pack("<IQ", s, secs[s][1]) + image[secs[s][0]:secs[s][0] + secs[s][1]] for s in keep)


def _bump(image, offset):
    """the 32-byte little-endian coordinate at `offset`, plus one"""
    e = bytearray(image)
    e[offset:offset + 32] = ((int.from_bytes(e[offset:offset + 32], "little") + 1) % (1 << 256)).to_bytes(32, "little")
    return bytes(e)


def test_errors(world, S, tmp_path):
    K, h = world.K, world.handles["mixed"]
    before = _devices(K)
    ptau = world.ptau[10]
    secs = ZC.sections(ptau)[0]
    with pytest.raises(K.ProverError, match=r"\(-2\).*has not been prepared for phase 2"):
        h.new_zkey(_without_sections(ptau, {12, 13, 14, 15}))
    with pytest.raises(K.ProverError, match=r"\(-3\).*power 8 is below the key's domain 2\^9"):
        world.handles["fan"].new_zkey(world.ptau[8])
    low = S.write_ptau(7, world.fbm, points_to_mont=world.to_mont)
    with pytest.raises(K.ProverError, match=r"\(-3\).*power 7 is below the key's domain 2\^8"):
        h.new_zkey(low)
    # CONSTRUCTED: one coordinate of one point of each range that is read, plus one; domain 2^8, so block 8 and block 9 of 12
    for sid, block, elem, coord in ((12, 8, 0, 0), (13, 8, 255, 3), (14, 8, 7, 1), (15, 8, 128, 0), (12, 9, 511, 1)):
        size = 128 if sid == 13 else 64
        bad = _bump(ptau, secs[sid][0] + ((1 << block) - 1 + elem) * size + 32 * coord)
        with pytest.raises(K.ProverError, match=r"\(-2\).*section %d, block %d, element %d: the point is not on the curve" % (sid, block, elem)):
            h.new_zkey(bad)
        path, out = tmp_path / "bad.ptau", tmp_path / "never.zkey"
        path.write_bytes(bad)
        with pytest.raises(K.ProverError, match=r"\(-2\).*section %d, block %d, element %d" % (sid, block, elem)):
            h.new_zkey(path, out=out)
        assert sorted(os.listdir(tmp_path)) == ["bad.ptau"]          # neither the key nor a temporary
    # the same edit in blocks that are not read: block 7 and block 10 of section 12, block 9 of 14, and section 2
    for sid, block, elem in ((12, 7, 127), (12, 10, 0), (14, 9, 3), (13, 7, 5)):
        size = 128 if sid == 13 else 64
        got, _ = h.new_zkey(_bump(ptau, secs[sid][0] + ((1 << block) - 1 + elem) * size))
        assert got == h.new_zkey(ptau)[0]
        _same_key(world, "mixed", got)
    got, _ = h.new_zkey(_bump(ptau, secs[2][0] + 64 * 5))
    _same_key(world, "mixed", got)
    # cap one byte short: −3, and the report still says what is needed
    need = len(world.want["mixed"])
    opt, rep = K.ZkeyNewOptions(0), K.ZkeyNewReport()
    buf = C.create_string_buffer(need)
    rc = K.lib().groth16_zkey_new(h._h, C.c_char_p(ptau), C.c_size_t(len(ptau)), buf, C.c_size_t(need - 1), C.byref(opt), C.byref(rep))
    assert rc == -3 and rep.zkey_bytes == need and rep.n_coeffs == len(ZC.records(world.want["mixed"]))
    assert buf.raw == bytes(need)                                    # nothing was written
    rc = K.lib().groth16_zkey_new(h._h, C.c_char_p(ptau), C.c_size_t(len(ptau)), buf, C.c_size_t(need), C.byref(opt), C.byref(rep))
    assert rc == 0
    _same_key(world, "mixed", buf.raw, rep)
    with pytest.raises(K.ProverError, match=r"\(-1\).*cannot open"):
        h.new_zkey(tmp_path / "missing.ptau", out=tmp_path / "never.zkey")
    assert not (tmp_path / "never.zkey").exists()
    assert _devices(K) == before
    # the handle is as good as before
    assert h.match_zkey(world.want["mixed"], seed=SEED)[0] is True


def test_the_repl_writes_the_same_key(world, S, tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    (tmp_path / "c.r1cs").write_bytes(S.write_r1cs(world.circuits["chain7"]))
    (tmp_path / "pot.ptau").write_bytes(world.ptau[8])
    cmds = (f"zkey-new --r1cs {tmp_path}/c.r1cs --ptau {tmp_path}/pot.ptau --zkey {tmp_path}/out.zkey --device HIP\n"
            f"zkey-new --r1cs {tmp_path}/c.r1cs --ptau {tmp_path}/missing.ptau --zkey {tmp_path}/never.zkey\nnonsense\nexit\n")
    out = subprocess.run([os.path.join(root, "icicle-snark_amd", "lib", "prove")], input=cmds, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [ln.replace("> ", "") for ln in out.stdout.splitlines()]
    assert lines[0].startswith("wires 9 public 1 domain 16 coefficients 16 bytes %d longest column " % len(world.want["chain7"]))
    assert lines[1:4] == ["ZKEY_WRITTEN", "COMMAND_COMPLETED", "COMMAND_COMPLETED"] and "zkey-new failed (-1)" in out.stderr
    assert "zkey-new --r1cs <file> --ptau <file> --zkey <file> [--device HIP]" in out.stdout
    _same_key(world, "chain7", (tmp_path / "out.zkey").read_bytes())
    assert not (tmp_path / "never.zkey").exists()
