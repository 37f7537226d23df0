"""groth16_ptau_prepare on the GPU (needs an MI355X): sections 12 to 15 of a powers-of-tau file made from its sections 2 to 5.
Expected bytes never come from the library's transform: they are the Python model's (tests/ptau_prepare_model.py — a direct
O(n²) inverse transform of the discrete logarithms) turned into points by the generator multiplication, as the other key-tool
tests do.  The shapes are the smallest at which the kernels can still go wrong: power 0 and 1 (blocks smaller than a wave, one
butterfly, the zero-extended blocks of 2 and 4 points), power 3, and power 7 (the top G1 block has 256 points: 128 butterflies, two
workgroups, the other blocks partly filled ones)."""
import ctypes as C
import json
import os
import subprocess

import pytest

import groth16_dlog_model as M
import ptau_prepare_model as PM
import zkey_new_circuits as ZC

pytestmark = pytest.mark.gpu

R, Q = PM.R, PM.Q
SEED = bytes(range(32))
POWERS = [0, 1, 3, 7]
OFF_CURVE, OFF_SUBGROUP, NONCANONICAL = 2, 3, 1


class World:
    def __init__(self, K, O, S):
        self.K, self.S = K, S
        self.fbm = lambda g, sc: K.generator_mul(g, sc)
        self.to_mont = lambda a: O.fq_convert_montgomery(a, True)
        self.toxic = S.toxic_waste()[:3]
        self._raw, self._got = {}, {}

    def raw(self, power, toxic=None):
        key = (power, toxic or self.toxic)
        if key not in self._raw:
            self._raw[key] = PM.write_unprepared(power, *key[1], self.fbm, self.to_mont)
        return self._raw[key]

    def want(self, power, toxic=None):
        return PM.expected_prepared(self.raw(power, toxic), power, *(toxic or self.toxic), self.fbm, self.to_mont)

    def got(self, power, toxic=None):
        key = (power, toxic or self.toxic)
        if key not in self._got:
            self._got[key] = self.K.ptau_prepare(self.raw(power, toxic))
        return self._got[key]


@pytest.fixture(scope="module")
def world(gpu, O, S):
    return World(gpu, O, S)


def _devices(K):
    dev = K.Device()
    K.check(K.lib().icicle_get_active_device(C.byref(dev)), "get_active_device")
    hip = C.c_int(-1)
    C.CDLL("libamdhip64.so").hipGetDevice(C.byref(hip))
    return dev.type, dev.id, hip.value


def _first_difference(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


@pytest.mark.parametrize("power", POWERS)
def test_every_byte_is_the_models(world, power):
    K, S = world.K, world.S
    before = _devices(K)
    raw = world.raw(power)
    got, rep = world.got(power)
    want = world.want(power)
    assert len(got) == len(want) == K.ptau_prepared_size(raw) == rep.ptau_bytes
    assert got == want, "first difference at byte %d of %d" % (_first_difference(got, want), len(want))
    N = 1 << power
    assert (rep.power, list(rep.points)) == (power, [4 * N - 1, 2 * N - 1, 2 * N - 1, 2 * N - 1])
    assert rep.device_ms > 0 and rep.download_ms > 0 and (rep.fault_section, rep.fault_kind) == (0, 0)
    # sections 1 to 7 byte for byte, 12 to 15 behind them in this order
    assert PM.sections(got)[1] == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15] and got[12:len(raw)] == raw[12:]
    # the synthesiser's prepared file, which knows τ, everywhere outside section 12's last block
    full = S.write_ptau(power, world.fbm, points_to_mont=world.to_mont)
    cut = PM.sections(full)[0][12][0] + (2 * N - 1) * 64
    assert len(full) == len(got) and got[:cut] == full[:cut] and got[cut + 2 * N * 64:] == full[cut + 2 * N * 64:]
    assert got[cut:cut + 2 * N * 64] != full[cut:cut + 2 * N * 64]
    # the library's own reader takes it
    assert K.ptau_info(got, domain_power=power).power == power
    assert _devices(K) == before


def test_the_shapes_are_what_the_cases_need():
    """conditions, not measurements: the kernels run 64-lane workgroups, one lane per butterfly (or per input in the load)"""
    assert 0 in POWERS and 1 in POWERS                      # blocks of 1, 2 and 4 points: no butterfly, one, two
    assert (1 << 7) // 2 == 64 and (2 << 7) // 2 == 128     # power 7: a full workgroup, and two (section 12's last block)
    assert all((1 << p) // 2 < 64 for p in range(7))        # every smaller block alone: less than a workgroup
    assert (1 << 7) - 1 > 64 and ((1 << 7) - 1) % 64        # the blocks below the top one side by side: two workgroups, the last not full
    assert (2 << 7) // 2 // 2 == 64                         # level 1 of the 256-point block has two twiddles: 64 butterflies share each


DEGENERATE = {"one": 1, "minus_one": R - 1, "omega3": PM.omega(3)}


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_ceremonies(world, name):
    """τ inside a domain: equal inputs (level 0 doubles and cancels), identities that travel through the later levels"""
    tau = DEGENERATE[name]
    toxic = (tau,) + world.toxic[1:]
    sc = PM.prepared_scalars(3, *toxic)
    zeros = {sid: [i for i, x in enumerate(xs) if x == 0] for sid, xs in sc.items()}
    # conditions on the inputs: where the model has the identity, and that it has points elsewhere
    if name == "one":         # τ^i = 1: every block p ≤ 3 is e₀; the zero-extended block 4 has no zero at all
        assert all(sc[13][(1 << p) - 1] != 0 and not any(sc[13][1 << p:(2 << p) - 1]) for p in range(4))
        assert all(sc[12][15:]) and len(zeros[12]) == len(zeros[13]) == 1 + 3 + 7
    elif name == "minus_one":  # τ = ω₁: block p ≥ 1 is the unit vector at j = 2^(p−1); block 4 (15 of 16 inputs) has no zero
        assert all([j for j in range(1 << p) if sc[13][(1 << p) - 1 + j]] == [1 << (p - 1)] for p in range(1, 4))
        assert all(sc[12][15:])
    else:                      # τ = ω₃: blocks 0 … 2 are dense, block 3 is e₁: a single point in the top block of 13, 14, 15
        assert [j for j in range(8) if sc[13][7 + j]] == [1] and all(sc[13][:7]) and all(sc[12][15:])
    got, _ = world.got(3, toxic)
    want = world.want(3, toxic)
    assert got == want, "first difference at byte %d" % _first_difference(got, want)
    for sid in (12, 13, 14, 15):
        size = PM.ELEM[sid]
        body = PM.payload(got, sid)
        assert [i for i in range(len(body) // size) if body[i * size:(i + 1) * size] == bytes(size)] == zeros[sid]
    assert sum(len(z) for z in zeros.values()) > 0


def _bump(image, offset):
    """the 32-byte little-endian coordinate at `offset`, plus one"""
    e = bytearray(image)
    e[offset:offset + 32] = ((int.from_bytes(e[offset:offset + 32], "little") + 1) % (1 << 256)).to_bytes(32, "little")
    return bytes(e)


def test_faults(world, tmp_path):
    K = world.K
    before = _devices(K)
    raw = world.raw(3)
    off = {sid: o for sid, (o, _) in PM.sections(raw)[0].items()}

    def refused(bad, text, section=None, element=None, kind=None):
        with pytest.raises(K.ProverError, match=r"\(-2\)") as e:
            K.ptau_prepare(bad)
        assert text in str(e.value), str(e.value)
        if section is not None:
            rep, got = K.PtauPrepareReport(), C.c_uint64(99)
            buf = C.create_string_buffer(K.ptau_prepared_size(raw))
            rc = K.lib().groth16_ptau_prepare(C.c_char_p(bad), C.c_size_t(len(bad)), buf, C.c_size_t(len(buf)), C.byref(got), b"HIP", C.byref(rep))
            assert rc == -2 and got.value == 0 and (rep.fault_section, rep.fault_index, rep.fault_kind) == (section, element, kind)

    # CONSTRUCTED: one coordinate plus one — section 2's last element (the one only the last block reads), and section 4
    refused(_bump(raw, off[2] + 14 * 64 + 32), "section 2, element 14: the point is not on the curve", 2, 14, OFF_CURVE)
    refused(_bump(raw, off[4] + 5 * 64), "section 4, element 5: the point is not on the curve", 4, 5, OFF_CURVE)
    refused(_bump(raw, off[5] + 0 * 64), "section 5, element 0: the point is not on the curve", 5, 0, OFF_CURVE)
    # a point on the twist outside the subgroup in section 3, and as section 6
    tw = b"".join((c * (1 << 256) % Q).to_bytes(32, "little") for c in M.twist_point_outside_subgroup())
    e = bytearray(raw)
    e[off[3] + 6 * 128:off[3] + 7 * 128] = tw
    refused(bytes(e), "section 3, element 6: the point is outside the subgroup", 3, 6, OFF_SUBGROUP)
    e = bytearray(raw)
    e[off[6]:off[6] + 128] = tw
    refused(bytes(e), "section 6, element 0: the point is outside the subgroup", 6, 0, OFF_SUBGROUP)
    # a coordinate that is not below q
    e = bytearray(raw)
    e[off[2] + 3 * 64:off[2] + 3 * 64 + 32] = Q.to_bytes(32, "little")
    refused(bytes(e), "section 2, element 3: a coordinate is not below q", 2, 3, NONCANONICAL)
    # the lowest faulty element is the one named
    refused(_bump(_bump(raw, off[2] + 9 * 64), off[2] + 2 * 64), "section 2, element 2: ", 2, 2, OFF_CURVE)
    # an already prepared input, a short section 2
    refused(world.got(3)[0], "section 12 is present: the file is already prepared for phase 2")
    refused(PM.with_payload(raw, 2, PM.payload(raw, 2)[:-64]), "section 2 holds 896 bytes, an unprepared file of power 3 has 960")
    # the file entry leaves neither the file nor a temporary behind
    path, out = tmp_path / "bad.ptau", tmp_path / "never.ptau"
    path.write_bytes(_bump(raw, off[4] + 5 * 64))
    with pytest.raises(K.ProverError, match=r"\(-2\).*section 4, element 5"):
        K.ptau_prepare(path, out=out)
    assert sorted(os.listdir(tmp_path)) == ["bad.ptau"]
    with pytest.raises(K.ProverError, match=r"\(-1\).*cannot open"):
        K.ptau_prepare(tmp_path / "missing.ptau", out=out)
    with pytest.raises(K.ProverError, match=r"\(-3\).*the output path is the input's"):
        K.ptau_prepare(path, out=path)
    assert sorted(os.listdir(tmp_path)) == ["bad.ptau"]
    # cap one byte short: −3, the report says what is needed, nothing is written
    need = K.ptau_prepared_size(raw)
    rep, got = K.PtauPrepareReport(), C.c_uint64(99)
    buf = C.create_string_buffer(need)
    rc = K.lib().groth16_ptau_prepare(C.c_char_p(raw), C.c_size_t(len(raw)), buf, C.c_size_t(need - 1), C.byref(got), b"HIP", C.byref(rep))
    assert rc == -3 and rep.ptau_bytes == need and got.value == 0 and buf.raw == bytes(need)
    with pytest.raises(K.ProverError, match=r"\(-3\).*does not name one HIP device"):
        K.ptau_prepare(raw, device="HIP:0-1")
    assert _devices(K) == before
    assert K.ptau_prepare(raw)[0] == world.got(3)[0]                          # a following good call is as good as before


def test_file_entry_and_repl(world, tmp_path):
    K = world.K
    raw, want = world.raw(3), world.got(3)[0]
    src, out = tmp_path / "pot.ptau", tmp_path / "pot_final.ptau"
    src.write_bytes(raw)
    none, rep = K.ptau_prepare(str(src), out=out)
    assert none is None and out.read_bytes() == want and rep.write_ms > 0 and rep.ptau_bytes == len(want)
    assert sorted(os.listdir(tmp_path)) == ["pot.ptau", "pot_final.ptau"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmds = (f"ptau-prepare --ptau {src} --out {tmp_path}/repl.ptau --device HIP\n"
            f"ptau-prepare --ptau {tmp_path}/repl.ptau --out {tmp_path}/never.ptau\nnonsense\nexit\n")
    run = subprocess.run([os.path.join(root, "icicle-snark_amd", "lib", "prove")], input=cmds, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lines = [ln.replace("> ", "") for ln in run.stdout.splitlines()]
    assert lines[0].startswith("power 3 points 31 15 15 15 bytes %d; upload " % len(want)) and lines[1:3] == ["PTAU_WRITTEN", "COMMAND_COMPLETED"]
    assert lines[3] == "COMMAND_COMPLETED" and "ptau-prepare failed (-2)" in run.stderr and "already prepared" in run.stderr
    assert "ptau-prepare --ptau <file> --out <file> [--device HIP]" in run.stdout
    assert (tmp_path / "repl.ptau").read_bytes() == want and not (tmp_path / "never.ptau").exists()


def test_chain_new_zkey_over_the_prepared_file(world):
    """`mixed` has the domain 2^8.  Over a power-9 file the key reads blocks 8 and 9, none of them section 12's last: the key is the
    key over the synthesiser's file, byte for byte.  Over a power-8 file H comes from section 12's LAST block, which prepare defines
    as the transform of the zero-extended vector: every section but 9 is the same, and section 9 is the model's truncated basis."""
    K, S = world.K, world.S
    r = ZC.circuits(S)["mixed"]
    h = K.R1cs(S.write_r1cs(r))
    try:
        assert S.key_scalars(r, world.toxic + (1, 1))["n"] == 256
        got9 = K.ptau_prepare(world.raw(9))[0]
        full9 = S.write_ptau(9, world.fbm, points_to_mont=world.to_mont)
        assert got9 != full9
        assert h.new_zkey(got9)[0] == h.new_zkey(full9)[0]
        got8 = K.ptau_prepare(world.raw(8))[0]
        k_got, k_full = h.new_zkey(got8)[0], h.new_zkey(S.write_ptau(8, world.fbm, points_to_mont=world.to_mont))[0]
        assert ZC.sections(k_got)[1] == ZC.sections(k_full)[1]
        for sid in ZC.sections(k_got)[1]:
            assert (ZC.payload(k_got, sid) == ZC.payload(k_full, sid)) == (sid != 9), sid
        tau = world.toxic[0]
        src = PM.source_scalars(8, tau, 1, 1)[2]
        assert len(src) == 511
        trunc = PM.inverse_transform(src, 9)
        assert ZC.payload(k_got, 9) == PM._points("g1", trunc[1::2], world.fbm, world.to_mont)
        ok, rep = h.verify_zkey(k_got, got8, seed=SEED)
        assert ok is True and (rep.kind, rep.failed_mask) == (0, 0)
    finally:
        h.close()


def test_chain_a_domain_equal_to_the_power_proves(world):
    """chain7 (domain 16) over a prepared power-4 file: H is built from the zero-extended block.  The key verifies against that
    file, takes a contribution, proves, and the proof verifies."""
    K, S = world.K, world.S
    r, w = S.squaring_chain(7)
    h = K.R1cs(S.write_r1cs(r))
    try:
        assert S.key_scalars(r, world.toxic + (1, 1))["n"] == 16
        ptau = K.ptau_prepare(world.raw(4))[0]
        assert ptau == world.want(4)
        key = h.new_zkey(ptau)[0]
        ok, rep = h.verify_zkey(key, ptau, seed=SEED)
        assert ok is True and (rep.kind, rep.failed_mask) == (0, 0)
        trunc = PM.inverse_transform(PM.source_scalars(4, world.toxic[0], 1, 1)[2], 5)
        full = S.lagrange_at(32, 5, world.toxic[0])
        assert len(trunc) == 32 and all(a != b for a, b in zip(trunc, full))
        assert ZC.payload(key, 9) == PM._points("g1", trunc[1::2], world.fbm, world.to_mont)
        key1, _ = K.zkey_contribute(key, secret=bytes([0x51]) * 32, name="a")
        ok, rep = h.verify_zkey(key1, ptau, seed=SEED)
        assert ok is True and K.zkey_contributions(key1)[0] is True
        vk = K.zkey_export_vk(key1)
        cm = K.CacheManager()
        try:
            cm.load("prepared", key1)
            pj, qj, _ = cm.prove_mem("prepared", S.write_wtns(w), 3, 5)
            assert json.loads(qj) == [str(v) for v in w[1:1 + r.n_public]]
            assert K.groth16_verify_json(pj, qj, vk) is True
            bad = list(w)
            bad[3] = (bad[3] + 1) % R                                       # CONSTRUCTED: one wire off by one
            assert not ZC.check_r1cs(r, bad)
            pj, qj, _ = cm.prove_mem("prepared", S.write_wtns(bad), 3, 5)
            assert K.groth16_verify_json(pj, qj, vk) is False
        finally:
            cm.close()
    finally:
        h.close()
