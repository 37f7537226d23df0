"""groth16_ptau_contribute on the GPU (needs an MI355X): one participant's secrets applied to every point of an unprepared
powers-of-tau file.  Expected bytes never come from the library's kernels: sections 1 to 6 are tests/ptau_prepare_model.py's
write_unprepared over the PRODUCT of the secrets, turned into points by the generator multiplication as the other key-tool tests
do, and section 7 is tests/ptau_contribute_model.py's (hashlib and Python integers, points from the oracle).  The shapes are the
smallest at which the kernels can still go wrong: power 0 (one point per section, section 2's only scalar is 1), power 1 (3 and 2
points), power 3 (both table levels), power 7 (section 2 has 255 points: four 64-lane workgroups, the last a lane short; the other
sections fill two; the hi table has more than one entry)."""
import ctypes as C
import json
import os
import subprocess

import pytest

import groth16_dlog_model as M
import ptau_contribute_model as CM
import ptau_prepare_model as PM
import zkey_contribute_model as ZM
import zkey_new_circuits as ZC

pytestmark = pytest.mark.gpu

R, Q = PM.R, PM.Q
SEED = bytes(range(32))
POWERS = [0, 1, 3, 7]
OFF_CURVE, OFF_SUBGROUP, NONCANONICAL = 2, 3, 1
S1, S2 = bytes([0x11]) * 32, bytes([0x22]) * 32
P1 = (ZM.FULL, (R - 1) // 2, 12345)                                        # fixed (τ′, α′, β′) of the first participant
P2 = (3, R - 2, (1 << 127) + 9)                                            # … and of the second
OMEGA3 = PM.omega(3)


class World:
    def __init__(self, K, O, S):
        self.K, self.S = K, S
        self.fbm = lambda g, sc: K.generator_mul(g, sc)
        self.to_mont = lambda a: O.fq_convert_montgomery(a, True)
        self.pb = CM.PointBytes(O)
        self.toxic = S.toxic_waste()[:3]
        self._raw, self._two = {}, {}

    def raw(self, power, toxic=None):
        key = (power, toxic or self.toxic)
        if key not in self._raw:
            self._raw[key] = PM.write_unprepared(power, *key[1], self.fbm, self.to_mont)
        return self._raw[key]

    def want(self, raw, power, toxic, primes, secret, name):
        return CM.expected_contributed(raw, power, toxic, primes, secret, name, self.fbm, self.to_mont, self.pb)

    def two(self, power):
        """new → contribute → contribute with the fixed secrets: (image 0, image 1, image 2, report 1, report 2), made once"""
        if power not in self._two:
            K = self.K
            i0 = K.ptau_new(power)
            i1, r1 = K.ptau_contribute(i0, secret=S1, name="alice", tau=P1[0], alpha=P1[1], beta=P1[2])
            i2, r2 = K.ptau_contribute(i1, secret=S2, name=b"bob \xc3\xa9", tau=P2[0], alpha=P2[1], beta=P2[2])
            self._two[power] = (i0, i1, i2, r1, r2)
        return self._two[power]


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


def _same(got, want):
    assert len(got) == len(want) and got == want, "first difference at byte %d of %d" % (_first_difference(got, want), len(want))


def test_the_shapes_are_what_the_cases_need():
    """conditions, not measurements: the scale kernel runs 64-lane workgroups, one lane per point"""
    assert (2 << 7) - 1 == 255 and 255 // 64 == 3 and 255 % 64 == 63       # power 7, section 2: four workgroups, the last a lane short
    assert (1 << 7) == 2 * 64                                              # … the other sections fill two
    assert [CM.table_bits(p) for p in POWERS] == [1, 1, 2, 4]
    assert [1 << (p + 1 - CM.table_bits(p)) for p in POWERS] == [1, 2, 4, 16]   # entries of a hi table: more than one from power 1 on
    assert all(0 < x < R for x in P1 + P2) and ZM.FULL.bit_length() >= 253


@pytest.mark.parametrize("power", POWERS)
def test_two_contributions_are_the_models_in_every_byte(world, power, tmp_path):
    K = world.K
    before = _devices(K)
    i0, i1, i2, r1, r2 = world.two(power)
    one = (1, 1, 1)
    assert i0 == world.raw(power, one)
    w1 = world.want(i0, power, one, P1, S1, b"alice")
    _same(i1, w1)
    w2 = world.want(w1, power, P1, P2, S2, b"bob \xc3\xa9")
    _same(i2, w2)
    # sections 1 to 6 are the file of the products, and nobody told the library the products
    prod = tuple(a * b % R for a, b in zip(P1, P2))
    full = world.raw(power, prod)
    cut = PM.sections(full)[0][7][0] - 12
    assert i2[:cut] == full[:cut] and PM.sections(i2)[1] == [1, 2, 3, 4, 5, 6, 7]
    N = 1 << power
    for n, (rep, image, name) in enumerate(((r1, i1, b"alice"), (r2, i2, b"bob \xc3\xa9")), 1):
        assert (rep.contribution, rep.power, list(rep.points), rep.ptau_bytes) == (n, power, [2 * N - 1, N, N, N], len(image))
        assert rep.device_ms > 0 and rep.download_ms > 0 and rep.upload_ms > 0 and (rep.fault_section, rep.fault_kind) == (0, 0)
        assert len(image) == len(i0) + n * CM.FIXED + len(b"alice") + (len(name) if n == 2 else 0)
    # the file entry writes the same bytes and leaves nothing else
    src, out = tmp_path / "pot0.ptau", tmp_path / "pot1.ptau"
    src.write_bytes(i0)
    none, rep = K.ptau_contribute(src, secret=S1, name="alice", out=out, tau=P1[0], alpha=P1[1], beta=P1[2])
    assert none is None and rep.write_ms > 0 and rep.ptau_bytes == len(w1)
    _same(out.read_bytes(), w1)
    assert sorted(os.listdir(tmp_path)) == ["pot0.ptau", "pot1.ptau"]
    # the audit
    ok, rep = K.ptau_contributions(i2)
    assert ok is True and (rep.count, rep.kind, rep.index) == (2, 0, 0) and [r[5] for r in rep.records] == [b"alice", b"bob \xc3\xa9"]
    assert rep.records[1][:5] == tuple(w2[-(CM.FIXED + 6):][o:o + n] for o, n in ((0, 64), (64, 64), (128, 64), (192, 128), (320, 128)))
    # the library's own reader of an unprepared file takes it
    assert K.ptau_prepared_size(i2) == PM.prepared_size(power, len(i2))
    assert _devices(K) == before


def test_the_secrets_come_from_the_participants_bytes(world):
    """without fixed values: (τ′, α′, β′) = W(secret ‖ TAG ‖ label), and another secret gives another file"""
    K = world.K
    i0 = K.ptau_new(1)
    got, _ = K.ptau_contribute(i0, secret=S1, name="w")
    _same(got, world.want(i0, 1, (1, 1, 1), CM.secrets_of(S1), S1, b"w"))
    assert len(set(CM.secrets_of(S1))) == 3 and CM.secrets_of(S1) != CM.secrets_of(S2)
    other, _ = K.ptau_contribute(i0, secret=S2, name="w")
    drawn, _ = K.ptau_contribute(i0, name="w")                             # the operating system's: nobody knows it
    assert len({got, other, drawn}) == 3 and K.ptau_contributions(drawn)[0] is True


def test_a_file_that_did_not_start_at_the_generators(world):
    """τ, α, β ≠ 1 in the input, no record: every point is scaled all the same; the record's `before` is the generators, so the
    audit refuses the chain at record 1"""
    K = world.K
    raw = world.raw(3)
    assert all(t not in (0, 1) for t in world.toxic)
    got, rep = K.ptau_contribute(raw, secret=S1, name="late", tau=P1[0], alpha=P1[1], beta=P1[2])
    _same(got, world.want(raw, 3, world.toxic, P1, S1, b"late"))
    assert rep.contribution == 1
    ok, rep = K.ptau_contributions(got)
    assert ok is False and (rep.count, rep.kind, rep.index) == (1, CM.POK, 1)


EDGE_TAUS = {"one": 1, "minus_one": R - 1, "omega3": OMEGA3, "longest_form": 3 << 252, "full_width": ZM.FULL}


@pytest.mark.parametrize("name", list(EDGE_TAUS))
def test_edge_secrets_through_the_kernel(world, name):
    """τ′ = 1: every lane of sections 2 and 3 has s = 1; r − 1: s alternates 1 and −1; ω₃: the powers cycle with period 8, so lanes
    0 and 8 share a scalar; 3·2²⁵²: the longest signed-digit form; α′ = r − 1: section 4 is the negated section 2 prefix"""
    K = world.K
    tau = EDGE_TAUS[name]
    primes = (tau, R - 1, (R + 1) // 2)
    assert pow(OMEGA3, 8, R) == 1 and len(ZM.naf(3 << 252)) == 255
    raw = world.raw(3)
    got, _ = K.ptau_contribute(raw, secret=S2, name=name, tau=primes[0], alpha=primes[1], beta=primes[2])
    _same(got, world.want(raw, 3, world.toxic, primes, S2, name.encode()))


def test_the_secrets_one_change_nothing(world):
    K = world.K
    raw = world.raw(3)
    got, _ = K.ptau_contribute(raw, secret=S2, name="", tau=1, alpha=1, beta=1)
    cut = PM.sections(raw)[0][7][0] - 12
    assert got[:cut] == raw[:cut] and len(got) == len(raw) + CM.FIXED
    _same(got, world.want(raw, 3, world.toxic, (1, 1, 1), S2, b""))


def _bump(image, offset):
    """the 32-byte little-endian coordinate at `offset`, plus one"""
    e = bytearray(image)
    e[offset:offset + 32] = ((int.from_bytes(e[offset:offset + 32], "little") + 1) % (1 << 256)).to_bytes(32, "little")
    return bytes(e)


def test_faults(world, tmp_path):
    K = world.K
    before = _devices(K)
    i0, i1, i2, _, _ = world.two(3)
    off = {sid: o for sid, (o, _) in PM.sections(i1)[0].items()}
    need = len(i1) + CM.FIXED

    def call(image, cap=None, name=b"", opt=None):
        rep, buf = K.PtauContributeReport(), C.create_string_buffer(need)
        rc = K.lib().groth16_ptau_contribute(C.c_char_p(image), C.c_size_t(len(image)), (C.c_uint8 * 32).from_buffer_copy(S1), name, buf,
                                             C.c_size_t(need if cap is None else cap), b"HIP", opt, C.byref(rep))
        return rc, rep, buf.raw

    def refused(bad, text, section=None, element=None, kind=None):
        with pytest.raises(K.ProverError, match=r"\(-2\)") as e:
            K.ptau_contribute(bad, secret=S1)
        assert text in str(e.value), str(e.value)
        rc, rep, written = call(bad)
        assert rc == -2 and written == bytes(need)                           # nothing is written
        if section is not None:
            assert (rep.fault_section, rep.fault_index, rep.fault_kind) == (section, element, kind)

    # CONSTRUCTED: one coordinate plus one in section 4; a point of the twist outside the subgroup in section 3 and as section 6
    refused(_bump(i1, off[4] + 5 * 64), "ptau: section 4, element 5: the point is not on the curve", 4, 5, OFF_CURVE)
    tw = b"".join((c * (1 << 256) % Q).to_bytes(32, "little") for c in M.twist_point_outside_subgroup())
    e = bytearray(i1)
    e[off[3] + 6 * 128:off[3] + 7 * 128] = tw
    refused(bytes(e), "ptau: section 3, element 6: the point is outside the subgroup", 3, 6, OFF_SUBGROUP)
    e = bytearray(i0)                                                      # (a file without a record: section 6 is compared with nothing first)
    e[off[6]:off[6] + 128] = tw
    refused(bytes(e), "ptau: section 6, element 0: the point is outside the subgroup", 6, 0, OFF_SUBGROUP)
    e = bytearray(i1)
    e[off[6]:off[6] + 128] = tw
    refused(bytes(e), "section 7's last record is not what sections 2 to 6 hold")
    # section 2's last element, the one lane of its last workgroup's end; a coordinate that is not below q; the lowest element is named
    refused(_bump(i1, off[2] + 14 * 64 + 32), "ptau: section 2, element 14: the point is not on the curve", 2, 14, OFF_CURVE)
    e = bytearray(i1)
    e[off[5] + 3 * 64:off[5] + 3 * 64 + 32] = Q.to_bytes(32, "little")
    refused(bytes(e), "ptau: section 5, element 3: a coordinate is not below q", 5, 3, NONCANONICAL)
    refused(_bump(_bump(i1, off[2] + 9 * 64), off[2] + 2 * 64), "ptau: section 2, element 2: ", 2, 2, OFF_CURVE)
    # a faulty point in a later section is found although an earlier section is sound: every verdict is in before any scaling
    refused(_bump(_bump(i1, off[5] + 7 * 64), off[4] + 64), "ptau: section 4, element 1: ", 4, 1, OFF_CURVE)
    # a prepared input: contribute first, prepare last
    refused(K.ptau_prepare(i1)[0], "section 12 is present: the file is already prepared for phase 2")
    # section 7: stale (the records of an earlier file), malformed
    refused(PM.with_payload(i2, 7, PM.payload(i1, 7)), "section 7's last record is not what sections 2 to 6 hold")
    refused(PM.with_payload(i1, 7, PM.payload(i2, 7)), "section 7's last record is not what sections 2 to 6 hold")
    refused(PM.with_payload(i1, 7, PM.payload(i1, 7)[:-3]), "section 7 is malformed at record 1 of 1")
    refused(PM.with_payload(i1, 7, b"\7\0\0\0" + PM.payload(i1, 7)[4:]), "section 7 is malformed at record 0 of 0")
    # the file entry leaves neither the file nor a temporary behind
    path, out = tmp_path / "bad.ptau", tmp_path / "never.ptau"
    path.write_bytes(_bump(i1, off[4] + 5 * 64))
    with pytest.raises(K.ProverError, match=r"\(-2\).*section 4, element 5"):
        K.ptau_contribute(path, secret=S1, out=out)
    assert sorted(os.listdir(tmp_path)) == ["bad.ptau"]
    with pytest.raises(K.ProverError, match=r"\(-1\).*cannot open"):
        K.ptau_contribute(tmp_path / "missing.ptau", out=out)
    # equal paths, by name and by inode
    with pytest.raises(K.ProverError, match=r"\(-3\).*the output path is the input's"):
        K.ptau_contribute(path, out=path)
    os.link(path, tmp_path / "alias.ptau")
    with pytest.raises(K.ProverError, match=r"\(-3\).*the output path is the input's"):
        K.ptau_contribute(path, out=tmp_path / "alias.ptau")
    assert sorted(os.listdir(tmp_path)) == ["alias.ptau", "bad.ptau"] and path.read_bytes() == _bump(i1, off[4] + 5 * 64)
    # cap one byte short: −3, the report says what is needed, nothing is written
    rc, rep, written = call(i1, cap=need - 1)
    assert rc == -3 and rep.ptau_bytes == need and written == bytes(need)
    # arguments
    with pytest.raises(K.ProverError, match=r"\(-3\).*does not name one HIP device"):
        K.ptau_contribute(i1, device="HIP:0-1")
    with pytest.raises(K.ProverError, match=r"\(-3\).*name has 256 bytes"):
        K.ptau_contribute(i1, name="n" * 256)
    for kw, text in (({"tau": 0}, "fixed_tau"), ({"alpha": R}, "fixed_alpha"), ({"beta": R + 5}, "fixed_beta")):
        with pytest.raises(K.ProverError, match=r"\(-3\).*%s is not in \[1, r\)" % text):
            K.ptau_contribute(i1, **kw)
    assert _devices(K) == before
    assert K.ptau_contribute(i1, secret=S2, name=b"bob \xc3\xa9", tau=P2[0], alpha=P2[1], beta=P2[2])[0] == i2   # a following good call is as good as before


def test_the_chain_from_nothing_to_a_verified_proof(world):
    """ptau_new(4) → contribute ×2 → ptau_contributions → ptau_prepare → new_zkey(chain7, domain 16) → zkey_contribute → verify_zkey +
    zkey_contributions → prove → verify.  The secrets are the operating system's: nobody in this test knows τ."""
    K, S = world.K, world.S
    r, w = S.squaring_chain(7)
    h = K.R1cs(S.write_r1cs(r))
    try:
        pot = K.ptau_new(4)
        for name in ("first", "second"):
            pot, rep = K.ptau_contribute(pot, name=name)
        assert rep.contribution == 2
        ok, rep = K.ptau_contributions(pot)
        assert ok is True and rep.count == 2 and [rec[5] for rec in rep.records] == [b"first", b"second"]
        assert PM.payload(pot, 2)[64:128] == rep.records[1][0] != CM.generators(world.pb)[:64]
        ptau = K.ptau_prepare(pot)[0]
        key = h.new_zkey(ptau)[0]
        ok, rep = h.verify_zkey(key, ptau, seed=SEED)
        assert ok is True and (rep.kind, rep.failed_mask) == (0, 0)
        key1, _ = K.zkey_contribute(key, name="phase 2")
        ok, rep = h.verify_zkey(key1, ptau, seed=SEED)
        assert ok is True and K.zkey_contributions(key1)[0] is True
        vk = K.zkey_export_vk(key1)
        cm = K.CacheManager()
        try:
            cm.load("ceremony", key1)
            pj, qj, _ = cm.prove_mem("ceremony", S.write_wtns(w), 3, 5)
            assert json.loads(qj) == [str(v) for v in w[1:1 + r.n_public]]
            assert K.groth16_verify_json(pj, qj, vk) is True
            bad = list(w)
            bad[3] = (bad[3] + 1) % R                                       # CONSTRUCTED: one wire off by one
            assert not ZC.check_r1cs(r, bad)
            pj, qj, _ = cm.prove_mem("ceremony", S.write_wtns(bad), 3, 5)
            assert K.groth16_verify_json(pj, qj, vk) is False
        finally:
            cm.close()
    finally:
        h.close()


def test_repl(world, tmp_path):
    K = world.K
    t = tmp_path
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    (t / "stale.ptau").write_bytes(PM.with_payload(world.two(3)[2], 7, PM.payload(world.two(3)[1], 7)))
    cmds = (f"ptau-new --power 3 --out {t}/p0.ptau\n"
            f"ptau-contribute --ptau {t}/p0.ptau --out {t}/p1.ptau --name ann --device HIP\n"
            f"ptau-contribute --ptau {t}/p1.ptau --out {t}/p2.ptau\n"
            f"ptau-contributions --ptau {t}/p2.ptau\n"
            f"ptau-contributions --ptau {t}/stale.ptau\n"
            f"ptau-contribute --ptau {t}/stale.ptau --out {t}/never.ptau\n"
            f"ptau-new --power 28 --out {t}/never.ptau\nnonsense\nexit\n")
    run = subprocess.run([os.path.join(root, "icicle-snark_amd", "lib", "prove")], input=cmds, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lines = [ln.replace("> ", "") for ln in run.stdout.splitlines()]
    assert lines[0:2] == ["PTAU_WRITTEN", "COMMAND_COMPLETED"]
    size = K.ptau_new_size(3)
    assert lines[2].startswith("contribution 1 power 3 points 15 8 8 8 bytes %d; upload " % (size + CM.FIXED + 3)) and lines[3:5] == ["PTAU_WRITTEN", "COMMAND_COMPLETED"]
    assert lines[5].startswith("contribution 2 power 3 points 15 8 8 8 bytes %d; upload " % (size + 2 * CM.FIXED + 3)) and lines[6:8] == ["PTAU_WRITTEN", "COMMAND_COMPLETED"]
    assert lines[8].startswith('contribution 1 name "ann" tau1 ') and lines[9].startswith('contribution 2 name "" tau1 ') and lines[10:12] == ["CHAIN_OK", "COMMAND_COMPLETED"]
    assert lines[12].startswith('contribution 1 name "alice" tau1 ') and lines[13:15] == ["CHAIN_BAD HEADER 0", "COMMAND_COMPLETED"]
    assert lines[15] == "COMMAND_COMPLETED" and "ptau-contribute failed (-2)" in run.stderr and "last record is not what sections 2 to 6 hold" in run.stderr
    assert lines[16] == "COMMAND_COMPLETED" and "ptau-new failed (-3)" in run.stderr
    for usage in ("ptau-new --power <P> --out <file>", "ptau-contribute --ptau <file> --out <file> [--name <text>] [--device HIP]", "ptau-contributions --ptau <file>"):
        assert usage in run.stdout
    assert (t / "p0.ptau").read_bytes() == K.ptau_new(3) and not (t / "never.ptau").exists()
    assert sorted(os.listdir(t)) == ["p0.ptau", "p1.ptau", "p2.ptau", "stale.ptau"]
    ok, rep = K.ptau_contributions((t / "p2.ptau").read_bytes())
    assert ok is True and rep.count == 2
