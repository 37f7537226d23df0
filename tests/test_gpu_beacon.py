"""groth16_ptau_beacon and groth16_zkey_beacon on the GPU (needs an MI355X): the random beacon of both ceremony phases.  Expected
bytes never come from the library's kernels: sections 1 to 6 of a .ptau are tests/ptau_prepare_model.py's write_unprepared over the
PRODUCT of the secrets, sections 1 to 9 of a .zkey are the synthesiser's setup() over δ·δ′, and sections 7 and 10 are
tests/beacon_model.py's (hashlib and Python integers, points from the oracle).  The shapes are the contribute tests' own: powers 0,
1, 3 and 7, where the two-table split of the scale kernel has 1, 2, 4 and 16 high entries and section 2 of power 7 ends a lane short
of its fourth 64-lane workgroup; the circuits are tests/zkey_new_circuits.py's over a power-8 ptau."""
import ctypes as C
import hashlib
import json
import os

import pytest

import beacon_model as BM
import ptau_contribute_model as CM
import ptau_prepare_model as PM
import zkey_contribute_model as ZM
import zkey_new_circuits as ZC

pytestmark = pytest.mark.gpu

R = BM.R
SEED = bytes(range(32))
POWERS = [0, 1, 3, 7]
S1, S2 = bytes([0x11]) * 32, bytes([0x22]) * 32
P1 = (ZM.FULL, (R - 1) // 2, 12345)                                        # fixed (τ′, α′, β′) of the participant before the beacon
P2 = (3, R - 2, (1 << 127) + 9)                                            # … and of the one behind it
H1, H2 = hashlib.sha256(b"a block hash").digest(), bytes(range(200, 232))
OFF_CURVE = 2


class World:
    def __init__(self, K, O, S):
        self.K, self.S = K, S
        self.fbm = lambda g, sc: K.generator_mul(g, sc)
        self.to_mont = lambda a: O.fq_convert_montgomery(a, True)
        self.pb = CM.PointBytes(O)
        self.g1 = ZM.G1Bytes(O)
        self._one, self._zkey = {}, None

    def one(self, power):
        """new → one participant's contribution with fixed secrets: the file a beacon is applied to (its logarithms are P1)"""
        if power not in self._one:
            self._one[power] = self.K.ptau_contribute(self.K.ptau_new(power), secret=S1, name="alice", tau=P1[0], alpha=P1[1], beta=P1[2])[0]
        return self._one[power]

    def want_ptau(self, raw, power, toxic, name, **kw):
        return BM.expected_ptau(raw, power, toxic, name, self.fbm, self.to_mont, self.pb, **kw)

    def zkey(self):
        """the phase-2 side, made once: a power-8 ptau of known (τ, α, β), the circuits, their zkey-new keys after one contribution"""
        if self._zkey is None:
            K, S = self.K, self.S
            z = type("Zkey", (), {})()
            z.ptau = S.write_ptau(8, self.fbm, points_to_mont=self.to_mont)
            z.toxic = S.toxic_waste()[:3]
            z.circuits = {n: r for n, r in ZC.circuits(S).items() if n in ("mixed", "chain7", "tiny")}
            z.handles = {n: K.R1cs(S.write_r1cs(r)) for n, r in z.circuits.items()}
            z.d1 = ZM.delta_of(S1)
            z.k1 = {n: K.zkey_contribute(h.new_zkey(z.ptau)[0], secret=S1, name="a")[0] for n, h in z.handles.items()}
            self._zkey = z
        return self._zkey

    def setup(self, name, delta):
        z = self.zkey()
        return self.S.setup(z.circuits[name], self.fbm, points_to_mont=self.to_mont, toxic=z.toxic + (1, delta))[0]

    def close(self):
        if self._zkey is not None:
            for h in self._zkey.handles.values():
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


def _same(got, want):
    first = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    assert len(got) == len(want) and got == want, "first difference at byte %d of %d" % (first, len(want))


def _bump(image, offset):
    """the 32-byte little-endian coordinate at `offset`, plus one"""
    e = bytearray(image)
    e[offset:offset + 32] = ((int.from_bytes(e[offset:offset + 32], "little") + 1) % (1 << 256)).to_bytes(32, "little")
    return bytes(e)


def test_the_shapes_are_what_the_cases_need():
    """conditions, not measurements: the scale kernel runs 64-lane workgroups, a lane per point, over two tables"""
    assert [1 << (p + 1 - CM.table_bits(p)) for p in POWERS] == [1, 2, 4, 16]
    assert (2 << 7) - 1 == 3 * 64 + 63
    assert all(0 < x < R for x in CM.secrets_of(BM.digest(H1, 10)) + CM.secrets_of(BM.digest(H1, 0)))
    assert BM.digest(H1, 0) == hashlib.sha256(H1).digest() != BM.digest(H1, 10)


# ---- phase 1 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iter_exp", [0, 10])
@pytest.mark.parametrize("power", POWERS)
def test_ptau_beacon_is_the_models_in_every_byte(world, power, iter_exp, tmp_path):
    K = world.K
    before = _devices(K)
    i1 = world.one(power)
    got, rep = K.ptau_beacon(i1, H1, iter_exp, name="beacon")
    want, primes = world.want_ptau(i1, power, P1, b"beacon", beacon=(H1, iter_exp))
    _same(got, want)
    N = 1 << power
    assert (rep.contribution, rep.power, list(rep.points), rep.ptau_bytes) == (2, power, [2 * N - 1, N, N, N], len(got))
    assert len(got) == len(i1) + CM.FIXED + len(b"beacon") + 36 and rep.device_ms > 0 and (rep.fault_section, rep.fault_kind) == (0, 0)
    # the points are a contribution's of the public digest; only the record's tail, challenge and responses differ
    digest = K.beacon_digest(H1, iter_exp)
    assert digest == BM.digest(H1, iter_exp) and primes == CM.secrets_of(digest)
    via, _ = K.ptau_contribute(i1, secret=digest, name="beacon")
    cut = PM.sections(got)[0][7][0] - 12
    assert got[:cut] == via[:cut] and PM.sections(got)[1] == [1, 2, 3, 4, 5, 6, 7] and len(got) == len(via) + 36
    mine, theirs = BM.split_records(PM.payload(got, 7), "ptau")[1], BM.split_records(PM.payload(via, 7), "ptau")[1]
    assert mine[:CM.Z_TAU] == theirs[:CM.Z_TAU] and mine[CM.Z_TAU:CM.NAME_LEN] != theirs[CM.Z_TAU:CM.NAME_LEN]
    assert BM.beacon_of(mine, "ptau") == (H1, iter_exp) and BM.beacon_of(theirs, "ptau") is None
    # the audit, the beacon's parameters, the powers
    ok, crep = K.ptau_contributions(got)
    assert ok is True and (crep.count, crep.kind, crep.index) == (2, 0, 0) and crep.beacons == {2: (H1, iter_exp)}
    assert [r[5] for r in crep.records] == [b"alice", b"beacon"]
    ok, vrep = K.ptau_verify(got, seed=SEED)
    assert ok is True and (vrep.kind, vrep.failed_mask) == (0, 0)
    # the record of the digest's plain contribution is NOT a beacon's: nothing in that file says so
    ok, crep = K.ptau_contributions(via)
    assert ok is True and crep.beacons == {}
    if iter_exp == 0:                                                       # the file entry writes the same bytes and leaves nothing else
        src, out = tmp_path / "pot1.ptau", tmp_path / "pot2.ptau"
        src.write_bytes(i1)
        none, rep = K.ptau_beacon(src, H1, iter_exp, name=b"beacon", out=out)
        assert none is None and rep.write_ms > 0 and rep.ptau_bytes == len(want)
        _same(out.read_bytes(), want)
        assert sorted(os.listdir(tmp_path)) == ["pot1.ptau", "pot2.ptau"]
    assert _devices(K) == before


def test_a_beacon_on_a_fresh_file_and_a_contribution_behind_it(world):
    """[beacon] over ptau_new's file, then a participant: contribute appends behind a beacon record, and the audit walks both"""
    K = world.K
    i0 = K.ptau_new(3)
    b1, rep = K.ptau_beacon(i0, H2, 3)
    want, primes = world.want_ptau(i0, 3, (1, 1, 1), b"", beacon=(H2, 3))
    _same(b1, want)
    assert rep.contribution == 1 and K.ptau_contributions(b1)[1].beacons == {1: (H2, 3)}
    c2, rep = K.ptau_contribute(b1, secret=S2, name="late", tau=P2[0], alpha=P2[1], beta=P2[2])
    _same(c2, world.want_ptau(b1, 3, primes, b"late", secret=S2, primes=P2)[0])
    ok, crep = K.ptau_contributions(c2)
    assert ok is True and (crep.count, crep.kind, crep.index) == (2, 0, 0) and crep.beacons == {1: (H2, 3)} and rep.contribution == 2
    b3, _ = K.ptau_beacon(c2, H1, 0, name="second beacon")
    ok, crep = K.ptau_contributions(b3)
    assert ok is True and crep.count == 3 and crep.beacons == {1: (H2, 3), 3: (H1, 0)} and K.ptau_verify(b3, seed=SEED)[0] is True


def test_ptau_refusals(world, tmp_path):
    K = world.K
    before = _devices(K)
    i1 = world.one(3)
    beaconed, _ = K.ptau_beacon(i1, H1, 10, name="beacon")
    need = len(beaconed)

    def call(image, iter_exp=10, cap=None):
        rep, buf = K.PtauContributeReport(), C.create_string_buffer(need)
        rc = K.lib().groth16_ptau_beacon(C.c_char_p(image), C.c_size_t(len(image)), (C.c_uint8 * 32).from_buffer_copy(H1), C.c_uint32(iter_exp), b"beacon", buf,
                                         C.c_size_t(need if cap is None else cap), b"HIP", C.byref(rep))
        return rc, rep, buf.raw

    assert call(i1)[2] == beaconed
    # a truncated file (P = 3 → p = 1) audits as the full file does, and takes no beacon: apply it to the full file, then truncate
    cut, _ = K.ptau_truncate(beaconed, 1)
    ok, crep = K.ptau_contributions(cut)
    full = K.ptau_contributions(beaconed)[1]
    assert ok is True and (crep.count, crep.kind, crep.index) == (2, 0, 0) and crep.beacons == full.beacons == {2: (H1, 10)} and crep.records[1][5] == b"beacon"
    with pytest.raises(K.ProverError, match=r"\(-2\).*the file is a truncation"):
        K.ptau_beacon(cut, H2, 0)
    rc, rep, written = call(K.ptau_truncate(i1, 1)[0])
    assert rc == -2 and written == bytes(need)
    # CONSTRUCTED: one coordinate plus one in section 4 — −2, the report names it, nothing is written, the file entry leaves nothing
    off = {sid: o for sid, (o, _) in PM.sections(i1)[0].items()}
    bad = _bump(i1, off[4] + 5 * 64)
    rc, rep, written = call(bad)
    assert rc == -2 and (rep.fault_section, rep.fault_index, rep.fault_kind) == (4, 5, OFF_CURVE) and written == bytes(need)
    path, out = tmp_path / "bad.ptau", tmp_path / "never.ptau"
    path.write_bytes(bad)
    with pytest.raises(K.ProverError, match=r"\(-2\).*section 4, element 5: the point is not on the curve"):
        K.ptau_beacon(path, H1, 10, out=out)
    assert sorted(os.listdir(tmp_path)) == ["bad.ptau"]
    # a prepared file, a stale chain
    with pytest.raises(K.ProverError, match=r"\(-2\).*already prepared"):
        K.ptau_beacon(K.ptau_prepare(i1)[0], H1, 0)
    with pytest.raises(K.ProverError, match=r"\(-2\).*last record is not what sections 2 to 6 hold"):
        K.ptau_beacon(PM.with_payload(beaconed, 7, PM.payload(i1, 7)), H1, 0)
    # iter_exp = 25: −3 before any work — no size is reported, nothing is written
    rc, rep, written = call(i1, iter_exp=25)
    assert rc == -3 and rep.ptau_bytes == 0 and written == bytes(need)
    with pytest.raises(K.ProverError, match=r"\(-3\).*iter_exp 25 is above 24"):
        K.ptau_beacon(i1, H1, 25)
    # cap one byte short: −3, the report says what is needed, nothing is written; a name too long
    rc, rep, written = call(i1, cap=need - 1)
    assert rc == -3 and rep.ptau_bytes == need and written == bytes(need)
    with pytest.raises(K.ProverError, match=r"\(-3\).*name has 256 bytes"):
        K.ptau_beacon(i1, H1, 0, name="n" * 256)
    assert _devices(K) == before and call(i1)[2] == beaconed                # a following good call is as good as before


# ---- phase 2 -----------------------------------------------------------------------------------------------------------------------
COPIED = [1, 2, 3, 5, 6, 7, 8, 9]          # compared as bytes; section 4 as records (zkey-new's stated order is not setup()'s)


@pytest.mark.parametrize("name, iter_exp", [("mixed", 10), ("chain7", 0), ("tiny", 0)])
def test_zkey_beacon_is_the_synthesisers_and_the_models(world, name, iter_exp, tmp_path):
    K = world.K
    z = world.zkey()
    before = _devices(K)
    k1 = z.k1[name]
    got, rep = K.zkey_beacon(k1, H2, iter_exp, name="beacon")
    p10, delta = BM.expected_section10(k1, z.d1, b"beacon", world.g1, beacon=(H2, iter_exp))
    digest = K.beacon_digest(H2, iter_exp)
    assert digest == BM.digest(H2, iter_exp) and delta == ZM.delta_of(digest)
    # sections 1 to 9: contributing δ′ to the key of δ must give the synthesiser's key of δ·δ′
    want = world.setup(name, z.d1 * delta % R)
    assert ZC.sections(got)[1] == list(range(1, 11)) and got[:8] == want[:8]
    for sid in COPIED:
        assert ZC.payload(got, sid) == ZC.payload(want, sid), (name, sid)
    assert sorted(ZC.records(got)) == sorted(ZC.records(want)) and ZC.payload(got, 4) == ZC.payload(k1, 4)
    assert ZC.payload(got, 10) == p10
    n8, n9 = (len(ZC.payload(k1, s)) // 64 for s in (8, 9))
    assert (rep.contribution, rep.points_c, rep.points_h, rep.zkey_bytes, rep.faults) == (2, n8, n9, len(got), 0)
    assert len(got) == len(k1) + ZM.FIXED + len(b"beacon") + 36
    # … which is what the plain contribution of the digest writes there
    via, _ = K.zkey_contribute(k1, secret=digest, name="beacon")
    assert all(ZC.payload(got, s) == ZC.payload(via, s) for s in range(1, 10)) and len(got) == len(via) + 36
    ok, crep = K.zkey_contributions(got)
    assert ok is True and (crep.count, crep.kind, crep.index) == (2, 0, 0) and crep.beacons == {2: (H2, iter_exp)} and [n for _, n in crep.records] == [b"a", b"beacon"]
    assert K.zkey_contributions(via)[1].beacons == {}
    ok, vrep = z.handles[name].verify_zkey(got, z.ptau, seed=SEED)
    assert ok is True and (vrep.kind, vrep.failed_mask) == (0, 0)
    if name == "chain7":                                                    # the file entry; a contribution behind the beacon
        src, out = tmp_path / "k1.zkey", tmp_path / "k2.zkey"
        src.write_bytes(k1)
        none, rep = K.zkey_beacon(src, H2, iter_exp, name="beacon", out=out)
        assert none is None and out.read_bytes() == got and rep.write_ms > 0 and sorted(os.listdir(tmp_path)) == ["k1.zkey", "k2.zkey"]
        k3, _ = K.zkey_contribute(got, secret=S2, name="late")
        assert ZC.payload(k3, 10) == BM.expected_section10(got, z.d1 * delta % R, b"late", world.g1, secret=S2)[0]
        ok, crep = K.zkey_contributions(k3)
        assert ok is True and crep.count == 3 and crep.beacons == {2: (H2, iter_exp)}
    assert _devices(K) == before


def test_zkey_refusals(world, tmp_path):
    K = world.K
    z = world.zkey()
    k1 = z.k1["mixed"]
    need = len(k1) + ZM.FIXED + 36

    def call(key, iter_exp=0, cap=None):
        rep, buf = K.ZkeyContributeReport(), C.create_string_buffer(need)
        rc = K.lib().groth16_zkey_beacon(C.c_char_p(key), C.c_size_t(len(key)), (C.c_uint8 * 32).from_buffer_copy(H2), C.c_uint32(iter_exp), b"", buf,
                                         C.c_size_t(need if cap is None else cap), b"HIP", C.byref(rep))
        return rc, rep, buf.raw

    good = K.zkey_beacon(k1, H2, 0)[0]
    assert call(k1)[2] == good
    bad = _bump(k1, ZC.sections(k1)[0][8][0] + 64 * 100)
    rc, rep, written = call(bad)
    assert rc == -2 and (rep.fault_section, rep.fault_index, rep.fault_kind, rep.faults) == (8, 100, K.ZKEY_OFF_CURVE, 1)
    path, out = tmp_path / "bad.zkey", tmp_path / "never.zkey"
    path.write_bytes(bad)
    with pytest.raises(K.ProverError, match=r"\(-2\).*section 8, element 100"):
        K.zkey_beacon(path, H2, 0, out=out)
    assert sorted(os.listdir(tmp_path)) == ["bad.zkey"]
    rc, rep, written = call(k1, iter_exp=25)
    assert rc == -3 and rep.zkey_bytes == 0 and written == bytes(need)
    with pytest.raises(K.ProverError, match=r"\(-3\).*iter_exp 25 is above 24"):
        K.zkey_beacon(k1, H2, 25)
    rc, rep, written = call(k1, cap=need - 1)
    assert rc == -3 and rep.zkey_bytes == need and written == bytes(need)
    with pytest.raises(K.ProverError, match=r"\(-2\).*last record is not the header's delta1"):
        K.zkey_beacon(ZM.with_section(good, 10, ZC.payload(k1, 10)), H2, 0)
    assert call(k1)[2] == good


# ---- both phases, secrets nobody knows ---------------------------------------------------------------------------------------------
def test_the_ceremony_from_nothing_to_a_verified_proof_with_both_beacons(world):
    """ptau_new(4) → contribute → beacon → contributions → ptau_verify → prepare → new_zkey(chain7, domain 16) → zkey_contribute →
    zkey_beacon → zkey_contributions → verify_zkey → prove → verify.  The participants' secrets are the operating system's: nobody in
    this test knows τ or δ, although everybody knows the beacons' shares."""
    K, S = world.K, world.S
    r, w = S.squaring_chain(7)
    h = K.R1cs(S.write_r1cs(r))
    try:
        pot, _ = K.ptau_contribute(K.ptau_new(4), name="first")
        pot, rep = K.ptau_beacon(pot, H1, 10, name="phase 1 beacon")
        assert rep.contribution == 2
        ok, crep = K.ptau_contributions(pot)
        assert ok is True and crep.count == 2 and crep.beacons == {2: (H1, 10)} and [rec[5] for rec in crep.records] == [b"first", b"phase 1 beacon"]
        assert PM.payload(pot, 2)[64:128] == crep.records[1][0] != CM.generators(world.pb)[:64]
        assert K.ptau_verify(pot, seed=SEED)[0] is True
        ptau = K.ptau_prepare(pot)[0]
        key = h.new_zkey(ptau)[0]
        key, _ = K.zkey_contribute(key, name="phase 2")
        key, rep = K.zkey_beacon(key, H2, 10, name="phase 2 beacon")
        assert rep.contribution == 2
        ok, crep = K.zkey_contributions(key)
        assert ok is True and crep.count == 2 and crep.beacons == {2: (H2, 10)} and crep.records[1][0] == ZC.payload(key, 2)[468:532]
        ok, vrep = h.verify_zkey(key, ptau, seed=SEED)
        assert ok is True and (vrep.kind, vrep.failed_mask) == (0, 0)
        vk = K.zkey_export_vk(key)
        cm = K.CacheManager()
        try:
            cm.load("beaconed", key)
            pj, qj, _ = cm.prove_mem("beaconed", S.write_wtns(w), 3, 5)
            assert json.loads(qj) == [str(v) for v in w[1:1 + r.n_public]]
            assert K.groth16_verify_json(pj, qj, vk) is True
            bad = list(w)
            bad[3] = (bad[3] + 1) % R                                       # CONSTRUCTED: one wire off by one
            assert not ZC.check_r1cs(r, bad)
            pj, qj, _ = cm.prove_mem("beaconed", S.write_wtns(bad), 3, 5)
            assert K.groth16_verify_json(pj, qj, vk) is False
        finally:
            cm.close()
    finally:
        h.close()
