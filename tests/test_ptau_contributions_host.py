"""groth16_ptau_new and groth16_ptau_contributions — the ceremony's starting file and the host's audit of section 7 — against the
Python model of tests/ptau_contribute_model.py.  The files are the model's (write_unprepared over the oracle's generator
multiplication, section 7 from hashlib and Python integers), never the library's: chains of 0 to 3 records that must hold, at power
3 and at power 0, and CONSTRUCTED faults, each with the kind and index stated here and by the model.  Host only: neither call
initialises a GPU — this file runs, and passes, on a machine that has none."""
import ctypes as C
import struct

import pytest

import groth16_dlog_model as M
import ptau_contribute_model as CM
import ptau_prepare_model as PM

R, Q = CM.R, CM.Q
SECRETS = [bytes([i]) * 32 for i in (1, 2, 3)]
NAMES = [b"alice", b"", b"carol \xc3\xa9"]


class Chain:
    """files[i]: the unprepared file of `power` after i of the model's contributions, from toxic[0]; recs: the records"""

    def __init__(self, world, power, start=(1, 1, 1)):
        self.power, self.toxic, self.recs, self.trace = power, [start], [], []
        self.files = [world.raw(power, start)]
        for secret, name in zip(SECRETS, NAMES):
            primes, held = CM.secrets_of(secret), self.toxic[-1]
            d_before = held if self.recs else (1, 1, 1)
            before = self.recs[-1][:192] if self.recs else CM.generators(world.pb)[:192]
            rec, _, kcz = CM.make_record(CM.chain_hash(self.files[-1], self.recs, world.pb), before, d_before, held, primes, secret, name, world.pb)
            world.note(rec, d_before, held, primes, kcz)
            self.trace.append((d_before, held, primes, kcz))
            self.recs.append(rec)
            self.toxic.append(tuple(t * x % R for t, x in zip(held, primes)))
            self.files.append(PM.with_payload(world.raw(power, self.toxic[-1]), 7, CM.join_records(self.recs)))


class World:
    def __init__(self, K, O):
        self.K = K
        G = {g: O.ec_to_affine(g, O.ec_generator(g)) for g in ("g1", "g2")}
        self.fbm = lambda g, sc: O.fixed_base_mul(g, G[g], sc)
        self.to_mont = lambda a: O.fq_convert_montgomery(a, True)
        self.pb = CM.PointBytes(O)
        self.dlog = {self.pb.g1(1): 1, bytes(64): 0}
        self.g2log = {self.pb.g2(1): 1, bytes(128): 0}
        self._raw = {}
        self.c3, self.c0 = Chain(self, 3), Chain(self, 0)

    def raw(self, power, toxic):
        key = (power, toxic)
        if key not in self._raw:
            self._raw[key] = PM.write_unprepared(power, *toxic, self.fbm, self.to_mont)
        return self._raw[key]

    def note(self, rec, d_before, held, primes, kcz, g2_after=None):
        after = [t * x % R for t, x in zip(held, primes)]
        for x in range(3):
            self.dlog[rec[64 * x:64 * x + 64]] = after[x]
            self.dlog[rec[CM.R_TAU + 64 * x:CM.R_TAU + 64 * x + 64]] = kcz[x][0] * d_before[x] % R
        t2, b2 = g2_after or (after[0], after[2])
        self.g2log[rec[CM.TAU2:CM.TAU2 + 128]] = t2 % R
        self.g2log[rec[CM.BETA2:CM.BETA2 + 128]] = b2 % R

    def audit(self, image):
        ok, rep = self.K.ptau_contributions(image)
        return (ok, rep.count, rep.kind, rep.index), rep


@pytest.fixture(scope="module")
def world(K, O):
    return World(K, O)


# ---- groth16_ptau_new ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", [0, 1, 3])
def test_ptau_new_is_the_file_of_ones(world, power, tmp_path):
    K = world.K
    want = world.raw(power, (1, 1, 1))
    N = 1 << power
    assert K.ptau_new_size(power) == len(want) == 12 + 7 * 12 + 44 + (2 * N - 1) * 64 + N * 128 + 2 * N * 64 + 128 + 4
    assert K.ptau_new(power) == want
    assert K.ptau_new(power, out=tmp_path / "pot.ptau") is None and (tmp_path / "pot.ptau").read_bytes() == want
    assert [p.name for p in tmp_path.iterdir()] == ["pot.ptau"]
    # the library's own reader of an unprepared file takes it
    assert K.ptau_prepared_size(want) == PM.prepared_size(power, len(want))


def test_ptau_new_refuses_what_it_cannot_write(world, tmp_path):
    K = world.K
    assert K.ptau_new_size(27) == 12 + 7 * 12 + 44 + ((2 << 27) - 1) * 64 + (1 << 27) * 256 + 128 + 4
    for call in (lambda: K.ptau_new_size(28), lambda: K.ptau_new(28), lambda: K.ptau_new(28, out=tmp_path / "never.ptau"), lambda: K.ptau_new_size(1 << 31)):
        with pytest.raises(K.ProverError, match=r"\(-3\).*above 27"):
            call()
    assert list(tmp_path.iterdir()) == []
    # cap one byte short: −3, the size comes back, nothing is written
    need = K.ptau_new_size(3)
    buf, got = C.create_string_buffer(need), C.c_uint64(99)
    assert K.lib().groth16_ptau_new(C.c_uint32(3), buf, C.c_size_t(need - 1), C.byref(got)) == -3
    assert got.value == need and buf.raw == bytes(need)
    assert K.lib().groth16_ptau_new(C.c_uint32(3), None, C.c_size_t(0), C.byref(got)) == -3 and got.value == need
    with pytest.raises(K.ProverError, match=r"\(-1\).*cannot create"):
        K.ptau_new(1, out=tmp_path / "no_such_directory" / "pot.ptau")


# ---- groth16_ptau_contributions --------------------------------------------------------------------------------------------------
def test_the_model_is_three_schnorr_proofs_in_the_exponent(world):
    """z_x·d_x = k_x·d_x + c·(d_x·x′) for x ∈ {τ, α, β}: the equations the audit checks on points, on their logarithms"""
    for chain in (world.c3, world.c0):
        assert len(chain.trace) == 3
        for d_before, held, primes, kcz in chain.trace:
            assert len({c for _, c, _ in kcz}) == 1 and len({k for k, _, _ in kcz}) == 3 and len(set(primes)) == 3
            for d, t, x, (k, c, z) in zip(d_before, held, primes, kcz):
                assert 0 < x < R and 0 < k < R and 0 < c < 1 << 128 and z == (k + c * x) % R and d == t
                assert (z * d - k * d - c * (t * x % R)) % R == 0
        assert all(CM.h0(f) == CM.h0(chain.files[0]) for f in chain.files)
    assert CM.secrets_of(SECRETS[0])[1] == CM.W(SECRETS[0] + b"icicle-snark ptau contribution v1" + b"\2")
    assert CM.h0(world.c3.files[0]) != CM.h0(world.c0.files[0])            # section 1 holds the power


@pytest.mark.parametrize("power", [3, 0])
@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_a_chain_of_the_models_records_holds(world, power, n):
    chain = world.c3 if power == 3 else world.c0
    image = chain.files[n]
    assert CM.audit(image, power, world.dlog, world.g2log, world.pb) == (True, n, 0, 0)
    verdict, rep = world.audit(image)
    assert verdict == (True, n, 0, 0)
    assert rep.records == [(rec[0:64], rec[64:128], rec[128:192], rec[192:320], rec[320:448], name) for rec, name in zip(chain.recs[:n], NAMES)]


def _flip(b, byte, bit=0):
    e = bytearray(b)
    e[byte] ^= 1 << bit
    return bytes(e)


def _cases(w):
    """name → (image, power, the verdict stated here)"""
    c3, c0 = w.c3, w.c0
    f, recs = c3.files, c3.recs
    join = CM.join_records
    put = lambda image, p7: PM.with_payload(image, 7, p7)
    out = {}
    # SECTION
    out["the last record cut short"] = (put(f[3], join(recs)[:-10]), 3, (CM.SECTION, 3))
    out["count larger than the bytes hold"] = (put(f[3], struct.pack("<I", 1000) + join(recs)[4:]), 3, (CM.SECTION, 0))
    out["bytes behind the last record"] = (put(f[3], join(recs) + b"\0"), 3, (CM.SECTION, 3))
    out["name_len 256"] = (put(f[1], join([recs[0][:CM.NAME_LEN] + struct.pack("<I", 256) + bytes(256)])), 3, (CM.SECTION, 1))
    # POINT
    out["tau1 off the curve, record 1"] = (put(f[1], join([_flip(recs[0], CM.TAU1 + 32)])), 3, (CM.POINT, 1))
    twist = b"".join((c * CM.MONT % Q).to_bytes(32, "little") for c in M.twist_point_outside_subgroup())
    out["tau2 outside the subgroup, record 2"] = (put(f[3], join([recs[0], recs[1][:CM.TAU2] + twist + recs[1][CM.BETA2:], recs[2]])), 3, (CM.POINT, 2))
    out["alpha1 the identity, record 1"] = (put(f[1], join([recs[0][:CM.ALPHA1] + bytes(64) + recs[0][CM.BETA1:]])), 3, (CM.POINT, 1))
    out["beta2 the identity, record 3"] = (put(f[3], join([recs[0], recs[1], recs[2][:CM.BETA2] + bytes(128) + recs[2][CM.R_TAU:]])), 3, (CM.POINT, 3))
    big = recs[1][:CM.R_TAU + 128] + Q.to_bytes(32, "little") + recs[1][CM.R_TAU + 160:]
    out["a coordinate of R_beta not below q, record 2"] = (put(f[3], join([recs[0], big, recs[2]])), 3, (CM.POINT, 2))
    # POK
    out["z_beta not below r, record 1"] = (put(f[1], join([recs[0][:CM.Z_TAU + 64] + R.to_bytes(32, "little") + recs[0][CM.NAME_LEN:]])), 3, (CM.POK, 1))
    out["one bit of z_tau, record 1"] = (put(f[3], join([_flip(recs[0], CM.Z_TAU + 5, 2), recs[1], recs[2]])), 3, (CM.POK, 1))
    out["one bit of z_alpha, record 2"] = (put(f[3], join([recs[0], _flip(recs[1], CM.Z_TAU + 32 + 9), recs[2]])), 3, (CM.POK, 2))
    out["one bit of z_beta, record 3"] = (put(f[3], join([recs[0], recs[1], _flip(recs[2], CM.Z_TAU + 64 + 17, 6)])), 3, (CM.POK, 3))
    out["one bit of a name, record 1"] = (put(f[3], join([_flip(recs[0], CM.FIXED + 2), recs[1], recs[2]])), 3, (CM.POK, 1))
    out["records reordered"] = (put(f[2], join([recs[1], recs[0]])), 3, (CM.POK, 1))
    out["a record of another power's file"] = (put(f[1], join([c0.recs[0]])), 3, (CM.POK, 1))
    # a chain that did not start at the generators: record 1 over a file of (5, 7, 11), its `before` the generators all the same
    start = (5, 7, 11)
    primes = CM.secrets_of(SECRETS[0])
    rec, _, kcz = CM.make_record(CM.h0(f[0]), CM.generators(w.pb)[:192], (1, 1, 1), start, primes, SECRETS[0], NAMES[0], w.pb)
    w.note(rec, (1, 1, 1), start, primes, kcz)
    grown = w.raw(3, tuple(t * x % R for t, x in zip(start, primes)))
    assert PM.payload(grown, 4)[:64] == rec[CM.ALPHA1:CM.ALPHA1 + 64]     # the file is what the record ends in: only the proof fails
    out["a chain not starting at the generators"] = (put(grown, join([rec])), 3, (CM.POK, 1))
    # PAIR: a record whose G2 point has another logarithm, its three proofs intact
    tau_a, _, beta_a = c3.toxic[1]
    rec, _, kcz = CM.make_record(CM.h0(f[0]), CM.generators(w.pb)[:192], (1, 1, 1), (1, 1, 1), primes, SECRETS[0], NAMES[0], w.pb, g2_after=(tau_a + 1, beta_a))
    w.note(rec, (1, 1, 1), (1, 1, 1), primes, kcz, g2_after=(tau_a + 1, beta_a))
    out["tau2 is not tau1's, record 1"] = (put(f[1], join([rec])), 3, (CM.PAIR, 1))
    tau_b, _, beta_b = c3.toxic[2]
    p2 = CM.secrets_of(SECRETS[1])
    rec, _, kcz = CM.make_record(CM.chain_hash(f[1], recs[:1], w.pb), recs[0][:192], c3.toxic[1], c3.toxic[1], p2, SECRETS[1], NAMES[1], w.pb, g2_after=(tau_b, 2 * beta_b))
    w.note(rec, c3.toxic[1], c3.toxic[1], p2, kcz, g2_after=(tau_b, 2 * beta_b))
    out["beta2 is not beta1's, record 2"] = (put(f[2], join([recs[0], rec])), 3, (CM.PAIR, 2))
    # HEADER: the chain holds and ends in something the file does not hold
    for sid, what in ((4, "alpha1 is not section 4's"), (5, "beta1 is not section 5's"), (6, "beta2 is not section 6"), (2, "tau1 is not section 2's"), (3, "tau2 is not section 3's")):
        assert PM.payload(f[1], sid) != PM.payload(f[2], sid)
        out[what] = (PM.with_payload(f[2], sid, PM.payload(f[1], sid)), 3, (CM.HEADER, 0))
    out["the last record is an earlier one"] = (put(f[3], join(recs[:2])), 3, (CM.HEADER, 0))
    out["count 0, the file is not the generators'"] = (w.raw(3, (1, 1, 5)), 3, (CM.HEADER, 0))
    out["power 0: beta2 is not section 6"] = (PM.with_payload(c0.files[2], 6, PM.payload(c0.files[1], 6)), 0, (CM.HEADER, 0))
    return out


CASES = ["the last record cut short", "count larger than the bytes hold", "bytes behind the last record", "name_len 256", "tau1 off the curve, record 1",
         "tau2 outside the subgroup, record 2", "alpha1 the identity, record 1", "beta2 the identity, record 3", "a coordinate of R_beta not below q, record 2",
         "z_beta not below r, record 1", "one bit of z_tau, record 1", "one bit of z_alpha, record 2", "one bit of z_beta, record 3", "one bit of a name, record 1",
         "records reordered", "a record of another power's file", "a chain not starting at the generators", "tau2 is not tau1's, record 1", "beta2 is not beta1's, record 2",
         "alpha1 is not section 4's", "beta1 is not section 5's", "beta2 is not section 6", "tau1 is not section 2's", "tau2 is not section 3's",
         "the last record is an earlier one", "count 0, the file is not the generators'", "power 0: beta2 is not section 6"]


@pytest.fixture(scope="module")
def cases(world):
    c = _cases(world)
    assert sorted(c) == sorted(CASES)
    return c


@pytest.mark.parametrize("name", CASES)
def test_a_constructed_fault_gives_its_kind_and_index(world, cases, name):
    image, power, (kind, index) = cases[name]
    model = CM.audit(image, power, world.dlog, world.g2log, world.pb)
    assert (model[0], model[2], model[3]) == (False, kind, index), name
    verdict, rep = world.audit(image)
    assert verdict == model, name
    if kind != CM.SECTION:                                                  # the records whose bounds hold come back whatever the verdict
        assert len(rep.records) == rep.count


def test_power_0_holds_no_power_of_tau(world):
    """the power-0 rule: sections 2 and 3 hold one element each, τ⁰, so the last record's tau1 and tau2 are compared with nothing —
    the file of any τ is the file of τ = 1 — while alpha1, beta1 and beta2 still are"""
    c0 = world.c0
    assert PM.payload(c0.files[3], 2) == world.pb.g1(1) and PM.payload(c0.files[3], 3) == world.pb.g2(1)
    assert world.raw(0, (5, 1, 1)) == world.raw(0, (1, 1, 1)) and world.audit(world.raw(0, (5, 1, 1)))[0] == (True, 0, 0, 0)
    assert c0.recs[2][:64] != world.pb.g1(1)                                # the record's tau1 is a real point all the same
    assert world.audit(world.raw(0, (1, 7, 1)))[0] == (False, 0, CM.HEADER, 0)


def test_a_malformed_or_prepared_file_is_an_error_not_a_verdict(world):
    K = world.K
    image = world.c3.files[1]
    with pytest.raises(K.ProverError, match=r"\(-2\)"):
        K.ptau_contributions(image[:200])
    with pytest.raises(K.ProverError, match=r"\(-2\).*Missing section 7"):
        K.ptau_contributions(PM.without(image, {7}))
    prepared = image[:8] + struct.pack("<I", 8) + image[12:] + struct.pack("<IQ", 12, 0)
    with pytest.raises(K.ProverError, match=r"\(-2\).*section 12 is present: the file is already prepared"):
        K.ptau_contributions(prepared)
