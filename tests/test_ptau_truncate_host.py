"""The host half of groth16_ptau_truncate: an UNPREPARED file cut down to a lower power, the size function, the refusals, and what
groth16_ptau_contributions says about a truncated file, against tests/ptau_truncate_model.py.  Expected bytes are the model's own file
of the lower power — tests/ptau_prepare_model.py's write_unprepared over the oracle's generator multiplication — with ceremonyPower
and section 7 patched; the records are tests/ptau_contribute_model.py's.  Nothing here opens a GPU: every call names device "HIP:99",
which no machine has, and this file runs, and passes, on a machine without one.  Parameters, never measurements."""
import ctypes as C
import os
import struct

import pytest

import point_pack_model as PK
import ptau_contribute_model as CM
import ptau_prepare_model as PM
import ptau_truncate_model as TM

R = PM.R
TOXIC = (0x1234567, 0x89abcde, 0xf012345)
NOWHERE = "HIP:99"
SECRETS = [bytes([i]) * 32 for i in (1, 2)]
NAMES = [b"alice", b"bob \xc3\xa9"]
PAIRS = [(P, p) for P in (1, 3, 7) for p in sorted({0, 1, P - 1, P})]


class World:
    def __init__(self, K, O):
        self.K = K
        G = {g: O.ec_to_affine(g, O.ec_generator(g)) for g in ("g1", "g2")}
        self.fbm = lambda g, sc: O.fixed_base_mul(g, G[g], sc)
        self.to_mont = lambda a: O.fq_convert_montgomery(a, True)
        self.pb = CM.PointBytes(O)
        self._raw = {}
        self.dlog = {self.pb.g1(1): 1, bytes(64): 0}
        self.g2log = {self.pb.g2(1): 1, bytes(128): 0}

    def raw(self, power, toxic=TOXIC):
        if (power, toxic) not in self._raw:
            self._raw[power, toxic] = PM.write_unprepared(power, *toxic, self.fbm, self.to_mont)
        return self._raw[power, toxic]

    def chain(self, power):
        """the model's ceremony of two contributions from (1, 1, 1): the file, its records, the final logarithms"""
        toxic, recs = (1, 1, 1), []
        image = self.raw(power, toxic)
        for secret, name in zip(SECRETS, NAMES):
            primes = CM.secrets_of(secret)
            d_before = toxic if recs else (1, 1, 1)
            before = recs[-1][:192] if recs else CM.generators(self.pb)[:192]
            rec, _, kcz = CM.make_record(CM.chain_hash(image, recs, self.pb), before, d_before, toxic, primes, secret, name, self.pb)
            after = [t * x % R for t, x in zip(toxic, primes)]
            for x in range(3):
                self.dlog[rec[64 * x:64 * x + 64]] = after[x]
                self.dlog[rec[CM.R_TAU + 64 * x:CM.R_TAU + 64 * x + 64]] = kcz[x][0] * d_before[x] % R
            self.g2log[rec[CM.TAU2:CM.TAU2 + 128]] = after[0]
            self.g2log[rec[CM.BETA2:CM.BETA2 + 128]] = after[2]
            recs.append(rec)
            toxic = tuple(after)
            image = PM.with_payload(self.raw(power, toxic), 7, CM.join_records(recs))
        return image, recs, toxic


@pytest.fixture(scope="module")
def world(K, O):
    return World(K, O)


def _same(got, want):
    first = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    assert len(got) == len(want) and got == want, "first difference at byte %d of %d" % (first, len(want))


def test_the_models_two_statements_agree(world):
    """the model's file of the lower power, patched, IS the slices of the larger one: conditions on the model, before the library"""
    for P, p in PAIRS:
        full = world.raw(P)
        want = TM.expected(full, p, TOXIC, world.fbm, world.to_mont, False)
        assert want == TM.cut_unprepared(full, p) and len(want) == TM.truncated_size(full, p)
        assert TM.powers(want) == (p, P) and PM.sections(want)[1] == [1, 2, 3, 4, 5, 6, 7]
        n = 1 << p
        assert [len(PM.payload(want, s)) for s in (2, 3, 4, 5, 6)] == [(2 * n - 1) * 64, n * 128, n * 64, n * 64, 128]
    assert (1 + TM.CUBE_ROOT + TM.CUBE_ROOT ** 2) % R == 0 and TM.CUBE_ROOT != 1


@pytest.mark.parametrize("P,p", PAIRS)
def test_unprepared_truncation_is_the_models_file(world, P, p, tmp_path):
    K = world.K
    full = world.raw(P)
    want = TM.expected(full, p, TOXIC, world.fbm, world.to_mont, False)
    assert K.ptau_truncated_size(full, p) == len(want)
    got, rep = K.ptau_truncate(full, p, device=NOWHERE)
    _same(got, want)
    assert (rep.power_in, rep.power_out, rep.prepared, rep.points_fixed, rep.in_bytes, rep.out_bytes) == (P, p, 0, 0, len(full), len(want))
    assert (rep.fault_section, rep.fault_kind, rep.fault_count, rep.upload_ms, rep.device_ms, rep.download_ms) == (0, 0, 0, 0, 0, 0)
    (tmp_path / "in.ptau").write_bytes(full)
    none, rep = K.ptau_truncate(tmp_path / "in.ptau", p, out=tmp_path / "out.ptau", device=NOWHERE)
    assert none is None and rep.out_bytes == len(want) and (rep.power_in, rep.power_out) == (P, p)
    _same((tmp_path / "out.ptau").read_bytes(), want)
    assert sorted(os.listdir(tmp_path)) == ["in.ptau", "out.ptau"]
    if p == P:
        assert got == full
    else:
        # the library's own reader of an unprepared file takes it, and a second cut is the cut
        assert K.ptau_prepared_size(got) == PM.prepared_size(p, len(got))
        if p:
            _same(K.ptau_truncate(got, 0, device=NOWHERE)[0], TM.expected(full, 0, TOXIC, world.fbm, world.to_mont, False))


def _with_unknown_sections(image):
    """an unknown section behind section 3 and another at the end"""
    secs, order = PM.sections(image)
    sec = lambda s, p: struct.pack("<IQ", s, len(p)) + p
    parts = []
    for s in order:
        parts.append(sec(s, image[secs[s][0]:secs[s][0] + secs[s][1]]))
        if s == 3:
            parts.append(sec(99, b"in the middle" * 5))
    parts.append(sec(9, bytes(range(77))))
    return image[:8] + struct.pack("<I", len(order) + 2) + b"".join(parts)


def test_unknown_sections_survive_in_place(world):
    K = world.K
    image = _with_unknown_sections(world.raw(3))
    want = TM.cut_unprepared(image, 1)
    assert PM.sections(want)[1] == [1, 2, 3, 99, 4, 5, 6, 7, 9]
    got, _ = K.ptau_truncate(image, 1, device=NOWHERE)
    _same(got, want)
    assert PM.payload(got, 99) == b"in the middle" * 5 and PM.payload(got, 9) == bytes(range(77))
    assert K.ptau_truncated_size(image, 1) == len(want) == TM.truncated_size(image, 1)


def test_refusals(world, tmp_path):
    K = world.K
    full = world.raw(3)
    # a power above the file's: −3 from both entries and from the size function
    for call in (lambda: K.ptau_truncate(full, 4, device=NOWHERE), lambda: K.ptau_truncated_size(full, 4), lambda: K.ptau_truncated_size(full, 1 << 31)):
        with pytest.raises(K.ProverError, match=r"\(-3\).*above the file's 3"):
            call()
    rep = K.PtauTruncateReport()
    assert K.lib().groth16_ptau_truncate(C.c_char_p(full), C.c_size_t(len(full)), C.c_uint32(4), None, C.c_size_t(0), NOWHERE.encode(), C.byref(rep)) == -3
    # cap one byte short: −3, the report says what is needed, nothing is written
    need = TM.truncated_size(full, 1)
    rep, buf = K.PtauTruncateReport(), C.create_string_buffer(need)
    rc = K.lib().groth16_ptau_truncate(C.c_char_p(full), C.c_size_t(len(full)), C.c_uint32(1), buf, C.c_size_t(need - 1), NOWHERE.encode(), C.byref(rep))
    assert rc == -3 and rep.out_bytes == need and buf.raw == bytes(need)
    # equal paths, by name and by inode; a missing input
    path = tmp_path / "in.ptau"
    path.write_bytes(full)
    with pytest.raises(K.ProverError, match=r"\(-3\).*the output path is the input's"):
        K.ptau_truncate(path, 1, out=path, device=NOWHERE)
    os.link(path, tmp_path / "alias.ptau")
    with pytest.raises(K.ProverError, match=r"\(-3\).*the output path is the input's"):
        K.ptau_truncate(path, 1, out=tmp_path / "alias.ptau", device=NOWHERE)
    with pytest.raises(K.ProverError, match=r"\(-1\).*cannot open"):
        K.ptau_truncate(tmp_path / "missing.ptau", 1, out=tmp_path / "never.ptau", device=NOWHERE)
    # a packed file: −2 with the reader's text; a malformed section table; a section of another power's size
    for call in (lambda x: K.ptau_truncate(x, 1, device=NOWHERE), lambda x: K.ptau_truncated_size(x, 1)):
        for bad, text in ((PK.pack_file(full), "Invalid File format (expected 'ptau')"), (full[:20], "truncated section table"), (full[:-3], "section 7 exceeds the file"),
                          (PM.without(full, {5}), "Missing section 5"), (PM.with_payload(full, 4, PM.payload(full, 4)[:-64]), "ptau: section 4 holds 448 bytes, a file of power 3 has 512")):
            with pytest.raises(K.ProverError, match=r"\(-2\)") as e:
                call(bad)
            assert text in str(e.value), str(e.value)
    path.write_bytes(PK.pack_file(full))
    with pytest.raises(K.ProverError, match=r"\(-2\).*Invalid File format \(expected 'ptau'\)"):
        K.ptau_truncate(path, 1, out=tmp_path / "never.ptau", device=NOWHERE)
    assert sorted(os.listdir(tmp_path)) == ["alias.ptau", "in.ptau"]
    # a device string that names no ONE device is an argument error, also where no device would be opened
    with pytest.raises(K.ProverError, match=r"\(-3\).*does not name one HIP device"):
        K.ptau_truncate(full, 1, device="HIP:0-1")


# ---- the audit of a truncated file -----------------------------------------------------------------------------------------------
def _verdict(K, image):
    ok, rep = K.ptau_contributions(image)
    return (ok, rep.count, rep.kind, rep.index), rep


def test_the_chain_of_a_truncated_file_holds(world):
    K = world.K
    full, recs, toxic = world.chain(3)
    assert CM.audit(full, 3, world.dlog, world.g2log, world.pb) == (True, 2, 0, 0) and TM.h0(full) == CM.h0(full)
    full_verdict, full_rep = _verdict(K, full)
    assert full_verdict == (True, 2, 0, 0)                                    # a full file's verdict is what it was
    for p in (0, 1, 2):
        want = TM.expected(full, p, toxic, world.fbm, world.to_mont, False)
        got, _ = K.ptau_truncate(full, p, device=NOWHERE)
        _same(got, want)
        assert TM.h0(got) == CM.h0(full) != CM.h0(got)                      # the rule: the full file's start, not the bytes' own
        assert TM.audit(got, world.dlog, world.g2log, world.pb) == (True, 2, 0, 0)
        verdict, rep = _verdict(K, got)
        assert verdict == (True, 2, 0, 0) and rep.records == full_rep.records
        # ceremonyPower altered: another h₀, and the first proof no longer holds — upwards, and down to the file's own power
        for c in (4, p):
            bad = PM.with_payload(got, 1, TM.header(p, c))
            assert TM.audit(bad, world.dlog, world.g2log, world.pb) == (False, 2, CM.POK, 1)
            assert _verdict(K, bad)[0] == (False, 2, CM.POK, 1)
    # power ≥ ceremonyPower hashes its own bytes, as before: a full file with a LOWER ceremonyPower is not the chain's file
    odd = PM.with_payload(full, 1, TM.header(3, 2))
    assert TM.h0(odd) == CM.h0(odd) != CM.h0(full)
    assert _verdict(K, odd)[0] == TM.audit(odd, world.dlog, world.g2log, world.pb) == (False, 2, CM.POK, 1)


def test_a_fresh_file_truncated_has_an_empty_chain_that_holds(world):
    K = world.K
    got, _ = K.ptau_truncate(world.raw(3, (1, 1, 1)), 1, device=NOWHERE)
    assert _verdict(K, got)[0] == (True, 0, 0, 0)
    assert got == TM.patched(world.raw(1, (1, 1, 1)), 3, struct.pack("<I", 0))
