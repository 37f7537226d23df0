"""groth16_points_pack / _unpack and groth16_ptau_pack / _unpack on the GPU (needs an MI355X): every point of a powers-of-tau file as
x and one bit of y, and back by a square root per point.  Expected bytes never come from the library's kernels: the packed words and
the packed file are tests/point_pack_model.py's, Python integers over the input's bytes, and the unpacked file is the input itself.
The shapes are the smallest at which the kernels can still go wrong: n = 0, 1, the edges of a wave (63, 64, 65) and of the G1
workgroup (257 = 256 + 1); files of power 0 (one point per section), 1, 3 and 7 (section 2 has 255 points, section 12 of the
prepared file 511: two G1 workgroups, the last a lane short; the G2 sections fill two and four 64-lane workgroups)."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import groth16_dlog_model as M
import point_pack_model as PK
import ptau_contribute_model as CM
import ptau_prepare_model as PM
import zkey_contribute_model as ZM

pytestmark = pytest.mark.gpu

R, Q = PM.R, PM.Q
SEED = bytes(range(32))
POWERS = [0, 1, 3, 7]
NONCANONICAL, OFF_CURVE, OFF_SUBGROUP = 1, 2, 3
S1, S2 = bytes([0x11]) * 32, bytes([0x22]) * 32
P1 = (ZM.FULL, (R - 1) // 2, 12345)
P2 = (3, R - 2, (1 << 127) + 9)
TWIST_OUTSIDE = M.twist_point_outside_subgroup()                            # standard form (x0, x1, y0, y1)
TWIST_OUTSIDE_FILE = b"".join(PK.to_file(c).to_bytes(32, "little") for c in TWIST_OUTSIDE)
TWIST_OUTSIDE_WORD = PK.pack_g2(TWIST_OUTSIDE_FILE)


class World:
    def __init__(self, K, O):
        self.K = K
        self.pb = CM.PointBytes(O)
        self._files = {}

    def files(self, power):
        """(unprepared, prepared): ptau_new → contribute ×2 with fixed secrets, and ptau_prepare of that; made once"""
        if power not in self._files:
            K = self.K
            i1, _ = K.ptau_contribute(K.ptau_new(power), secret=S1, name="alice", tau=P1[0], alpha=P1[1], beta=P1[2])
            i2, _ = K.ptau_contribute(i1, secret=S2, name=b"bob \xc3\xa9", tau=P2[0], alpha=P2[1], beta=P2[2])
            self._files[power] = (i2, K.ptau_prepare(i2)[0])
        return self._files[power]

    def points(self, g2, n):
        """n file-form points: multiples of the generator with mixed signs, the identity at the first and at the last index"""
        ks = [0 if i in (0, n - 1) else (i if i % 3 else R - i) for i in range(n)]
        self.pb.prefetch(**{"g2" if g2 else "g1": ks})
        f = self.pb.g2 if g2 else self.pb.g1
        return b"".join(f(k) for k in ks)


@pytest.fixture(scope="module")
def world(gpu, O):
    return World(gpu, O)


def _devices(K):
    dev = K.Device()
    K.check(K.lib().icicle_get_active_device(C.byref(dev)), "get_active_device")
    hip = C.c_int(-1)
    C.CDLL("libamdhip64.so").hipGetDevice(C.byref(hip))
    return dev.type, dev.id, hip.value


def _same(got, want):
    first = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    assert len(got) == len(want) and got == want, "first difference at byte %d of %d" % (first, len(want))


def _word(v):
    return int(v).to_bytes(32, "little")


# ---- the raw entries
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_raw_round_trip(world, g2, n):
    K = world.K
    pts = world.points(g2, n)
    want = PK.pack_points(pts, g2)
    elem = 64 if g2 else 32
    assert n < 63 or {want[i * elem + elem - 1] >> 7 for i in range(1, n - 1)} == {0, 1}   # both signs occur
    assert n < 2 or want[:elem] == want[-elem:] == bytes(elem - 1) + b"\x40"
    packed, rep = K.points_pack(pts, g2=g2)
    _same(packed, want)
    assert (rep.n, rep.fault_kind, rep.fault_count) == (n, 0, 0)
    back, rep = K.points_unpack(want, g2=g2)
    _same(back, pts)
    assert (rep.n, rep.fault_kind, rep.fault_count) == (n, 0, 0)


def _bad_points(g2):
    """kind → one faulty file-form point"""
    size = 128 if g2 else 64
    out = {NONCANONICAL: _word(Q) + bytes(size - 32), OFF_CURVE: _word(PK.to_file(1)) + bytes(size - 32)}
    if g2:
        out[OFF_SUBGROUP] = TWIST_OUTSIDE_FILE
    return out


def _bad_words(g2):
    """kind → one faulty packed word"""
    if not g2:
        assert PK.unpack_g1(_word(PK.to_file(4)))[0] == OFF_CURVE
        return {NONCANONICAL: _word(Q), OFF_CURVE: _word(PK.to_file(4))}
    assert PK.sqrt_fq2(PK.g2_rhs((3, 0))) is None
    return {NONCANONICAL: _word(1) + _word(Q), OFF_CURVE: _word(PK.to_file(3)) + _word(0), OFF_SUBGROUP: TWIST_OUTSIDE_WORD}


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_raw_faults_name_the_lowest_and_count_all(world, g2):
    """one fault of each kind at the last index and a second at a lower one, in another workgroup"""
    K = world.K
    n, low = 257, 70
    pts = world.points(g2, n)
    words = PK.pack_points(pts, g2)
    for entry, buf, elem, bad in ((K.points_pack, pts, 128 if g2 else 64, _bad_points(g2)), (K.points_unpack, words, 64 if g2 else 32, _bad_words(g2))):
        for kind, b in bad.items():
            e = bytearray(buf)
            e[(n - 1) * elem:n * elem] = b
            e[low * elem:(low + 1) * elem] = b
            with pytest.raises(K.PointFault, match=r"\(-2\).*points: element %d: %s" % (low, PK.KIND_TEXT[kind])) as err:
                entry(bytes(e), g2=g2)
            rep = err.value.report
            assert (rep.fault_index, rep.fault_kind, rep.fault_count) == (low, kind, 2), (entry.__name__, kind)
    # nothing is written
    out, rep = C.create_string_buffer(b"\x5a" * (n * 128), n * 128), K.PointsPackReport()
    e = bytearray(words)
    e[0:len(_bad_words(g2)[OFF_CURVE])] = _bad_words(g2)[OFF_CURVE]
    rc = K.lib().groth16_points_unpack(C.c_char_p(bytes(e)), C.c_uint64(n), C.c_int(int(g2)), out, b"HIP", C.byref(rep))
    assert rc == -2 and out.raw == b"\x5a" * (n * 128) and (rep.fault_index, rep.fault_count) == (0, 1)
    with pytest.raises(K.ProverError, match=r"\(-3\).*does not name one HIP device"):
        K.points_pack(pts, g2=g2, device="HIP:0-1")


# ---- files
def _with_unknown_sections(image):
    """an unknown section behind section 3 and another at the end"""
    secs, order = PM.sections(image)
    body = lambda s: image[secs[s][0]:secs[s][0] + secs[s][1]]
    sec = lambda s, p: struct.pack("<IQ", s, len(p)) + p
    parts = []
    for s in order:
        parts.append(sec(s, body(s)))
        if s == 3:
            parts.append(sec(99, b"in the middle" * 5))
    parts.append(sec(9, bytes(range(77))))
    return image[:8] + struct.pack("<I", len(order) + 2) + b"".join(parts)


@pytest.mark.parametrize("prepared", [False, True], ids=["unprepared", "prepared"])
@pytest.mark.parametrize("power", POWERS)
def test_files_round_trip_in_every_byte(world, power, prepared, tmp_path):
    K = world.K
    before = _devices(K)
    image = world.files(power)[1 if prepared else 0]
    want = PK.pack_file(image)
    N = 1 << power
    packed, rep = K.ptau_pack(image)
    _same(packed, want)
    g1 = (2 * N - 1) + 2 * N + ((4 * N - 1) + 2 * (2 * N - 1) if prepared else 0)
    g2 = N + 1 + ((2 * N - 1) if prepared else 0)
    assert (rep.power, rep.prepared, list(rep.points), rep.in_bytes, rep.out_bytes) == (power, int(prepared), [g1, g2], len(image), len(want))
    assert rep.upload_ms > 0 and rep.device_ms > 0 and rep.download_ms > 0 and (rep.fault_section, rep.fault_kind, rep.fault_count) == (0, 0, 0)
    assert len(want) == K.ptau_packed_size(power, prepared, len(image)) and len(image) == K.ptau_unpacked_size(power, prepared, len(want))
    back, rep = K.ptau_unpack(want)
    _same(back, image)
    assert (rep.power, rep.prepared, list(rep.points), rep.in_bytes, rep.out_bytes) == (power, int(prepared), [g1, g2], len(want), len(image))
    _same(K.ptau_pack(back)[0], want)                                       # pack(unpack(p)) = p
    # the file entries write the same bytes and leave nothing else
    (tmp_path / "in.ptau").write_bytes(image)
    none, rep = K.ptau_pack(tmp_path / "in.ptau", out=tmp_path / "out.ptaz")
    assert none is None and rep.write_ms > 0 and rep.out_bytes == len(want)
    _same((tmp_path / "out.ptaz").read_bytes(), want)
    none, rep = K.ptau_unpack(tmp_path / "out.ptaz", out=tmp_path / "back.ptau")
    assert none is None and rep.write_ms > 0
    _same((tmp_path / "back.ptau").read_bytes(), image)
    assert sorted(os.listdir(tmp_path)) == ["back.ptau", "in.ptau", "out.ptaz"]
    assert _devices(K) == before


@pytest.mark.parametrize("prepared", [False, True], ids=["unprepared", "prepared"])
def test_section_7_and_unknown_sections_survive_in_place(world, prepared):
    K = world.K
    image = _with_unknown_sections(world.files(3)[1 if prepared else 0])
    want = PK.pack_file(image)
    order = PM.sections(image)[1]
    assert order.index(99) == order.index(3) + 1 and order[-1] == 9 and len(PM.payload(image, 7)) > 2 * CM.FIXED
    packed = K.ptau_pack(image)[0]
    _same(packed, want)
    assert PM.sections(packed)[1] == order
    for sid in (1, 7, 9, 99):
        assert PM.payload(packed, sid) == PM.payload(image, sid)
    _same(K.ptau_unpack(packed)[0], image)
    assert len(packed) == K.ptau_packed_size(3, prepared, len(image))


def test_the_starting_file_and_its_identities(world):
    """ptau_new(3): tau = 1, so its prepared blocks hold identities — the identity path inside real sections"""
    K = world.K
    new = K.ptau_new(3)
    prepared = K.ptau_prepare(new)[0]
    assert bytes(64) in [PM.payload(prepared, 12)[i:i + 64] for i in range(0, 31 * 64, 64)] and PM.payload(prepared, 13)[256:384] == bytes(128)
    for image in (new, prepared):
        want = PK.pack_file(image)
        _same(K.ptau_pack(image)[0], want)
        _same(K.ptau_unpack(want)[0], image)
    assert bytes(31) + b"\x40" in [PM.payload(want, 12)[i:i + 32] for i in range(0, 31 * 32, 32)]


def _put(image, sid, element, elem_bytes, new):
    off = PM.sections(image)[0][sid][0] + element * elem_bytes
    e = bytearray(image)
    e[off:off + len(new)] = new
    return bytes(e)


def test_refusals_leave_nothing_written(world, tmp_path):
    K = world.K
    before = _devices(K)
    raw, prepared = world.files(3)
    packed, pp = PK.pack_file(raw), PK.pack_file(prepared)

    def refused(buffer_entry, wrapper, bad, room, section, element, kind):
        text = "ptau: section %d, element %d: %s" % (section, element, PK.KIND_TEXT[kind])
        with pytest.raises(K.PointFault, match=r"\(-2\)") as e:
            wrapper(bad)
        assert text in str(e.value), str(e.value)
        rep, buf = K.PtauPackReport(), C.create_string_buffer(b"\x5a" * room, room)
        rc = buffer_entry(C.c_char_p(bad), C.c_size_t(len(bad)), buf, C.c_size_t(room), b"HIP", C.byref(rep))
        assert rc == -2 and buf.raw == b"\x5a" * room                        # nothing is written
        assert (rep.fault_section, rep.fault_index, rep.fault_kind) == (section, element, kind)
        return rep

    unpack = lambda bad, *a: refused(K.lib().groth16_ptau_unpack, K.ptau_unpack, bad, len(prepared), *a)
    pack = lambda bad, *a: refused(K.lib().groth16_ptau_pack, K.ptau_pack, bad, len(prepared), *a)
    # CONSTRUCTED words: x = 4 has no point on the curve; a twist point outside the subgroup; x = q; the identity flag with a bit of x
    assert unpack(_put(packed, 2, 6, 32, _word(PK.to_file(4))), 2, 6, OFF_CURVE).fault_count == 1
    unpack(_put(packed, 3, 6, 64, TWIST_OUTSIDE_WORD), 3, 6, OFF_SUBGROUP)
    unpack(_put(pp, 13, 9, 64, TWIST_OUTSIDE_WORD), 13, 9, OFF_SUBGROUP)
    unpack(_put(pp, 14, 14, 32, _word(Q)), 14, 14, NONCANONICAL)
    unpack(_put(packed, 6, 0, 64, _word(1) + _word(PK.IDENTITY_BIT)), 6, 0, NONCANONICAL)
    unpack(_put(packed, 6, 0, 64, TWIST_OUTSIDE_WORD), 6, 0, OFF_SUBGROUP)
    # the lowest faulty section is named, its lowest element, its count; a later section's faults are not counted
    two = _put(_put(_put(packed, 4, 7, 32, _word(Q)), 4, 2, 32, _word(PK.to_file(4))), 5, 1, 32, _word(Q))
    assert unpack(two, 4, 2, OFF_CURVE).fault_count == 2
    # a faulty point in a .ptau handed to pack: one coordinate plus one; a twist point outside the subgroup
    y = int.from_bytes(PM.payload(raw, 4)[5 * 64 + 32:5 * 64 + 64], "little")
    pack(_put(raw, 4, 5, 64, PM.payload(raw, 4)[5 * 64:5 * 64 + 32] + _word((y + 1) % Q)), 4, 5, OFF_CURVE)
    pack(_put(prepared, 13, 14, 128, TWIST_OUTSIDE_FILE), 13, 14, OFF_SUBGROUP)
    pack(_put(raw, 6, 0, 128, TWIST_OUTSIDE_FILE), 6, 0, OFF_SUBGROUP)
    # the file entry leaves neither the file nor a temporary behind
    path, out = tmp_path / "bad.ptaz", tmp_path / "never.ptau"
    path.write_bytes(_put(packed, 2, 6, 32, _word(PK.to_file(4))))
    with pytest.raises(K.PointFault, match=r"\(-2\).*section 2, element 6"):
        K.ptau_unpack(path, out=out)
    assert sorted(os.listdir(tmp_path)) == ["bad.ptaz"]
    with pytest.raises(K.ProverError, match=r"\(-1\).*cannot open"):
        K.ptau_unpack(tmp_path / "missing.ptaz", out=out)
    # equal paths, by name and by inode
    for f in (K.ptau_pack, K.ptau_unpack):
        with pytest.raises(K.ProverError, match=r"\(-3\).*the output path is the input's"):
            f(path, out=path)
    os.link(path, tmp_path / "alias.ptaz")
    with pytest.raises(K.ProverError, match=r"\(-3\).*the output path is the input's"):
        K.ptau_unpack(path, out=tmp_path / "alias.ptaz")
    assert sorted(os.listdir(tmp_path)) == ["alias.ptaz", "bad.ptaz"]
    # cap one byte short: −3, the report says what is needed, nothing is written
    for entry, image, need in ((K.lib().groth16_ptau_pack, raw, len(packed)), (K.lib().groth16_ptau_unpack, packed, len(raw))):
        rep, buf = K.PtauPackReport(), C.create_string_buffer(need)
        rc = entry(C.c_char_p(image), C.c_size_t(len(image)), buf, C.c_size_t(need - 1), b"HIP", C.byref(rep))
        assert rc == -3 and rep.out_bytes == need and buf.raw == bytes(need)
    with pytest.raises(K.ProverError, match=r"\(-3\).*does not name one HIP device"):
        K.ptau_pack(raw, device="HIP:0-1")
    assert _devices(K) == before
    _same(K.ptau_unpack(packed)[0], raw)                                     # a following good call is as good as before


def test_the_existing_tools_refuse_the_packed_form(world):
    K = world.K
    raw, prepared = world.files(1)
    for packed in (PK.pack_file(raw), PK.pack_file(prepared)):
        for call in (lambda p: K.ptau_verify(p, seed=SEED), lambda p: K.ptau_contribute(p, secret=S1), K.ptau_prepare):
            with pytest.raises(K.ProverError, match=r"\(-2\).*Invalid File format \(expected 'ptau'\)"):
                call(packed)


def test_a_ceremony_through_the_packed_form(world):
    """ptau_new(4) → contribute → pack → unpack → ptau_contributions → ptau_verify → ptau_prepare: all pass, and the file is the one
    that never went through the packed form"""
    K = world.K
    pot, _ = K.ptau_contribute(K.ptau_new(4), name="first")
    packed, rep = K.ptau_pack(pot)
    assert len(packed) == rep.out_bytes < 0.51 * len(pot) + 1000
    back, _ = K.ptau_unpack(packed)
    _same(back, pot)
    ok, rep = K.ptau_contributions(back)
    assert ok is True and rep.count == 1
    ok, rep = K.ptau_verify(back, seed=SEED)
    assert ok is True and (rep.kind, rep.failed_mask) == (0, 0)
    prepared = K.ptau_prepare(back)[0]
    assert prepared == K.ptau_prepare(pot)[0]
    assert K.ptau_verify(K.ptau_unpack(K.ptau_pack(prepared)[0])[0], seed=SEED)[0] is True


def test_repl(world, tmp_path):
    K = world.K
    t = tmp_path
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = world.files(3)[0]
    want = PK.pack_file(raw)
    (t / "p.ptau").write_bytes(raw)
    (t / "bad.ptaz").write_bytes(_put(want, 3, 6, 64, TWIST_OUTSIDE_WORD))
    cmds = (f"ptau-pack --ptau {t}/p.ptau --out {t}/p.ptaz --device HIP\n"
            f"ptau-unpack --packed {t}/p.ptaz --out {t}/q.ptau\n"
            f"ptau-unpack --packed {t}/bad.ptaz --out {t}/never.ptau\n"
            f"ptau-pack --ptau {t}/p.ptaz --out {t}/never.ptaz\nexit\n")
    run = subprocess.run([os.path.join(root, "icicle-snark_amd", "lib", "prove")], input=cmds, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lines = [ln.replace("> ", "") for ln in run.stdout.splitlines()]
    assert lines[0].startswith("power 3 unprepared points 31 9 bytes %d to %d; upload " % (len(raw), len(want))) and lines[1:3] == ["PTAU_WRITTEN", "COMMAND_COMPLETED"]
    assert lines[3].startswith("power 3 unprepared points 31 9 bytes %d to %d; upload " % (len(want), len(raw))) and lines[4:6] == ["PTAU_WRITTEN", "COMMAND_COMPLETED"]
    assert lines[6:8] == ["PTAU_BAD POINT 3 6", "COMMAND_COMPLETED"] and "ptau-unpack failed (-2): ptau: section 3, element 6: the point is outside the subgroup" in run.stderr
    assert lines[8] == "COMMAND_COMPLETED" and "ptau-pack failed (-2): Invalid File format (expected 'ptau')" in run.stderr
    _same((t / "p.ptaz").read_bytes(), want)
    _same((t / "q.ptau").read_bytes(), raw)
    assert sorted(os.listdir(t)) == ["bad.ptaz", "p.ptau", "p.ptaz", "q.ptau"]
