"""groth16_ptau_truncate on the GPU (needs an MI355X): a PREPARED powers-of-tau file cut down to a lower power, section 12's block
p + 1 fixed up by the fixed-base kernel.  Expected bytes never come from the library's kernels: they are the Python model's own file
of the lower power (tests/ptau_truncate_model.py over tests/ptau_prepare_model.py — a direct O(n²) inverse transform of the discrete
logarithms, turned into points by the generator multiplication, as the other key-tool tests do).  The second diagram — truncate after
prepare against prepare after truncate — is the library against itself, and must agree with the first.  The shapes are the smallest
at which the kernel can still go wrong: blocks of 2 and 4 points (p = 0, 1: a fraction of a wave, tables of 2 + 1 and 2 + 2 entries),
of 8 (P = 3, p = 2), and of 128 (P = 7, p = 6: two waves of a workgroup, the scalar tables' boundary inside the block); the
workgroup strides, so no size takes another path."""
import ctypes as C
import json
import os
import subprocess

import pytest

import ptau_contribute_model as CM
import ptau_prepare_model as PM
import ptau_truncate_model as TM
import zkey_new_circuits as ZC

pytestmark = pytest.mark.gpu

R, Q = PM.R, PM.Q
SEED = bytes(range(32))
TOXIC = (0x1234567 + (5 << 200), 0x89abcde, 0xf012345)
PAIRS = [(P, p) for P in (1, 3, 7) for p in sorted({0, 1, P - 1, P})]
NONCANONICAL, OFF_CURVE = 1, 2
KIND_TEXT = {NONCANONICAL: "a coordinate is not below q", OFF_CURVE: "the point is not on the curve"}


class World:
    def __init__(self, K, O, S):
        self.K, self.S = K, S
        self.fbm = lambda g, sc: K.generator_mul(g, sc)
        self.to_mont = lambda a: O.fq_convert_montgomery(a, True)
        self.pb = CM.PointBytes(O)
        self._raw, self._prepared, self._lib = {}, {}, {}

    def raw(self, power, toxic=TOXIC):
        if (power, toxic) not in self._raw:
            self._raw[power, toxic] = PM.write_unprepared(power, *toxic, self.fbm, self.to_mont)
        return self._raw[power, toxic]

    def prepared(self, power, toxic=TOXIC):
        """the MODEL's prepared file"""
        if (power, toxic) not in self._prepared:
            self._prepared[power, toxic] = PM.expected_prepared(self.raw(power, toxic), power, *toxic, self.fbm, self.to_mont)
        return self._prepared[power, toxic]

    def want(self, P, p, toxic=TOXIC):
        return TM.expected(self.prepared(P, toxic), p, toxic, self.fbm, self.to_mont, True)

    def lib_prepared(self, power):
        """the LIBRARY's prepared file of the model's unprepared one"""
        if power not in self._lib:
            self._lib[power] = self.K.ptau_prepare(self.raw(power))[0]
        return self._lib[power]


@pytest.fixture(scope="module")
def world(gpu, O, S):
    return World(gpu, O, S)


def _devices(K):
    dev = K.Device()
    K.check(K.lib().icicle_get_active_device(C.byref(dev)), "get_active_device")
    hip = C.c_int(-1)
    C.CDLL("libamdhip64.so").hipGetDevice(C.byref(hip))
    return dev.type, dev.id, hip.value


def _same(got, want):
    first = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    assert len(got) == len(want) and got == want, "first difference at byte %d of %d" % (first, len(want))


def test_the_shapes_are_what_the_cases_need():
    """conditions, not measurements: 256-lane workgroups, a lane per element of the block, scalar tables of 2^k and 2^(p+1−k)"""
    assert [(2 << p, CM.table_bits(p)) for p in (0, 1, 2, 6)] == [(2, 1), (4, 1), (8, 2), (128, 4)]
    assert 64 < (2 << 6) < 256                                               # p = 6: two of a workgroup's four waves hold lanes
    assert (0x1234567 + (5 << 200)) % R == TOXIC[0] and all(pow(TOXIC[0], 2 << p, R) != 1 for p in range(8))   # τ in no domain: no identity


@pytest.mark.parametrize("P,p", PAIRS)
def test_every_byte_is_the_models(world, P, p, tmp_path):
    K = world.K
    before = _devices(K)
    full, want = world.prepared(P), world.want(P, p)
    assert K.ptau_truncated_size(full, p) == len(want)
    got, rep = K.ptau_truncate(full, p)
    _same(got, want)
    fixed = 0 if p == P else 2 << p
    assert (rep.power_in, rep.power_out, rep.prepared, rep.points_fixed, rep.in_bytes, rep.out_bytes) == (P, p, 1, fixed, len(full), len(want))
    assert (rep.fault_section, rep.fault_kind, rep.fault_count) == (0, 0, 0)
    assert (rep.upload_ms > 0 and rep.device_ms > 0 and rep.download_ms > 0) == (p < P)
    if p < P:
        # a prefix copy is NOT the file: the block that was fixed up differs from the input's in every element
        n2 = 2 << p
        theirs, ours = PM.payload(full, 12)[(n2 - 1) * 64:(2 * n2 - 1) * 64], PM.payload(got, 12)[(n2 - 1) * 64:]
        assert len(ours) == n2 * 64 and all(theirs[64 * j:64 * j + 64] != ours[64 * j:64 * j + 64] for j in range(n2))
        assert PM.payload(got, 12)[:(n2 - 1) * 64] == PM.payload(full, 12)[:(n2 - 1) * 64]
        assert TM.powers(got) == (p, P) and PM.sections(got)[1] == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    (tmp_path / "in.ptau").write_bytes(full)
    none, rep = K.ptau_truncate(tmp_path / "in.ptau", p, out=tmp_path / "out.ptau")
    assert none is None and rep.write_ms > 0 and rep.out_bytes == len(want)
    _same((tmp_path / "out.ptau").read_bytes(), want)
    assert sorted(os.listdir(tmp_path)) == ["in.ptau", "out.ptau"]
    assert _devices(K) == before


@pytest.mark.parametrize("P,p", PAIRS)
def test_the_diagram_commutes_in_the_library(world, P, p):
    """truncate(prepare(U), p) == prepare(truncate(U, p)), and both are the model's"""
    K = world.K
    U = world.raw(P)
    left = K.ptau_truncate(world.lib_prepared(P), p)[0]
    right = K.ptau_prepare(K.ptau_truncate(U, p)[0])[0]
    _same(left, right)
    _same(left, world.want(P, p))


def _lane_scalars(toxic, p):
    """logarithms of B_j, T_j = s_j·Q and B′_j for the block p + 1 of the full file: the hand derivation, in integers"""
    tau = toxic[0]
    n2 = 2 << p
    B = PM.inverse_transform([pow(tau, i, R) for i in range(n2)], p + 1)
    w, ninv = PM.omega(p + 1), pow(n2, -1, R)
    T = [pow(w, j, R) * ninv % R * pow(tau, n2 - 1, R) % R for j in range(n2)]
    return B, T, [(b - t) % R for b, t in zip(B, T)]


DEGENERATE = {
    # name: (τ, P, p, the condition on (B, T, B′) that makes the case what it claims)
    "tau_one": (1, 3, 1, lambda B, T, Bp: B[0] == 1 and not any(B[1:]) and all(T) and all(Bp)),          # B_j the identity for j ≠ 0
    "cube_root": (TM.CUBE_ROOT, 3, 1, lambda B, T, Bp: T[0] == B[0] != 0 and Bp[0] == 0 and all(Bp[1:])),   # lane 0: T = B, the identity out
    "minus_half": (R - pow(2, -1, R), 3, 0, lambda B, T, Bp: (T[0] + B[0]) % R == 0 and B[0] and (T[1] + B[1]) % R),  # lane 0: T = −B
    "half": (pow(2, -1, R), 3, 0, lambda B, T, Bp: (T[1] + B[1]) % R == 0 and B[1] and (T[0] + B[0]) % R),            # lane 1: T = −B
}


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_lanes(world, name):
    K = world.K
    tau, P, p, holds = DEGENERATE[name]
    toxic = (tau,) + TOXIC[1:]
    B, T, Bp = _lane_scalars(toxic, p)
    assert holds(B, T, Bp), name                                             # a condition on the inputs
    assert Bp == PM.prepared_scalars(p, *toxic)[12][(2 << p) - 1:]            # the hand derivation IS the model's last block
    full, want = world.prepared(P, toxic), world.want(P, p, toxic)
    got, rep = K.ptau_truncate(full, p)
    _same(got, want)
    assert rep.points_fixed == 2 << p
    block = PM.payload(got, 12)[((2 << p) - 1) * 64:]
    assert [j for j in range(2 << p) if block[64 * j:64 * j + 64] == bytes(64)] == [j for j, x in enumerate(Bp) if x == 0]
    _same(K.ptau_prepare(K.ptau_truncate(world.raw(P, toxic), p)[0])[0], want)


def test_the_starting_file(world):
    """ptau_new's file, τ = α = β = 1, prepared by the library: every B_j but the first is the identity, and Q is the generator"""
    K = world.K
    new = K.ptau_new(3)
    for p in (0, 1, 2):
        _same(K.ptau_truncate(K.ptau_prepare(new)[0], p)[0], K.ptau_prepare(K.ptau_truncate(new, p)[0])[0])


def _put(image, sid, element, new):
    off = PM.sections(image)[0][sid][0] + element * 64
    e = bytearray(image)
    e[off:off + len(new)] = new
    return bytes(e)


def _word(v):
    return int(v).to_bytes(32, "little")


def test_faults(world, tmp_path):
    K = world.K
    before = _devices(K)
    P, p = 7, 4
    full, want = world.prepared(P), world.want(P, p)
    n2 = 2 << p
    first = n2 - 1                                                           # block p + 1 begins here in section 12; Q is here in section 2
    bad_points = {NONCANONICAL: _word(Q) + bytes(32), OFF_CURVE: _word(1) + bytes(32)}

    def refused(bad, section, element, kind, count):
        text = "ptau: section %d, element %d: %s" % (section, element, KIND_TEXT[kind])
        with pytest.raises(K.PointFault, match=r"\(-2\)") as e:
            K.ptau_truncate(bad, p)
        assert text in str(e.value), str(e.value)
        rep, buf = K.PtauTruncateReport(), C.create_string_buffer(b"\x5a" * len(want), len(want))
        rc = K.lib().groth16_ptau_truncate(C.c_char_p(bad), C.c_size_t(len(bad)), C.c_uint32(p), buf, C.c_size_t(len(want)), b"HIP", C.byref(rep))
        assert rc == -2 and buf.raw == b"\x5a" * len(want)                   # nothing is written
        assert (rep.fault_section, rep.fault_index, rep.fault_kind, rep.fault_count) == (section, element, kind, count)

    for kind, b in bad_points.items():
        # in the block: the lowest of two is named, both are counted; at Q
        refused(_put(_put(full, 12, first + n2 - 1, b), 12, first + 5, b), 12, first + 5, kind, 2)
        refused(_put(full, 12, first, b), 12, first, kind, 1)
        refused(_put(full, 2, first, b), 2, first, kind, 1)
        # in a copied prefix: copied; in a dropped tail: ignored
        for sid, element in ((12, first - 1), (12, 0), (2, first - 1), (14, 3), (4, 2)):
            got = K.ptau_truncate(_put(full, sid, element, b), p)[0]
            _same(got, _put(want, sid, element, b))
        for sid, element in ((12, first + n2), (12, 4 * (1 << P) - 2), (2, first + 1), (14, n2 - 1), (4, 1 << p)):
            _same(K.ptau_truncate(_put(full, sid, element, b), p)[0], want)
    # the file entry leaves neither the file nor a temporary behind
    (tmp_path / "bad.ptau").write_bytes(_put(full, 12, first + 5, bad_points[OFF_CURVE]))
    with pytest.raises(K.PointFault, match=r"\(-2\).*section 12, element %d" % (first + 5)):
        K.ptau_truncate(tmp_path / "bad.ptau", p, out=tmp_path / "never.ptau")
    assert sorted(os.listdir(tmp_path)) == ["bad.ptau"]
    # Q the identity (no honest file has one): nothing to subtract, the block is the input's
    zeroq = K.ptau_truncate(_put(full, 2, first, bytes(64)), p)
    assert zeroq[1].points_fixed == 0 and PM.payload(zeroq[0], 12) == PM.payload(full, 12)[:(2 * n2 - 1) * 64]
    with pytest.raises(K.ProverError, match=r"\(-3\).*does not name one HIP device"):
        K.ptau_truncate(full, p, device="HIP:0-1")
    assert _devices(K) == before
    _same(K.ptau_truncate(full, p)[0], want)                                 # a following good call is as good as before


def test_downstream(world):
    """a ceremony at power 7 served at power 4: verify, the audit, the packed form, and a key whose section-12 reads are the block
    that was fixed up (domain 16 reads block 5 of a power-4 file) — down to a verified proof"""
    K, S = world.K, world.S
    P, p = 7, 4
    pot = K.ptau_new(P)
    for name in ("first", "second"):
        pot, _ = K.ptau_contribute(pot, name=name)
    small_raw = K.ptau_truncate(pot, p)[0]
    ptau = K.ptau_truncate(K.ptau_prepare(pot)[0], p)[0]
    other = K.ptau_prepare(small_raw)[0]
    _same(ptau, other)
    ok, rep = K.ptau_verify(ptau, seed=SEED)
    assert ok is True and (rep.kind, rep.failed_mask, rep.prepared, rep.power) == (0, 0, 1, p)
    # the audit reads the unprepared file: sections 1 to 7 of the two are the same bytes
    assert ptau[12:len(small_raw)] == small_raw[12:]
    ok, rep = K.ptau_contributions(small_raw)
    full_ok, full_rep = K.ptau_contributions(pot)
    assert ok is True and full_ok is True and rep.count == 2 and rep.records == full_rep.records
    packed = K.ptau_pack(ptau)[0]
    _same(K.ptau_unpack(packed)[0], ptau)
    # contribute refuses a truncation, before any device work, and writes nothing
    rep, buf = K.PtauContributeReport(), C.create_string_buffer(b"\x5a" * (len(small_raw) + 1000), len(small_raw) + 1000)
    rc = K.lib().groth16_ptau_contribute(C.c_char_p(small_raw), C.c_size_t(len(small_raw)), None, b"late", buf, C.c_size_t(len(buf)), b"HIP:99", None, C.byref(rep))
    K.lib().groth16_last_error.restype = C.c_char_p
    assert rc == -2 and buf.raw == b"\x5a" * len(buf) and b"contribute to the full file" in K.lib().groth16_last_error()
    r, w = S.squaring_chain(7)
    h = K.R1cs(S.write_r1cs(r))
    try:
        key = h.new_zkey(ptau)[0]
        assert key == h.new_zkey(other)[0]
        ok, rep = h.verify_zkey(key, ptau, seed=SEED)
        assert ok is True and (rep.kind, rep.failed_mask) == (0, 0)
        key1, _ = K.zkey_contribute(key, name="phase 2")
        assert h.verify_zkey(key1, ptau, seed=SEED)[0] is True
        vk = K.zkey_export_vk(key1)
        cm = K.CacheManager()
        try:
            cm.load("truncated", key1)
            pj, qj, _ = cm.prove_mem("truncated", S.write_wtns(w), 3, 5)
            assert json.loads(qj) == [str(v) for v in w[1:1 + r.n_public]]
            assert K.groth16_verify_json(pj, qj, vk) is True
            bad = list(w)
            bad[3] = (bad[3] + 1) % R                                       # CONSTRUCTED: one wire off by one
            assert not ZC.check_r1cs(r, bad)
            pj, qj, _ = cm.prove_mem("truncated", S.write_wtns(bad), 3, 5)
            assert K.groth16_verify_json(pj, qj, vk) is False
        finally:
            cm.close()
    finally:
        h.close()


def test_repl(world, tmp_path):
    K = world.K
    t = tmp_path
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    P, p = 3, 1
    full, want = world.prepared(P), world.want(P, p)
    raw = world.raw(P, (1, 1, 1))                                            # the starting file: an empty chain that holds
    n2 = 2 << p
    (t / "f.ptau").write_bytes(full)
    (t / "u.ptau").write_bytes(raw)
    (t / "bad.ptau").write_bytes(_put(full, 12, n2 - 1 + 2, _word(1) + bytes(32)))
    cmds = (f"ptau-truncate --ptau {t}/f.ptau --power {p} --out {t}/f1.ptau --device HIP\n"
            f"ptau-truncate --ptau {t}/u.ptau --power {p} --out {t}/u1.ptau\n"
            f"ptau-truncate --ptau {t}/bad.ptau --power {p} --out {t}/never.ptau\n"
            f"ptau-truncate --ptau {t}/f.ptau --power 4 --out {t}/never.ptau\n"
            f"ptau-truncate --ptau {t}/f.ptau --out {t}/never.ptau\n"
            f"ptau-contributions --ptau {t}/u1.ptau\nnonsense\nexit\n")
    run = subprocess.run([os.path.join(root, "icicle-snark_amd", "lib", "prove")], input=cmds, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lines = [ln.replace("> ", "") for ln in run.stdout.splitlines()]
    small = TM.expected(raw, p, (1, 1, 1), world.fbm, world.to_mont, False)
    assert lines[0].startswith("power 3 to 1 prepared fixed 4 bytes %d to %d; upload " % (len(full), len(want))) and lines[1:3] == ["PTAU_WRITTEN", "COMMAND_COMPLETED"]
    assert lines[3].startswith("power 3 to 1 unprepared fixed 0 bytes %d to %d; upload 0 ms device 0 ms" % (len(raw), len(small))) and lines[4:6] == ["PTAU_WRITTEN", "COMMAND_COMPLETED"]
    assert lines[6:8] == ["PTAU_BAD POINT 12 %d 1" % (n2 - 1 + 2), "COMMAND_COMPLETED"]
    assert "ptau-truncate failed (-2): ptau: section 12, element %d: the point is not on the curve" % (n2 - 1 + 2) in run.stderr
    assert lines[8] == "COMMAND_COMPLETED" and "ptau-truncate failed (-3): ptau: power 4 is above the file's 3" in run.stderr
    assert lines[9] == "COMMAND_COMPLETED" and "--power <p> is required" in run.stderr
    assert lines[10:12] == ["CHAIN_OK", "COMMAND_COMPLETED"]
    assert "ptau-truncate --ptau <file> --power <p> --out <file> [--device HIP]" in run.stdout
    _same((t / "f1.ptau").read_bytes(), want)
    _same((t / "u1.ptau").read_bytes(), small)
    assert sorted(os.listdir(t)) == ["bad.ptau", "f.ptau", "f1.ptau", "u.ptau", "u1.ptau"]
