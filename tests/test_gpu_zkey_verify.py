"""groth16_zkey_verify_ptau on the GPU (needs an MI355X): is a proving key the Groth16 key of an .r1cs over a prepared .ptau?
The circuit is test_gpu_witness_check's (163 wires, 153 constraints, npub 2, domain 256), the ptaus have power 8 (the domain's own)
and power 10 (the blocks that are read begin in the middle of their sections).  Every key is CONSTRUCTED from scalar lists
(tests/zkey_verify_cases.py), and the kind, index and mask expected of the library come from the discrete-log model over the same
lists and the same seed (tests/zkey_verify_dlog_model.py) — never from the library."""
import hashlib
import os
import struct
import subprocess

import pytest

import zkey_verify_cases as cases
import zkey_verify_dlog_model as M
from test_gpu_witness_check import Circuit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [hashlib.sha256(b"zkey-verify %d" % k).digest() for k in range(8)]
CASE_NAMES = ["untouched", "other gamma and delta", "two points of a swapped", "two points of b1 swapped", "two points of b2 swapped",
              "two points of c swapped", "two points of h swapped", "two points of ic swapped", "C coefficient of a private wire",
              "C coefficient of a public wire", "another circuit of the same sizes", "another tau, header alpha and beta the ptau's",
              "another tau, alpha and beta", "built with another delta than the header's", "H on the plain domain"]


def _sections(image):
    pos, out = 12, {}
    for _ in range(struct.unpack_from("<I", image, 8)[0]):
        sid, ln = struct.unpack_from("<IQ", image, pos)
        out[sid] = (pos + 12, ln)
        pos += 12 + ln
    return out


class World:
    """the files of one circuit family: setup()'s key, the ptaus, and keys built from scalar lists"""

    def __init__(self, K, O, S, powers=(8, 10)):
        self.K, self.O, self.S = K, O, S
        self.fbm = lambda g, sc: K.generator_mul(g, sc)
        self.to_mont = lambda a: O.fq_convert_montgomery(a, True)
        self.ptau = {p: S.write_ptau(p, self.fbm, points_to_mont=self.to_mont) for p in powers}
        self.handles = {}

    def points(self, g, xs):
        return self.to_mont(self.fbm(g, self.S.ints_to_arr(xs))).tobytes() if xs else b""

    def setup(self, r, **kw):
        return self.S.setup(r, self.fbm, points_to_mont=self.to_mont, **kw)[0]

    def zkey(self, template, key, header):
        """`template` (a key of the same sizes) with the header's points and sections 3, 5, 6, 7, 8, 9 made from the scalars"""
        g1_lists = [[header["alpha1"], header["beta1"], header["delta1"]], key["ic"], key["a"], key["b1"], key["c"], key["h"]]
        g1 = self.points("g1", [x for xs in g1_lists for x in xs])
        g2 = self.points("g2", [header["beta2"], header["gamma2"], header["delta2"]] + key["b2"])
        cut, o = [], 0
        for xs in g1_lists:
            cut.append(g1[o:o + 64 * len(xs)])
            o += 64 * len(xs)
        hd, ic, a, b1, c, h = cut
        payload = {3: ic, 5: a, 6: b1, 7: g2[384:], 8: c, 9: h}
        secs = _sections(template)
        off2, len2 = secs[2]
        points = hd[0:64] + hd[64:128] + g2[0:128] + g2[128:256] + hd[128:192] + g2[256:384]
        payload[2] = template[off2:off2 + 84] + points + template[off2 + 84 + len(points):off2 + len2]
        out = bytes(template[:12])
        for sid, (off, ln) in secs.items():
            p = payload.get(sid, template[off:off + ln])
            assert len(p) == ln
            out += struct.pack("<IQ", sid, ln) + p
        return out

    def handle(self, r):
        if id(r) not in self.handles:
            self.handles[id(r)] = (r, self.K.R1cs(self.S.write_r1cs(r)))
        return self.handles[id(r)][1]

    def close(self):
        for _, h in self.handles.values():
            h.close()


@pytest.fixture(scope="module")
def world(gpu, O, S):
    w = World(gpu, O, S)
    yield w
    w.close()


@pytest.fixture(scope="module")
def base(world, S):
    """the base circuit, its setup() key, and every constructed case by name"""
    r = cases.base_circuit(S)
    zkey = world.setup(r)
    return r, zkey, {c[0]: c for c in cases.cases(S, r)}


def _triple(rep):
    return rep.kind, rep.index, rep.failed_mask


def test_the_inputs_have_the_shape_the_cases_need(world, base, gpu, S):
    r, zkey, by_name = base
    live = Circuit(gpu, S)
    try:
        assert (r.n_vars, r.n_public, r.n_constraints) == (163, 2, 153) and (r.A, r.B, r.C) == (live.r.A, live.r.B, live.r.C)
    finally:
        live.h.close()
    assert sorted(by_name) == sorted(CASE_NAMES)
    # the builder writes setup()'s own bytes from setup()'s own scalars
    assert world.zkey(zkey, by_name["untouched"][2], by_name["untouched"][3]) == zkey
    assert gpu.ptau_info(world.ptau[8], domain_power=8).power == 8 and gpu.ptau_info(world.ptau[10], domain_power=8).power == 10


def test_untouched_key_verifies_for_every_seed(world, base):
    r, zkey, _ = base
    h = world.handle(r)
    for power in (8, 10):
        for seed in SEEDS + [None]:
            ok, rep = h.verify_zkey(zkey, world.ptau[power], seed=seed)
            assert ok is True and _triple(rep) == (0, 0, 0) and rep.key.kind == 0, (power, _triple(rep), rep.key.kind)
            assert rep.device_ms > 0 and rep.upload_ms > 0 and rep.pairing_ms > 0
    # the same seed gives the same report
    a, b = h.verify_zkey(zkey, world.ptau[10], seed=SEEDS[3])[1], h.verify_zkey(zkey, world.ptau[10], seed=SEEDS[3])[1]
    assert _triple(a) == _triple(b) and list(a.key.faults) == list(b.key.faults)
    # the handle still answers the other two questions
    assert h.match_zkey(zkey, seed=SEEDS[0])[0] is True


@pytest.mark.parametrize("name", CASE_NAMES)
def test_constructed_case(world, base, S, name):
    r, zkey, by_name = base
    _, circuit, key, header, kind, mask = by_name[name]
    image = world.zkey(zkey, key, header)
    h = world.handle(circuit)
    for power, seed in ((8, SEEDS[1]), (10, SEEDS[2])):
        want = M.evaluate(S, circuit, key, header, S.toxic_waste()[:3], seed)
        assert want[0] == kind and (mask is None or want[2] == mask)
        ok, rep = h.verify_zkey(image, world.ptau[power], seed=seed)
        assert _triple(rep) == want, (name, power, M.NAMES[rep.kind], _triple(rep), want)
        assert ok == (kind == 0)
        # sections 6 and 7 swapped alone also disagree with each other: the key check says so, and the equations still run
        assert (rep.key.kind, rep.key.section) == ((world.K.ZKEY_PAIR_MISMATCH, 6) if kind in (M.B1, M.B2) else (0, 0))
    if name.startswith("two points"):
        sid = {"a": 5, "b1": 6, "b2": 7, "c": 8, "h": 9, "ic": 3}[name.split()[3]]
        off, ln = _sections(zkey)[sid]
        size = 128 if sid == 7 else 64
        differing = [k for k in range(ln // size) if image[off + k * size:off + (k + 1) * size] != zkey[off + k * size:off + (k + 1) * size]]
        assert len(differing) == 2                                   # two points, and they differ
        i, j = differing
        assert image[off + i * size:off + (i + 1) * size] == zkey[off + j * size:off + (j + 1) * size]
    if name.startswith("C coefficient"):
        # THE case the other checks cannot see: section 4 does not hold C, so the key still matches the changed circuit
        ok, mrep = h.match_zkey(image, seed=SEEDS[0])
        assert ok is True and mrep.kind == 0
        assert world.K.zkey_check(image, seed=SEEDS[0])[0] is True


def test_a_point_off_its_curve_is_the_key_checks_fault(world, base):
    r, zkey, _ = base
    bad = bytearray(zkey)
    bad[_sections(zkey)[5][0] + 64 * 3 + 32] ^= 1                    # CONSTRUCTED: one bit of A₃'s y
    ok, rep = world.handle(r).verify_zkey(bytes(bad), world.ptau[8], seed=SEEDS[0])
    assert ok is False and _triple(rep) == (M.KEY, 0, 0)
    assert (rep.key.kind, rep.key.section, rep.key.index, rep.key.faults[5]) == (world.K.ZKEY_OFF_CURVE, 5, 3, 1)


def test_a_ptau_point_off_its_curve_is_a_format_error(world, base):
    r, zkey, _ = base
    bad = bytearray(world.ptau[10])
    off14 = _sections(world.ptau[10])[14][0]
    bad[off14 + (255 + 7) * 64 + 32] ^= 1                            # block 8 of section 14, element 7
    with pytest.raises(world.K.ProverError, match=r"\(-2\).*section 14, block 8, element 7: the point is not on the curve"):
        world.handle(r).verify_zkey(zkey, bytes(bad), seed=SEEDS[0])
    bad = bytearray(world.ptau[10])
    bad[off14 + 254 * 64 + 32] ^= 1                                  # the last element of block 7: not read
    assert world.handle(r).verify_zkey(zkey, bytes(bad), seed=SEEDS[0])[0] is True


def test_an_early_error_of_the_file_entry_leaves_no_file_hint(world, base, tmp_path):
    """groth16_zkey_verify_ptau_file returns early from inside its ptau uploads — the staging workers are then reading the mapped
    ptau by descriptor — and the same thread's next call, a key check from memory, must copy out of memory again"""
    r, zkey, _ = base
    bad = bytearray(world.ptau[10])
    bad[_sections(world.ptau[10])[14][0] + (255 + 7) * 64 + 32] ^= 1   # block 8 of section 14, element 7
    (tmp_path / "k.zkey").write_bytes(zkey)
    (tmp_path / "bad.ptau").write_bytes(bytes(bad))
    with pytest.raises(world.K.ProverError, match=r"\(-2\).*section 14, block 8, element 7: the point is not on the curve"):
        world.handle(r).verify_zkey(tmp_path / "k.zkey", tmp_path / "bad.ptau", seed=SEEDS[0])
    ok, rep = world.K.zkey_check(zkey, seed=SEEDS[0])
    assert ok is True and rep.kind == 0 and list(rep.faults) == [0] * 10


def test_sizes(world, base, S):
    r, zkey, _ = base
    other, _ = S.random_circuit(150, 3, 9, seed=11)
    ok, rep = world.handle(other).verify_zkey(zkey, world.ptau[8], seed=SEEDS[0])
    assert ok is False and _triple(rep) == (M.SIZES, 1, 0) and list(rep.key.faults) == [0] * 10


def _edge(world, S, r, mutate="a"):
    """accepts setup()'s key, and names one swap, as the model does"""
    zkey = world.setup(r)
    toxic = S.toxic_waste()
    key, header = M.key_from(S.key_scalars(r, toxic)), cases.header_of(toxic)
    h = world.handle(r)
    ok, rep = h.verify_zkey(zkey, world.ptau[8], seed=SEEDS[4])
    assert M.evaluate(S, r, key, header, toxic[:3], SEEDS[4]) == (0, 0, 0)
    assert ok is True and _triple(rep) == (0, 0, 0), (M.NAMES[rep.kind], _triple(rep))
    bad = dict(key)
    bad[mutate], _ = cases.swapped(key[mutate])
    want = M.evaluate(S, r, bad, header, toxic[:3], SEEDS[5])
    assert want[0] != 0
    ok, rep = h.verify_zkey(world.zkey(zkey, bad, header), world.ptau[8], seed=SEEDS[5])
    assert ok is False and _triple(rep) == want
    return zkey


def test_edge_binding_rows_end_the_domain(world, S):
    r, _ = S.random_circuit(253, 2, 10, seed=21)
    assert r.n_constraints + r.n_public + 1 == 256
    _edge(world, S, r)
    _edge(world, S, r, "ic")          # IC reads the binding rows


def test_edge_no_public_signals(world, S):
    r, _ = S.random_circuit(20, 0, 5, seed=22)
    assert r.n_public == 0 and S.key_scalars(r)["n"] == 32
    _edge(world, S, r, "c")


def test_edge_no_private_wires(world, S):
    """section 8 is empty: both sides of C are the identity, and the equation holds"""
    r = S.R1CS(n_vars=3, n_public=2, n_constraints=2, A=[(0, 1, 1), (1, 2, 3)], B=[(0, 2, 1), (1, 0, 1)], C=[(0, 0, 5), (1, 1, 2)])
    zkey = _edge(world, S, r, "ic")
    assert _sections(zkey)[8][1] == 0 and S.key_scalars(r)["n"] == 8


def test_edge_one_wire_in_every_constraint(world, S):
    r, _ = S.random_circuit(70, 1, 4, seed=23)
    r.A += [(j, 5, 7 + j) for j in range(70)]
    r.C += [(j, 5, 1) for j in range(70)]
    _edge(world, S, r, "c")


def test_errors_leave_the_handle_usable(world, base, gpu, S):
    r, zkey, _ = base
    live = Circuit(gpu, S)
    try:
        h = live.h

        def still_works():
            assert h.check(live.wtns(live.w))[0] is True and h.match_zkey(zkey, seed=SEEDS[0])[0] is True

        low = S.write_ptau(7, world.fbm, points_to_mont=world.to_mont)
        with pytest.raises(gpu.ProverError, match=r"\(-3\).*power 7 is below the key's domain 2\^8"):
            h.verify_zkey(zkey, low, seed=SEEDS[0])
        still_works()
        with pytest.raises(ValueError):
            h.verify_zkey(zkey, world.ptau[8], seed=b"short")
        still_works()
        with pytest.raises(gpu.ProverError, match=r"\(-2\)"):
            h.verify_zkey(zkey[:1000], world.ptau[8], seed=SEEDS[0])
        still_works()
        with pytest.raises(gpu.ProverError, match=r"\(-2\).*expected 'ptau'"):
            h.verify_zkey(zkey, zkey, seed=SEEDS[0])
        still_works()
        assert h.verify_zkey(zkey, world.ptau[8], seed=SEEDS[0])[0] is True
    finally:
        live.h.close()


def test_files_and_the_repl_give_the_same_verdicts(world, base, S, tmp_path):
    r, zkey, by_name = base
    changed = by_name["C coefficient of a private wire"][1]
    swapped = world.zkey(zkey, by_name["two points of h swapped"][2], by_name["two points of h swapped"][3])
    for name, data in (("c.r1cs", S.write_r1cs(r)), ("changed.r1cs", S.write_r1cs(changed)), ("k.zkey", zkey), ("h.zkey", swapped), ("pot.ptau", world.ptau[10])):
        (tmp_path / name).write_bytes(data)
    ok, rep = world.handle(r).verify_zkey(tmp_path / "k.zkey", tmp_path / "pot.ptau", seed=SEEDS[6])
    assert ok is True and _triple(rep) == (0, 0, 0)
    ok, rep = world.handle(r).verify_zkey(str(tmp_path / "h.zkey"), str(tmp_path / "pot.ptau"), seed=SEEDS[6])
    assert ok is False and _triple(rep) == (M.H, 0, M.bit(M.H))
    exe = os.path.join(ROOT, "icicle-snark_amd", "lib", "prove")
    cmds = (f"zkey-verify --r1cs {tmp_path}/c.r1cs --zkey {tmp_path}/k.zkey --ptau {tmp_path}/pot.ptau --device HIP\n"
            f"zkey-verify --r1cs {tmp_path}/changed.r1cs --zkey {tmp_path}/k.zkey --ptau {tmp_path}/pot.ptau\n"
            f"zkey-verify --r1cs {tmp_path}/c.r1cs --zkey {tmp_path}/h.zkey --ptau {tmp_path}/pot.ptau\n"
            f"zkey-verify --r1cs {tmp_path}/c.r1cs --zkey {tmp_path}/k.zkey --ptau {tmp_path}/missing.ptau\nexit\n")
    out = subprocess.run([exe], input=cmds, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [ln.replace("> ", "") for ln in out.stdout.splitlines()]
    match = "section 4 against the circuit: match"
    points = "point sections against the circuit and the ptau: "
    assert lines[:12] == [match, points + "verified", "ZKEY_OK", "COMMAND_COMPLETED",
                          match, points + "not verified: C, failing: C", "ZKEY_NOT_OK", "COMMAND_COMPLETED",
                          match, points + "not verified: H, failing: H", "ZKEY_NOT_OK", "COMMAND_COMPLETED"], out.stdout
    assert lines[12:14] == [match, "COMMAND_COMPLETED"] and "zkey-verify failed (-1)" in out.stderr
    help_text = subprocess.run([exe], input="nonsense\nexit\n", capture_output=True, text=True, timeout=300).stdout
    assert "zkey-verify --r1cs <file> --zkey <file> --ptau <file> [--device HIP]" in help_text
