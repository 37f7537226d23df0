"""groth16_ptau_verify on the GPU (needs an MI355X): are sections 2 to 6 of a powers-of-tau file the powers of one (τ, α, β), and
sections 12 to 15 the transforms of 2 to 5?  Expected verdicts never come from the library: every file is written from lists of
discrete logarithms (tests/ptau_verify_model.py), whose exact truth — no randomness — gives (ok, kind, mask, fault); faulty points
are CONSTRUCTED and their expectation is stated here.  Every case goes through both the buffer and the _file entry.  The library's
randomised verdict can differ from the truth with probability < 2^-120: no case is skipped or retried.  The powers are 0, 1, 3, 7:
test_the_shapes_are_what_the_cases_need says why."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import groth16_dlog_model as M
import ptau_contribute_model as CM
import ptau_prepare_model as PM
import ptau_verify_model as VM

pytestmark = pytest.mark.gpu

R, Q = PM.R, PM.Q
SEED, SEED2 = bytes(range(32)), bytes([0x5A]) * 32
POWERS = [0, 1, 3, 7]
NONCANONICAL, OFF_CURVE, OFF_SUBGROUP = 1, 2, 3
MULT = 0x1234567
B = VM.bit


class World:
    def __init__(self, K, O, S):
        self.K, self.S = K, S
        self.fbm = lambda g, sc: K.generator_mul(g, sc)
        self.to_mont = lambda a: O.fq_convert_montgomery(a, True)
        self.toxic = S.toxic_waste()[:3]
        self.taus = {"random": self.toxic[0], "one": 1, "minus_one": R - 1, "omega3": PM.omega(3)}
        self._logs, self._image = {}, {}

    def logs(self, power, tau="random", prepared=True):
        """a fresh copy of the sound file's logarithms"""
        key = (power, tau, prepared)
        if key not in self._logs:
            self._logs[key] = VM.sound_logs(power, self.taus[tau], self.toxic[1], self.toxic[2], prepared)
        return {k: list(v) for k, v in self._logs[key].items()}

    def write(self, power, logs):
        return VM.write_file(power, logs, self.fbm, self.to_mont)

    def sound(self, power, tau="random", prepared=True):
        key = (power, tau, prepared)
        if key not in self._image:
            self._image[key] = self.write(power, self.logs(*key))
        return self._image[key]


@pytest.fixture(scope="module")
def world(gpu, O, S):
    return World(gpu, O, S)


def _devices(K):
    dev = K.Device()
    K.check(K.lib().icicle_get_active_device(C.byref(dev)), "get_active_device")
    hip = C.c_int(-1)
    C.CDLL("libamdhip64.so").hipGetDevice(C.byref(hip))
    return dev.type, dev.id, hip.value


def _verdict(K, image, tmp_path, seed=SEED):
    """(ok, kind, mask, fault) from the buffer entry, after the _file entry has said the same; fault = (section, element, point kind)"""
    out = []
    path = tmp_path / "case.ptau"
    path.write_bytes(image)
    for src in (image, str(path)):
        ok, rep = K.ptau_verify(src, seed=seed)
        point = rep.kind in (VM.POINT, VM.IDENTITY)
        assert rep.kind_name == VM.KIND_NAMES[rep.kind] and rep.failed == [VM.KIND_NAMES[k] for k in range(1, 12) if rep.failed_mask & B(k)]
        out.append((ok, rep.kind, rep.failed_mask, (rep.fault_section, rep.fault_index, rep.fault_kind) if point else None))
    assert out[0] == out[1]
    _verdict.report = rep
    return out[0]


def _expect(world, power, logs, tmp_path, bits=None):
    """the library on the file of `logs` against the exact truth; bits: what the specification's table lists for the case"""
    ok, kind, mask, fault = VM.truth(power, logs)
    if bits is not None:
        assert mask == bits and not ok
    want = (ok, kind, mask, fault + (0,) if fault else None)
    assert _verdict(world.K, world.write(power, logs), tmp_path) == want


def test_the_shapes_are_what_the_cases_need():
    """conditions, not measurements: the scalar kernels and the identity test run 256-lane workgroups of four waves, the G2 lane test
    64-lane ones; one lane per element"""
    assert 0 in POWERS and 1 in POWERS                                            # sections of 1, 2, 3 points; nothing to sum at power 0
    assert all((4 << p) - 1 < 64 for p in (0, 1, 3))                              # every section below one wave
    assert (1 << 7) == 2 * 64                                                     # power 7: two full 64-lane workgroups of the G2 test
    assert (2 << 7) - 1 == 255 and (4 << 7) - 1 == 511                            # … section 2's odd count a lane short of a 256-lane
    assert 255 // 256 == 0 and 511 // 256 == 1 and 511 % 256 == 255               # workgroup, section 12 two of them, the last a lane short
    assert all(((2 << p) - 1) % 2 == 1 for p in POWERS)                           # section 2's odd count 2N − 1: R's last base is the last point
    assert [CM.table_bits(p) for p in POWERS] == [1, 1, 2, 4]
    assert all((2 << p) - 2 >> CM.table_bits(p) >= 1 for p in (1, 3, 7))          # a table border inside section 2 from power 1 on
    assert [1 << (p + 1 - CM.table_bits(p)) for p in POWERS] == [1, 2, 4, 16]


@pytest.mark.parametrize("tau", ["random", "one", "minus_one", "omega3"])
@pytest.mark.parametrize("power", POWERS)
def test_sound_files(world, power, tau, tmp_path):
    K = world.K
    before = _devices(K)
    N = 1 << power
    for prepared in (False, True):
        logs = world.logs(power, tau, prepared)
        assert VM.truth(power, logs) == (True, 0, 0, None)
        image = world.sound(power, tau, prepared)
        assert _verdict(K, image, tmp_path) == (True, 0, 0, None)
        rep = _verdict.report
        assert (rep.power, rep.prepared, list(rep.points)) == (power, int(prepared), [2 * N - 1, N, N, N] + ([4 * N - 1] + [2 * N - 1] * 3 if prepared else [0] * 4))
        assert rep.device_ms > 0 and rep.upload_ms > 0 and rep.pairing_ms > 0
    if tau == "random":
        # the files are ptau_prepare_model's, byte for byte
        raw = PM.write_unprepared(power, *world.toxic, world.fbm, world.to_mont)
        assert world.sound(power, tau, False) == raw
        assert world.sound(power, tau, True) == PM.expected_prepared(raw, power, *world.toxic, world.fbm, world.to_mont)
    if tau == "one" and power >= 1:
        body = PM.payload(world.sound(power, tau, True), 12)                      # identities in section 12 are legitimate
        assert any(body[i * 64:(i + 1) * 64] == bytes(64) for i in range(len(body) // 64))
    assert _devices(K) == before


def test_two_seeds_and_the_operating_systems_agree(world, tmp_path):
    K = world.K
    good = world.sound(3)
    logs = world.logs(3)
    logs[14][9] = (logs[14][9] + 1) % R
    logs[2][5] = logs[2][5] * MULT % R
    bad = world.write(3, logs)
    want = VM.truth(3, logs)
    assert want == (False, VM.TAU_G1, B(VM.TAU_G1) | B(VM.LAGRANGE_12) | B(VM.LAGRANGE_14), None)    # (section 12 is section 2's transform)
    for seed in (SEED, SEED2, None):
        assert _verdict(K, good, tmp_path, seed) == (True, 0, 0, None)
        assert _verdict(K, bad, tmp_path, seed) == want


def test_a_ceremony_of_this_library_verifies(world, tmp_path):
    """ptau_new → two contributions with the operating system's secrets → verify → ptau_prepare → verify"""
    K = world.K
    i0 = K.ptau_new(4)
    i1, _ = K.ptau_contribute(i0, name="alice")
    i2, _ = K.ptau_contribute(i1, name="bob")
    assert K.ptau_contributions(i2)[0] is True
    assert _verdict(K, i0, tmp_path) == (True, 0, 0, None)                            # τ = α = β = 1
    assert _verdict(K, i2, tmp_path) == (True, 0, 0, None)
    prepared, _ = K.ptau_prepare(i2)
    assert _verdict(K, prepared, tmp_path, None) == (True, 0, 0, None)
    # a file whose record chain is valid and whose elements 0 and 1 are right, but whose element 9 is not: what every other tool accepts
    e = bytearray(i2)
    off = PM.sections(i2)[0][2][0]
    e[off + 9 * 64:off + 10 * 64] = e[off + 10 * 64:off + 11 * 64]
    assert K.ptau_contributions(bytes(e))[0] is True
    assert _verdict(K, bytes(e), tmp_path) == (False, VM.TAU_G1, B(VM.TAU_G1), None)


def test_faults_in_sections_2_to_6(world, tmp_path):
    power, N = 3, 8
    tau = world.toxic[0]

    def case(change, bits, prepared=False):
        logs = world.logs(power, prepared=prepared)
        change(logs)
        _expect(world, power, logs, tmp_path, bits)

    def times(s, k):
        def f(logs):
            logs[s][k] = logs[s][k] * MULT % R
        return f

    def whole(s):
        def f(logs):
            logs[s] = [v * MULT % R for v in logs[s]]
        return f

    def swap(logs):
        logs[2][3], logs[2][9] = logs[2][9], logs[2][3]

    def other_tau(logs):
        logs[4] = [world.toxic[1] * pow(tau + 1, i, R) % R for i in range(N)]

    for k in (2, N, 2 * N - 2):
        case(times(2, k), B(VM.TAU_G1))
    case(times(2, 1), B(VM.TAU_G1) | B(VM.TAU_PAIR))
    case(swap, B(VM.TAU_G1))
    case(times(3, 5), B(VM.TAU_G2))
    case(times(3, N - 1), B(VM.TAU_G2))
    case(other_tau, B(VM.ALPHA_TAU))
    case(whole(5), B(VM.BETA_PAIR))
    case(times(6, 0), B(VM.BETA_PAIR))
    case(whole(2), B(VM.GENERATORS) | B(VM.TAU_PAIR))
    case(times(5, 4), B(VM.BETA_TAU))
    # in a prepared file the transform of the faulty section fails with it: the truth says which
    case(times(4, 2), B(VM.ALPHA_TAU) | B(VM.LAGRANGE_14), prepared=True)
    # power 7: the last lane of section 2's workgroup, and the first of section 3's second
    for s, k, bits in ((2, 254, B(VM.TAU_G1)), (3, 64, B(VM.TAU_G2))):
        logs = world.logs(7, prepared=False)
        logs[s][k] = logs[s][k] * MULT % R
        _expect(world, 7, logs, tmp_path, bits)
    # power 1: three and two points
    logs = world.logs(1, prepared=False)
    logs[2][2] = logs[2][2] * MULT % R
    _expect(world, 1, logs, tmp_path, B(VM.TAU_G1))


@pytest.mark.parametrize("sid", [12, 13, 14, 15])
def test_one_wrong_element_of_a_prepared_section(world, sid, tmp_path):
    """another valid point in block 0, in block 1 (first and last j) and in the top block (first and last j): that LAGRANGE bit alone"""
    power = 3
    blocks = power + (2 if sid == 12 else 1)
    top = (1 << (blocks - 1)) - 1
    for e in (0, 1, 2, top, 2 * top):
        logs = world.logs(power)
        assert e < len(logs[sid]) == 2 * top + 1
        logs[sid][e] = (logs[sid][e] + 1) % R
        _expect(world, power, logs, tmp_path, B(VM.LAGRANGE_12 + sid - 12))


def test_cancelling_errors_and_the_untruncated_block(world, tmp_path):
    K, S = world.K, world.S
    power = 3
    # errors in blocks 1 and 2 of section 13 that equal multipliers would not see (tests/test_ptau_verify_model.py shows that)
    logs = world.logs(power)
    for e, err in VM.cancelling_errors(1, 1, 0x123456789ABCDEF).items():
        logs[13][e] = (logs[13][e] + err) % R
    _expect(world, power, logs, tmp_path, B(VM.LAGRANGE_13))
    # the synthesiser's file: section 12's last block is the untruncated L'_j(τ).  Documented: only the form prepare writes is accepted
    logs = world.logs(power)
    logs[12][15:] = S.lagrange_at(16, 4, world.toxic[0])
    full = S.write_ptau(power, world.fbm, points_to_mont=world.to_mont)
    assert world.write(power, logs) == full
    _expect(world, power, logs, tmp_path, B(VM.LAGRANGE_12))
    # power 7, the last element of section 12 — the last lane of its second workgroup
    logs = world.logs(7)
    logs[12][510] = (logs[12][510] + 1) % R
    _expect(world, 7, logs, tmp_path, B(VM.LAGRANGE_12))


def _bump(image, offset):
    """the 32-byte little-endian coordinate at `offset`, plus one"""
    e = bytearray(image)
    e[offset:offset + 32] = ((int.from_bytes(e[offset:offset + 32], "little") + 1) % (1 << 256)).to_bytes(32, "little")
    return bytes(e)


def test_faulty_points_are_a_verdict(world, tmp_path):
    K = world.K
    good = world.sound(3)
    off = {sid: o for sid, (o, _) in PM.sections(good)[0].items()}
    tw = b"".join((c * (1 << 256) % Q).to_bytes(32, "little") for c in M.twist_point_outside_subgroup())

    def put(image, offset, data):
        e = bytearray(image)
        e[offset:offset + len(data)] = data
        return bytes(e)

    def point(image, section, element, kind):
        assert _verdict(K, image, tmp_path) == (False, VM.POINT, 0, (section, element, kind))

    for sid in (3, 13):
        point(put(good, off[sid] + 6 * 128, tw), sid, 6, OFF_SUBGROUP)
        point(_bump(good, off[sid] + 4 * 128 + 64), sid, 4, OFF_CURVE)
        point(put(good, off[sid] + 2 * 128 + 32, Q.to_bytes(32, "little")), sid, 2, NONCANONICAL)
        point(_bump(_bump(good, off[sid] + 5 * 128), off[sid] + 1 * 128), sid, 1, OFF_CURVE)          # the lowest faulty element is named
    point(_bump(good, off[2] + 14 * 64 + 32), 2, 14, OFF_CURVE)
    point(_bump(good, off[12] + 30 * 64), 12, 30, OFF_CURVE)
    point(_bump(good, off[15] + 0 * 64), 15, 0, OFF_CURVE)
    point(put(good, off[6], tw), 6, 0, OFF_SUBGROUP)
    point(_bump(_bump(good, off[14] + 3 * 64), off[4] + 7 * 64), 4, 7, OFF_CURVE)                     # the source before its transform
    # an identity in sections 2 to 6 is a fault of its own, from the exact truth
    for s, k in ((2, 9), (6, 0), (3, 0), (5, 7)):
        logs = world.logs(3)
        logs[s][k] = 0
        assert VM.truth(3, logs) == (False, VM.IDENTITY, 0, (s, k))
        _expect(world, 3, logs, tmp_path)
    # … an identity in sections 12 to 15 is not: τ = 1 (test_sound_files), and here a lone one, which is merely wrong
    logs = world.logs(3)
    logs[13][4] = 0
    _expect(world, 3, logs, tmp_path, B(VM.LAGRANGE_13))
    assert _verdict(K, good, tmp_path) == (True, 0, 0, None)                                          # a following good call is as good as before


def test_containers(world, tmp_path):
    K = world.K
    good = world.sound(3)

    def refused(image, code, text):
        path = tmp_path / "bad.ptau"
        path.write_bytes(image)
        for src in (image, str(path)):
            with pytest.raises(K.ProverError, match=r"\(%d\)" % code) as e:
                K.ptau_verify(src, seed=SEED)
            assert text in str(e.value), str(e.value)

    refused(PM.without(good, {14}), -2, "3 of the sections 12 to 15 are present")
    refused(PM.without(good, {12, 13, 15}), -2, "1 of the sections 12 to 15 are present")
    refused(PM.with_payload(good, 13, PM.payload(good, 13)[:-128]), -2, "section 13 holds 1792 bytes, a file of power 3 has 1920")
    refused(PM.with_payload(good, 2, PM.payload(good, 2)[:-64]), -2, "section 2 holds 896 bytes, a file of power 3 has 960")
    refused(PM.without(good, {7}), -2, "")
    hdr = PM.sections(good)[0][1][0]
    e = bytearray(good)
    e[hdr + 36:hdr + 40] = (28).to_bytes(4, "little")
    refused(bytes(e), -3, "power 28 is above 27")
    refused(good[:-1], -2, "")
    with pytest.raises(K.ProverError, match=r"\(-1\).*cannot open"):
        K.ptau_verify(tmp_path / "missing.ptau")
    with pytest.raises(K.ProverError, match=r"\(-3\).*does not name one HIP device"):
        K.ptau_verify(good, device="HIP:0-1")
    # the other readers are what they were: the unprepared reader refuses the prepared file with its own text
    with pytest.raises(K.ProverError, match=r"\(-2\).*section 12 is present: the file is already prepared for phase 2"):
        K.ptau_prepare(good)


def test_the_process_is_as_it_was(world, O, tmp_path):
    """device and NTT domain untouched; ptau_info, ptau_prepare and a prove pass afterwards in the same process"""
    K, S = world.K, world.S
    before = _devices(K)
    n = 16
    K.release_domain()
    K.initialize_domain(K.get_root_of_unity(n))
    x = np.arange(4 * n, dtype=np.uint64).reshape(n, 4) + 7
    want = O.fr_ntt(x, True, batch=1)
    assert np.array_equal(K.ntt(x, True, batch_size=1), want)
    assert _verdict(K, world.sound(7), tmp_path) == (True, 0, 0, None)
    assert np.array_equal(K.ntt(x, True, batch_size=1), want)                    # the domain of size 16 is still the domain
    K.release_domain()
    assert _devices(K) == before
    assert K.ptau_info(world.sound(3), domain_power=3).power == 3
    assert K.ptau_prepare(world.sound(3, prepared=False))[0] == world.sound(3)
    r1, w = S.squaring_chain(7)
    zkey, vk = S.setup(r1, world.fbm, points_to_mont=world.to_mont)
    cm = K.CacheManager()
    try:
        cm.load("after-ptau-verify", zkey)
        pj, qj, _ = cm.prove_mem("after-ptau-verify", S.write_wtns(w), 3, 5)
        assert json.loads(qj) == [str(v) for v in w[1:1 + r1.n_public]]
        assert K.groth16_verify_json(pj, qj, S.vk_to_json(vk)) is True
    finally:
        cm.close()
    assert _devices(K) == before


def test_repl(world, tmp_path):
    K = world.K
    i0 = K.ptau_new(3)
    i1, _ = K.ptau_contribute(i0, name="alice")
    good, bad, point, prepared = tmp_path / "good.ptau", tmp_path / "bad.ptau", tmp_path / "point.ptau", tmp_path / "prepared.ptau"
    good.write_bytes(i1)
    off = PM.sections(i1)[0]
    e = bytearray(i1)
    e[off[2][0] + 5 * 64:off[2][0] + 6 * 64] = e[off[2][0] + 6 * 64:off[2][0] + 7 * 64]
    bad.write_bytes(bytes(e))
    point.write_bytes(_bump(i1, off[3][0] + 6 * 128))
    prepared.write_bytes(K.ptau_prepare(i1)[0])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmds = "".join(f"ptau-verify --ptau {p} --device HIP\n" for p in (good, bad, point, prepared)) + f"ptau-verify --ptau {tmp_path}/missing.ptau\nnonsense\nexit\n"
    run = subprocess.run([os.path.join(root, "icicle-snark_amd", "lib", "prove")], input=cmds, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lines = [ln.replace("> ", "") for ln in run.stdout.splitlines()]
    done = [i for i, ln in enumerate(lines) if ln == "COMMAND_COMPLETED"]
    first = lines[:done[0]]
    assert first[0] == "contributions: the chain holds, 1 records"
    assert first[1] == "power 3, sections 2 to 6 are the powers of one (tau, alpha, beta): yes" and first[2].startswith("upload ") and first[3] == "PTAU_OK"
    second = lines[done[0] + 1:done[1]]
    assert second[1].endswith("NO: TAU_G1") and second[-1] == "PTAU_BAD TAU_G1"
    third = lines[done[1] + 1:done[2]]
    assert third[1].endswith("not decided") and third[-1] == "PTAU_BAD POINT 3 6"
    fourth = lines[done[2] + 1:done[3]]
    assert fourth[0].startswith("contributions: not audited") and fourth[2] == "sections 12 to 15 are the transforms of 2 to 5: yes" and fourth[-1] == "PTAU_OK"
    assert lines[done[3] + 1:done[4]] == [] and "ptau-verify failed (-1)" in run.stderr
    assert "ptau-verify --ptau <file> [--device HIP]" in run.stdout
