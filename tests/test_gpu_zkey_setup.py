"""groth16_setup on the GPU (needs an MI355X): the proving key of a loaded circuit made directly from toxic waste (τ, α, β, γ, δ).
The expected key is the synthesiser's: setup(r, fbm, …, toxic=T) with `fbm` the CPU ORACLE's fixed-base multiplication on the
generators — the expectation shares no kernel with the code under test, and affine points are canonical, so the comparison is of
bytes.  The circuits are tests/zkey_new_circuits.py's, at most 300 constraints each; every faulty input is CONSTRUCTED."""
import ctypes as C
import json
import os
import subprocess

import pytest

import zkey_new_circuits as ZC

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))
ALL = ["mixed", "fan", "chain6", "chain7", "tiny"]
OTHER_SECTIONS = [1, 2, 3, 5, 6, 7, 8, 9, 10]
TOXICS = ["drawn", "unit"]


class World:
    def __init__(self, K, O, S):
        self.K, self.S = K, S
        gen = {g: O.ec_to_affine(g, O.ec_generator(g)) for g in ("g1", "g2")}
        self.fbm = lambda g, sc: O.fixed_base_mul(g, gen[g], sc)             # the CPU oracle's: tests/test_ptau_prepare_model.py: fbm
        self.to_mont = lambda a: O.fq_convert_montgomery(a, True)
        T = S.toxic_waste()
        self.toxic = {"drawn": T, "unit": T[:3] + (1, 1)}
        self.circuits = ZC.circuits(S)
        self.want = {(n, t): S.setup(r, self.fbm, self.to_mont, toxic=self.toxic[t])[0] for n, r in self.circuits.items() for t in TOXICS}
        self.handles = {n: K.R1cs(S.write_r1cs(r)) for n, r in self.circuits.items()}
        self.domain = {n: S.key_scalars(r)["n"] for n, r in self.circuits.items()}
        # ceremony files of the same τ, α, β, for the judges (inputs, not expectations: the library's own multiplication makes them)
        lib_fbm = lambda g, sc: K.generator_mul(g, sc)
        self.ptau = {p: S.write_ptau(p, lib_fbm, points_to_mont=self.to_mont) for p in (8, 10)}

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


def _same_key(world, name, toxic, got, rep=None):
    want, r = world.want[(name, toxic)], world.circuits[name]
    assert ZC.sections(got)[1] == list(range(1, 11)) and got[:12] == want[:12]
    for sid in OTHER_SECTIONS:
        assert ZC.payload(got, sid) == ZC.payload(want, sid), (name, toxic, sid)
    recs = ZC.records(got)
    assert sorted(recs) == sorted(ZC.records(want))
    assert recs == ZC.stated_records(r), name                       # zkey-new's stated order: by constraint, A then B, then the binding rows
    assert len(got) == len(want)
    if rep is not None:
        assert (rep.n_vars, rep.n_public, rep.domain, rep.n_coeffs, rep.zkey_bytes) == (r.n_vars, r.n_public, world.domain[name], len(recs), len(want))
        longest = max(sum(1 for t in mat if t[1] == s) + (1 if k == 0 and s <= r.n_public else 0) for k, mat in enumerate((r.A, r.B, r.C)) for s in range(r.n_vars))
        assert rep.longest_column == longest and rep.device_ms > 0 and rep.upload_ms > 0 and rep.download_ms > 0
        assert rep.lagrange_ms > 0 and rep.columns_ms > 0 and rep.g1_ms > 0 and rep.g2_ms > 0


def test_the_inputs_have_the_shape_the_cases_need(world, S):
    """conditions, checked against the synthesiser — not measurements"""
    want = world.want[("mixed", "drawn")]
    for sid, size in ((5, 64), (6, 64), (7, 128)):                   # a wire in no matrix is all-zero bytes in every section
        assert ZC.payload(want, sid)[165 * size:166 * size] == bytes(size)
    assert ZC.payload(want, 8)[(165 - 3) * 64:(166 - 3) * 64] == bytes(64)
    assert ZC.payload(want, 5)[164 * 64:165 * 64] == bytes(64) and ZC.payload(want, 5)[163 * 64:164 * 64] != bytes(64)    # the cancelling wire
    assert ZC.sections(world.want[("tiny", "drawn")])[0][8][1] == 0  # an empty section 8
    assert world.powers("fan") == [10] and all(world.powers(n) == [8, 10] for n in ALL if n != "fan")
    # γ, δ ≠ 1 move the header and sections 3, 8, 9, and nothing else
    unit = world.want[("mixed", "unit")]
    assert all((ZC.payload(want, s) == ZC.payload(unit, s)) == (s not in (2, 3, 8, 9)) for s in range(1, 11))
    assert all(world.K.setup_toxic_check(world.toxic[t], 9) == 0 for t in TOXICS)


@pytest.mark.parametrize("toxic", TOXICS)
@pytest.mark.parametrize("name", ALL)
def test_the_key_is_the_synthesisers_byte_for_byte(world, name, toxic, tmp_path):
    h = world.handles[name]
    before = _devices(world.K)
    got, rep = h.setup(toxic=world.toxic[toxic])
    _same_key(world, name, toxic, got, rep)
    out = tmp_path / "out.zkey"
    none, rep = h.setup(out=out, toxic=world.toxic[toxic])
    assert none is None and rep.write_ms > 0
    _same_key(world, name, toxic, out.read_bytes(), rep)
    assert os.listdir(tmp_path) == ["out.zkey"]
    assert _devices(world.K) == before
    assert world.K.zkey_new_size(world.S.write_r1cs(world.circuits[name])) == (len(got), len(ZC.records(got)))


@pytest.mark.parametrize("name", ["fan", "mixed"])
def test_heavy_column_threshold_does_not_change_a_byte(world, name):
    h = world.handles[name]
    reps = {}
    for thr in (0, 8, 64, 1 << 30):
        got, reps[thr] = h.setup(toxic=world.toxic["drawn"], heavy_column_terms=thr)
        _same_key(world, name, "drawn", got, reps[thr])
    assert reps[8].heavy_columns > 0 and reps[8].heavy_items >= 2 * reps[8].heavy_columns
    assert (reps[1 << 30].heavy_columns, reps[1 << 30].heavy_items) == (0, 0)
    assert (reps[0].heavy_columns, reps[0].heavy_items) == (reps[64].heavy_columns, reps[64].heavy_items)   # the default is 64
    if name == "fan":                                                # columns of 300 and 301 terms: cut at 64 as well
        assert reps[64].heavy_columns > 0 and reps[64].heavy_items > reps[64].heavy_columns


@pytest.mark.parametrize("name", ALL)
def test_with_unit_gamma_and_delta_it_is_zkey_news_key(world, name):
    h = world.handles[name]
    got, _ = h.setup(toxic=world.toxic["unit"])
    for p in world.powers(name):
        assert got == h.new_zkey(world.ptau[p])[0], (name, p)


@pytest.mark.parametrize("name", ALL)
def test_the_librarys_own_judges_accept_the_key(world, name):
    K, h = world.K, world.handles[name]
    key, _ = h.setup(toxic=world.toxic["drawn"])
    ok, rep = K.zkey_check(key, seed=SEED)
    assert ok is True and rep.kind == 0
    ok, rep = h.match_zkey(key, seed=SEED)
    assert ok is True and rep.kind == 0
    for q in world.powers(name):                                     # the ceremony of the same τ, α, β; the key's γ and δ are not 1
        ok, rep = h.verify_zkey(key, world.ptau[q], seed=SEED)
        assert ok is True and (rep.kind, rep.failed_mask) == (0, 0)
    ok, crep = K.zkey_contributions(key)                             # as for synth.setup's keys: δ ≠ 1 with no record
    assert ok is False and crep.count == 0
    key2, crep = K.zkey_contribute(key, secret=SEED, name="after setup")
    assert key2 != key and K.zkey_check(key2, seed=SEED)[0] is True
    ok, rep = h.verify_zkey(key2, world.ptau[world.powers(name)[-1]], seed=SEED)
    assert ok is True and (rep.kind, rep.failed_mask) == (0, 0)


def _proves_and_verifies(K, S, key, r, w, tag):
    vk = K.zkey_export_vk(key)
    cm = K.CacheManager()
    try:
        cm.load(tag, key)
        pj, qj, _ = cm.prove_mem(tag, S.write_wtns(w), 3, 5)
        assert json.loads(qj) == [str(v) for v in w[1:1 + r.n_public]]
        assert K.groth16_verify_json(pj, qj, vk) is True
        bad = list(w)
        bad[r.n_vars - 1 if r.n_vars < 40 else 40] += 1              # CONSTRUCTED: one private wire off by one
        bad = [v % ZC.R for v in bad]
        assert not ZC.check_r1cs(r, bad)
        pj, qj, _ = cm.prove_mem(tag, S.write_wtns(bad), 3, 5)
        assert K.groth16_verify_json(pj, qj, vk) is False
    finally:
        cm.close()


def test_the_key_loads_proves_and_verifies(world, S):
    r, w = ZC.mixed(S)
    assert ZC.check_r1cs(r, w)
    key, _ = world.handles["mixed"].setup(toxic=world.toxic["drawn"])
    _proves_and_verifies(world.K, S, key, r, w, "setup")


def test_fresh_randomness(world, S):
    """toxic=None: the operating system's randomness — two keys differ, and each is a sound key of the circuit"""
    K, h = world.K, world.handles["chain7"]
    r, w = S.squaring_chain(7)
    assert ZC.check_r1cs(r, w)
    k1, rep1 = h.setup()
    k2, rep2 = h.setup()
    assert k1 != k2 and len(k1) == len(k2) == rep1.zkey_bytes == len(world.want[("chain7", "drawn")])
    assert all(ZC.payload(k1, s) != ZC.payload(k2, s) for s in (2, 3, 5, 6, 7, 8, 9)) and ZC.payload(k1, 4) == ZC.payload(k2, 4)
    for i, key in enumerate((k1, k2)):
        assert ZC.records(key) == ZC.stated_records(r)
        assert K.zkey_check(key, seed=SEED)[0] is True and h.match_zkey(key, seed=SEED)[0] is True
        _proves_and_verifies(K, S, key, r, w, f"fresh{i}")


def test_errors(world, S, tmp_path):
    K, h = world.K, world.handles["mixed"]
    before = _devices(K)
    T = world.toxic["drawn"]
    need = len(world.want[("mixed", "drawn")])
    w8 = S.omega(8)
    names = ["tau", "alpha", "beta", "gamma", "delta"]
    faults = [(T[:i] + (0,) + T[i + 1:], rf"\(-2\).*toxic waste: {names[i]} is zero") for i in range(5)]
    faults += [(T[:i] + (S.R_MOD,) + T[i + 1:], rf"\(-2\).*toxic waste: {names[i]} is not below r") for i in range(5)]
    faults += [((tau,) + T[1:], r"\(-2\).*toxic waste: tau lies in the domain of order 2\^8 or in its coset")
               for tau in (pow(w8, 3, S.R_MOD), S.omega(9) * pow(w8, 3, S.R_MOD) % S.R_MOD, 1)]
    for toxic, match in faults:
        assert K.setup_toxic_check(toxic, 8) != 0
        with pytest.raises(K.ProverError, match=match):
            h.setup(toxic=toxic)
        with pytest.raises(K.ProverError, match=match):
            h.setup(out=tmp_path / "never.zkey", toxic=toxic)
        assert os.listdir(tmp_path) == []                            # neither the key nor a temporary
        # the buffer entry with room: −2, and the caller's buffer untouched
        opt, rep = K.SetupOptions(0), K.SetupReport()
        buf = C.create_string_buffer(b"\xa5" * need, need)
        rc = K.lib().groth16_setup(h._h, K.toxic160(toxic), buf, C.c_size_t(need), C.byref(opt), C.byref(rep))
        assert rc == -2 and buf.raw == b"\xa5" * need
    # cap one byte short: −3, and the report still says what is needed
    opt, rep = K.SetupOptions(0), K.SetupReport()
    buf = C.create_string_buffer(need)
    rc = K.lib().groth16_setup(h._h, K.toxic160(T), buf, C.c_size_t(need - 1), C.byref(opt), C.byref(rep))
    assert rc == -3 and rep.zkey_bytes == need and rep.n_coeffs == len(ZC.records(world.want[("mixed", "drawn")]))
    assert buf.raw == bytes(need)                                    # nothing was written
    K.lib().groth16_last_error.restype = C.c_char_p
    assert b"needs %d bytes" % need in K.lib().groth16_last_error()
    rc = K.lib().groth16_setup(h._h, K.toxic160(T), buf, C.c_size_t(need), C.byref(opt), C.byref(rep))
    assert rc == 0
    _same_key(world, "mixed", "drawn", buf.raw, rep)
    # a null handle, a null report
    assert K.lib().groth16_setup(None, K.toxic160(T), buf, C.c_size_t(need), C.byref(opt), C.byref(rep)) == -3
    assert K.lib().groth16_setup_file(None, K.toxic160(T), os.fsencode(tmp_path / "never.zkey"), C.byref(opt), C.byref(rep)) == -3
    assert K.lib().groth16_setup(h._h, K.toxic160(T), buf, C.c_size_t(need), C.byref(opt), None) == -3
    with pytest.raises(K.ProverError, match=r"\(-1\).*cannot create"):
        h.setup(out=tmp_path / "no_such_dir" / "out.zkey", toxic=T)
    assert os.listdir(tmp_path) == []
    assert _devices(K) == before
    # the handle is as good as before
    assert h.match_zkey(world.want[("mixed", "drawn")], seed=SEED)[0] is True


def test_the_repl_writes_a_sound_key(world, S, tmp_path):
    K = world.K
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r, w = S.squaring_chain(7)
    (tmp_path / "c.r1cs").write_bytes(S.write_r1cs(r))
    cmds = (f"zkey-setup --r1cs {tmp_path}/c.r1cs --zkey {tmp_path}/out.zkey --vk {tmp_path}/vk.json --device HIP\n"
            f"zkey-setup --r1cs {tmp_path}/missing.r1cs --zkey {tmp_path}/never.zkey\nnonsense\nexit\n")
    out = subprocess.run([os.path.join(root, "icicle-snark_amd", "lib", "prove")], input=cmds, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [ln.replace("> ", "") for ln in out.stdout.splitlines()]
    assert lines[0].startswith("wires 9 public 1 domain 16 coefficients 16 bytes %d longest column " % len(world.want[("chain7", "drawn")]))
    assert lines[1].startswith("single-party key: whoever ran this command can forge proofs")
    assert lines[2:6] == ["ZKEY_WRITTEN", "VK_WRITTEN", "COMMAND_COMPLETED", "COMMAND_COMPLETED"] and "zkey-setup failed (-1)" in out.stderr
    assert "zkey-setup --r1cs <file> --zkey <file> [--vk <file>] [--device HIP]" in out.stdout
    assert not (tmp_path / "never.zkey").exists()
    key = (tmp_path / "out.zkey").read_bytes()
    assert (tmp_path / "vk.json").read_text() == K.zkey_export_vk(key)
    assert ZC.records(key) == ZC.stated_records(r)
    assert K.zkey_check(key, seed=SEED)[0] is True and world.handles["chain7"].match_zkey(key, seed=SEED)[0] is True
    _proves_and_verifies(K, S, key, r, w, "repl")
