"""groth16_witness_check on the GPU (needs an MI355X): does a witness satisfy an .r1cs?  One circuit serves the module —
random_circuit(150, 2, 10, seed=11): 163 wires, so the constraints cross two wave boundaries and end mid-wave — plus three
constraints added by hand: an all-empty one, one with a 40-term A and one that names a wire twice.  Every fault is CONSTRUCTED, and
the expected kind, index and count always come from a small Python-integer model over the R1CS lists, never from the library."""
import copy
import json
import struct

import pytest

pytestmark = pytest.mark.gpu

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
NONCANONICAL, ONE, CONSTRAINT = 1, 2, 3
FIRST_OUT = 13          # 1 + 2 publics + 10 inputs: constraint j of the random circuit defines wire 13 + j


def model(r, w):
    """(kind, index, noncanonical, failed) by integers.  failed is counted only over canonical values, like the library's."""
    bad = [i for i, v in enumerate(w) if v >= R]
    if bad:
        return NONCANONICAL, bad[0], len(bad), 0
    rows = [[0, 0, 0] for _ in range(r.n_constraints)]
    for k, mat in enumerate((r.A, r.B, r.C)):
        for (j, i, v) in mat:
            rows[j][k] = (rows[j][k] + v * w[i]) % R
    failing = [j for j, (a, b, c) in enumerate(rows) if a * b % R != c]
    if w[0] != 1:
        return ONE, 0, 0, len(failing)
    return (CONSTRAINT, failing[0], 0, len(failing)) if failing else (0, 0, 0, 0)


def failing_set(r, w):
    rows = [[0, 0, 0] for _ in range(r.n_constraints)]
    for k, mat in enumerate((r.A, r.B, r.C)):
        for (j, i, v) in mat:
            rows[j][k] = (rows[j][k] + v * w[i]) % R
    return [j for j, (a, b, c) in enumerate(rows) if a * b % R != c]


class Circuit:
    def __init__(self, K, S):
        r, w = S.random_circuit(150, 2, 10, seed=11)
        self.base_constraints = r.n_constraints
        # by hand: constraint 150 all empty (0·0 = 0); 151 a 40-term A times the constant wire, its value as C's coefficient of the
        # constant wire; 152 names wire 5 twice in A (2·w₅ + 3·w₅)
        self.long_wires = list(range(20, 60))
        long_a = [(151, i, 1000 + 7 * k) for k, i in enumerate(self.long_wires)]
        r.A += long_a
        r.B.append((151, 0, 1))
        r.C.append((151, 0, sum(v * w[i] for _, i, v in long_a) % R))
        r.A += [(152, 5, 2), (152, 5, 3)]
        r.B.append((152, 0, 1))
        r.C.append((152, 0, 5 * w[5] % R))
        r.n_constraints = 153
        self.r, self.w, self.S = r, w, S
        self.image = S.write_r1cs(r)
        self.h = K.R1cs(self.image)

    def wtns(self, w):
        return self.S.write_wtns([v % (1 << 256) for v in w])


@pytest.fixture(scope="module")
def cir(gpu, S):
    c = Circuit(gpu, S)
    yield c
    c.h.close()


def _expect(cir, w):
    """the library's verdict on w is the model's, exactly"""
    ok, rep = cir.h.check(cir.wtns(w))
    want = model(cir.r, w)
    assert (rep.kind, rep.index, rep.noncanonical, rep.failed) == want, ((rep.kind, rep.index, rep.noncanonical, rep.failed), want)
    assert ok == (want[0] == 0)
    return rep


def test_the_circuit_has_the_shape_the_cases_need(cir):
    """conditions on the inputs, checked against the synthesiser — not measurements"""
    r = cir.r
    assert (r.n_vars, r.n_public, cir.base_constraints, r.n_constraints) == (163, 2, 150, 153)
    assert 128 < r.n_constraints < 192                     # two wave boundaries crossed, the last wave partly filled
    for j in range(150):
        assert (j, FIRST_OUT + j, 1) in r.C
    count = lambda mat, j: sum(1 for t in mat if t[0] == j)
    assert [count(m, 150) for m in (r.A, r.B, r.C)] == [0, 0, 0]
    assert count(r.A, 151) == 40 and count(r.B, 151) == 1
    assert [t[1] for t in r.A if t[0] == 152] == [5, 5]
    assert {count(r.A, j) for j in range(150)} >= {1, 3} and {count(r.B, j) for j in range(150)} >= {1, 2}   # uneven rows
    i = cir.h.info
    assert (i.n_wires, i.n_public, i.n_constraints, i.n_terms) == (163, 2, 153, len(r.A) + len(r.B) + len(r.C))
    assert i.device_bytes >= 36 * i.n_terms + 32 * 163 and i.device_ms > 0 and i.upload_ms > 0
    assert model(r, cir.w) == (0, 0, 0, 0)


def test_sound_witness(cir, tmp_path):
    rep = _expect(cir, cir.w)
    assert rep.kind == 0 and rep.failed == 0 and rep.upload_ms > 0 and rep.device_ms > 0
    p = tmp_path / "witness.wtns"
    p.write_bytes(cir.wtns(cir.w))
    for ok, again in (cir.h.check(str(p)), cir.h.check(p), cir.h.check(cir.wtns(cir.w))):
        assert ok is True and (again.kind, again.index, again.noncanonical, again.failed) == (0, 0, 0, 0)


@pytest.mark.parametrize("j", [0, 63, 64, 127, 128, 149])
def test_one_wire_off_by_one(cir, j):
    w = list(cir.w)
    w[FIRST_OUT + j] = (w[FIRST_OUT + j] + 1) % R
    fs = failing_set(cir.r, w)
    assert j in fs and fs[0] == min(fs)          # j itself, and whichever constraints read that wire
    rep = _expect(cir, w)
    assert rep.kind == CONSTRAINT and rep.index == fs[0] and rep.failed == len(fs)
    _expect(cir, cir.w)                           # the handle is as good as before


def test_two_faults_at_once(cir):
    w = list(cir.w)
    for j in (128, 63):
        w[FIRST_OUT + j] = (w[FIRST_OUT + j] + 1) % R
    fs = failing_set(cir.r, w)
    assert {63, 128} <= set(fs)
    rep = _expect(cir, w)
    assert rep.index == fs[0] <= 63 and rep.failed == len(fs) >= 2


def test_every_wire_changed_counts_every_constraint(cir):
    """hundreds of lanes on the two tally addresses: the count must be complete"""
    w = [v if i < FIRST_OUT else (v + 1 + i) % R for i, v in enumerate(cir.w)]
    fs = failing_set(cir.r, w)
    assert len(fs) >= 140 and 150 not in fs       # (the all-empty constraint cannot fail)
    rep = _expect(cir, w)
    assert rep.failed == len(fs) and rep.index == fs[0]


def test_hand_made_constraints_fail_when_their_wires_change(cir):
    # a wire only the 40-term row's tail reads … is also read by others; the model says which — what matters: 151 is among them
    w = list(cir.w)
    w[cir.long_wires[-1]] = (w[cir.long_wires[-1]] + 1) % R
    assert 151 in failing_set(cir.r, w)
    _expect(cir, w)
    w = list(cir.w)
    w[5] = (w[5] + 1) % R
    assert 152 in failing_set(cir.r, w)
    _expect(cir, w)


def test_wire_zero_must_be_one(cir):
    w = list(cir.w)
    w[0] = 2
    rep = _expect(cir, w)
    assert rep.kind == ONE and rep.index == 0


def test_noncanonical_values_stop_the_constraint_kernel(cir):
    w = list(cir.w)
    w[5], w[162] = R, (1 << 256) - 1
    assert failing_set(cir.r, [v % R for v in w])  # the values reduced would violate constraints: a kernel that ran would count them
    rep = _expect(cir, w)
    assert (rep.kind, rep.index, rep.noncanonical, rep.failed) == (NONCANONICAL, 5, 2, 0)
    w = list(cir.w)
    w[0] = R + 1                                   # wire 0 not canonical: kind 1 comes before kind 2
    rep = _expect(cir, w)
    assert (rep.kind, rep.index) == (NONCANONICAL, 0)


def test_witness_of_another_size_is_an_argument_error(gpu, cir):
    with pytest.raises(gpu.ProverError, match=r"\(-3\).*162 values.*163 wires"):
        cir.h.check(cir.wtns(cir.w[:162]))
    with pytest.raises(gpu.ProverError, match=r"\(-2\)"):
        cir.h.check(b"wtns" + struct.pack("<II", 2, 0))
    _expect(cir, cir.w)


def _term_offset(image, r, row, t):
    """byte offset in the file of term t (in list order) of row 3j + k"""
    n = struct.unpack_from("<I", image, 8)[0]
    pos = 12
    for _ in range(n):
        sid, ln = struct.unpack_from("<IQ", image, pos)
        if sid == 2:
            break
        pos += 12 + ln
    counts = [0] * (3 * r.n_constraints)
    for k, mat in enumerate((r.A, r.B, r.C)):
        for (j, _, _) in mat:
            counts[3 * j + k] += 1
    return pos + 12 + 36 * (sum(counts[:row]) + t) + 4 * (row + 1)


def test_bad_records_fail_the_load(gpu, S, cir):
    """a wire id of 163 or a coefficient of r anywhere: -2 at LOAD, naming the lowest constraint at fault, and no handle"""
    r = cir.r
    # constructed: wire id 163 in B of constraint 100 (its first term)
    image = bytearray(cir.image)
    off = _term_offset(image, r, 3 * 100 + 1, 0)
    assert struct.unpack_from("<I", image, off)[0] == next(i for (j, i, _) in r.B if j == 100)
    struct.pack_into("<I", image, off, 163)
    with pytest.raises(gpu.ProverError, match=r"\(-2\).*constraint 100, matrix B: a wire id"):
        gpu.R1cs(bytes(image))
    struct.pack_into("<I", image, off, 162)       # the largest wire id is fine
    gpu.R1cs(bytes(image)).close()
    # … and in C of constraint 37 as well: the lower constraint is named
    struct.pack_into("<I", image, off, 163)
    off2 = _term_offset(image, r, 3 * 37 + 2, 0)
    struct.pack_into("<I", image, off2, 0xFFFFFFFF)
    with pytest.raises(gpu.ProverError, match=r"\(-2\).*constraint 37, matrix C: a wire id"):
        gpu.R1cs(bytes(image))
    # constructed: coefficient = r in a term of the 40-term A (the last one whose wire is not 0 in the witness); r − 1 is fine,
    # and changes the row's value
    t = max(k for k, i in enumerate(cir.long_wires) if cir.w[i] != 0)
    image = bytearray(cir.image)
    off = _term_offset(image, r, 3 * 151, t)
    assert struct.unpack_from("<I", image, off)[0] == cir.long_wires[t]
    assert int.from_bytes(image[off + 4:off + 36], "little") == 1000 + 7 * t
    image[off + 4:off + 36] = R.to_bytes(32, "little")
    with pytest.raises(gpu.ProverError, match=r"\(-2\).*constraint 151, matrix A: a coefficient"):
        gpu.R1cs(bytes(image))
    image[off + 4:off + 36] = (R - 1).to_bytes(32, "little")
    with gpu.R1cs(bytes(image)) as h:
        r2 = copy.deepcopy(r)
        k = next(n for n, e in enumerate(r2.A) if e[0] == 151 and e[1] == cir.long_wires[t])
        r2.A[k] = (151, cir.long_wires[t], R - 1)
        want = model(r2, cir.w)
        assert want == (CONSTRAINT, 151, 0, 1)
        ok, rep = h.check(cir.wtns(cir.w))
        assert (rep.kind, rep.index, rep.noncanonical, rep.failed) == want and not ok
    # a one-wire circuit whose one wire id is out of range
    tiny = S.R1CS(n_vars=1, n_public=0, n_constraints=1, A=[(0, 1, 1)])
    with pytest.raises(gpu.ProverError, match=r"\(-2\).*constraint 0, matrix A: a wire id"):
        gpu.R1cs(S.write_r1cs(tiny))
    with pytest.raises(gpu.ProverError, match=r"\(-3\)"):
        gpu.R1cs(cir.image, device="HIP:0,1")
    _expect(cir, cir.w)


def test_empty_circuit_and_empty_rows(gpu, S):
    with gpu.R1cs(S.write_r1cs(S.R1CS(n_vars=3, n_public=1, n_constraints=0))) as h:
        ok, rep = h.check(S.write_wtns([1, 5, 7]))
        assert ok and rep.failed == 0
        ok, rep = h.check(S.write_wtns([2, 5, 7]))
        assert not ok and rep.kind == ONE
    with gpu.R1cs(S.write_r1cs(S.R1CS(n_vars=3, n_public=1, n_constraints=2))) as h:      # constraints without any term
        ok, rep = h.check(S.write_wtns([1, 5, 7]))
        assert ok and rep.failed == 0


def test_a_refused_witness_proves_to_a_rejected_proof(gpu, O, S, cir):
    """the motivation as a test: the prover takes A∘B for the third QAP row, so it proves an unsatisfying witness without a word
    — and the proof fails verification.  The check says so beforehand, and says where."""
    zkey, vk = S.setup(cir.r, lambda g, sc: gpu.generator_mul(g, sc), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
    vk_json = S.vk_to_json(vk)
    bad = list(cir.w)
    bad[FIRST_OUT + 64] = (bad[FIRST_OUT + 64] + 1) % R
    cm = gpu.CacheManager()
    try:
        cm.load("wc", zkey)
        for w, want in ((cir.w, True), (bad, False)):
            wtns = cir.wtns(w)
            ok, rep = cir.h.check(wtns)
            assert ok is want
            pj, qj, _ = cm.prove_mem("wc", wtns, 3, 5)
            assert json.loads(qj) == [str(w[1]), str(w[2])]
            assert gpu.groth16_verify_json(pj, qj, vk_json) is want
    finally:
        cm.close()
        gpu.release_domain()
