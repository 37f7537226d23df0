"""groth16_r1cs_match_zkey on the GPU (needs an MI355X): does a proving key's section 4 carry the A and B of an .r1cs?  The circuit
and its key are test_gpu_witness_check's (163 wires, 153 constraints, domain 256).  Every edit of section 4 is CONSTRUCTED, and the
expected kind, index and counts come from a Python-integer model that compares the two files entry by entry."""
import hashlib
import struct

import pytest

from test_gpu_witness_check import Circuit, R

pytestmark = pytest.mark.gpu

SIZES, ROW_A, ROW_B = 1, 2, 3
SEEDS = [hashlib.sha256(b"r1cs-match %d" % k).digest() for k in range(8)]
R2_INV = pow(pow(2, 512, R), -1, R)
R2 = pow(2, 512, R)


def _sections(z):
    n = struct.unpack_from("<I", z, 8)[0]
    pos, out = 12, []
    for _ in range(n):
        sid, ln = struct.unpack_from("<IQ", z, pos)
        out.append((sid, pos + 12, ln))
        pos += 12 + ln
    return out


def records(zkey):
    """section 4 as [(matrix, row, wire, value·R² as stored)]"""
    off, ln = next((o, l) for s, o, l in _sections(zkey) if s == 4)
    n = (ln - 4) // 44
    return [struct.unpack_from("<III", zkey, off + 4 + 44 * k) + (int.from_bytes(zkey[off + 16 + 44 * k:off + 48 + 44 * k], "little"),) for k in range(n)]


def with_records(zkey, recs):
    """the key with section 4 replaced"""
    body = struct.pack("<I", len(recs)) + b"".join(struct.pack("<III", m, c, s) + int(v).to_bytes(32, "little") for m, c, s, v in recs)
    out = bytes(zkey[:12])
    for sid, off, ln in _sections(zkey):
        payload = body if sid == 4 else zkey[off:off + ln]
        out += struct.pack("<IQ", sid, len(payload)) + payload
    return out


def model(r, recs, domain=256):
    """(kind, index, rows_a, rows_b): the key's rows against the circuit's, entry by entry"""
    want = [dict(), dict()]
    for k, mat in enumerate((r.A, r.B)):
        for (j, i, v) in mat:
            want[k][(j, i)] = (want[k].get((j, i), 0) + v) % R
    for s in range(r.n_public + 1):
        want[0][(r.n_constraints + s, s)] = 1
    got = [dict(), dict()]
    for m, c, s, v in recs:
        got[m][(c, s)] = (got[m].get((c, s), 0) + v * R2_INV) % R
    diff = []
    for k in range(2):
        keys = set(want[k]) | set(got[k])
        diff.append(sorted({c for (c, s) in keys if want[k].get((c, s), 0) != got[k].get((c, s), 0)}))
    if diff[0]:
        return ROW_A, diff[0][0], len(diff[0]), len(diff[1])
    if diff[1]:
        return ROW_B, diff[1][0], len(diff[0]), len(diff[1])
    return 0, 0, 0, 0


class Key:
    def __init__(self, K, O, S):
        self.cir = Circuit(K, S)
        self.zkey, _ = S.setup(self.cir.r, lambda g, sc: K.generator_mul(g, sc), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
        self.recs = records(self.zkey)


@pytest.fixture(scope="module")
def key(gpu, O, S):
    k = Key(gpu, O, S)
    yield k
    k.cir.h.close()


def _expect(key, recs, seed=SEEDS[0]):
    ok, rep = key.cir.h.match_zkey(with_records(key.zkey, recs), seed=seed)
    want = model(key.cir.r, recs)
    assert (rep.kind, rep.index, rep.rows_a, rep.rows_b) == want, ((rep.kind, rep.index, rep.rows_a, rep.rows_b), want)
    assert ok == (want[0] == 0)
    return rep


def _find(key, pred):
    return next(k for k, rec in enumerate(key.recs) if pred(*rec))


def test_the_key_has_the_shape_the_cases_need(key):
    r = key.cir.r
    assert struct.unpack_from("<III", key.zkey, next(o for s, o, l in _sections(key.zkey) if s == 2) + 72) == (163, 2, 256)
    assert len(key.recs) == len(r.A) + len(r.B) + 3
    assert with_records(key.zkey, key.recs) == key.zkey
    assert model(r, key.recs) == (0, 0, 0, 0)
    assert [rec for rec in key.recs if rec[1] >= 153] == [(0, 153 + s, s, R2 % R) for s in range(3)]


def test_untouched_key_matches(key):
    for seed in SEEDS + [None]:
        ok, rep = key.cir.h.match_zkey(key.zkey, seed=seed)
        assert ok is True and (rep.kind, rep.index, rep.rows_a, rep.rows_b) == (0, 0, 0, 0) and rep.device_ms > 0
    # the witness check still works on the handle that has just held z in the witness's place
    ok, _ = key.cir.h.check(key.cir.wtns(key.cir.w))
    assert ok


def test_record_order_and_split_records_do_not_matter(key):
    assert _expect(key, key.recs[::-1]).kind == 0
    k = _find(key, lambda m, c, s, v: m == 0 and c == 40)
    m, c, s, v = key.recs[k]
    part = 12345 * R2 % R
    split = key.recs[:k] + [(m, c, s, (v - part) % R)] + key.recs[k + 1:] + [(m, c, s, part)]
    assert _expect(key, split).kind == 0


def test_value_plus_one_in_an_a_record(key):
    for c in (0, 63, 64, 151):
        k = _find(key, lambda m, cc, s, v: m == 0 and cc == c)
        recs = list(key.recs)
        m, cc, s, v = recs[k]
        recs[k] = (m, cc, s, (v + R2) % R)           # coefficient + 1
        rep = _expect(key, recs)
        assert (rep.kind, rep.index, rep.rows_a, rep.rows_b) == (ROW_A, c, 1, 0)
        recs[k] = (m, cc, s, (v + 1) % R)            # the stored residue + 1
        assert _expect(key, recs).index == c


def test_wire_changed_in_a_b_record(key):
    k = _find(key, lambda m, c, s, v: m == 1 and c == 129)
    recs = list(key.recs)
    m, c, s, v = recs[k]
    recs[k] = (m, c, (s + 1) % 163, v)
    rep = _expect(key, recs)
    assert (rep.kind, rep.index, rep.rows_a, rep.rows_b) == (ROW_B, 129, 0, 1)


def test_matrix_byte_flipped(key):
    k = _find(key, lambda m, c, s, v: m == 0 and c == 77)
    recs = list(key.recs)
    m, c, s, v = recs[k]
    recs[k] = (1, c, s, v)
    rep = _expect(key, recs)
    assert (rep.kind, rep.index, rep.rows_a, rep.rows_b) == (ROW_A, 77, 1, 1)


def test_public_binding_record_zeroed(key):
    k = _find(key, lambda m, c, s, v: m == 0 and c == 153 + 1 and s == 1)
    recs = list(key.recs)
    recs[k] = (0, 154, 1, 0)
    rep = _expect(key, recs)
    assert (rep.kind, rep.index, rep.rows_a, rep.rows_b) == (ROW_A, 150 + 3 + 1, 1, 0)
    # … and a record ABOVE the binding rows, where A must be 0
    rep = _expect(key, key.recs + [(0, 200, 7, R2 % R)])
    assert (rep.kind, rep.index, rep.rows_a, rep.rows_b) == (ROW_A, 200, 1, 0)
    rep = _expect(key, key.recs + [(1, 153, 0, R2 % R)])
    assert (rep.kind, rep.index, rep.rows_a, rep.rows_b) == (ROW_B, 153, 0, 1)


def test_values_swapped_across_rows(key):
    ka = _find(key, lambda m, c, s, v: m == 0 and c == 151)
    kb = next(k for k, (m, c, s, v) in enumerate(key.recs) if m == 0 and c < 150 and v != key.recs[ka][3])
    recs = list(key.recs)
    recs[ka], recs[kb] = recs[ka][:3] + (recs[kb][3],), recs[kb][:3] + (recs[ka][3],)
    rep = _expect(key, recs)
    assert (rep.kind, rep.index, rep.rows_a, rep.rows_b) == (ROW_A, min(recs[ka][1], recs[kb][1]), 2, 0)


def test_sizes(gpu, S, key):
    r = key.cir.r
    with gpu.R1cs(S.write_r1cs(r, n_pub_out=1, section_order=(2, 3, 1))) as h:
        ok, rep = h.match_zkey(key.zkey, seed=SEEDS[1])
        assert ok and rep.kind == 0
    other, _ = S.random_circuit(150, 3, 9, seed=11)
    assert other.n_vars == 163 and other.n_public == 3
    with gpu.R1cs(S.write_r1cs(other)) as h:
        ok, rep = h.match_zkey(key.zkey, seed=SEEDS[1])
        assert not ok and (rep.kind, rep.index, rep.rows_a, rep.rows_b) == (SIZES, 1, 0, 0)
    with gpu.R1cs(S.write_r1cs(S.squaring_chain(150)[0])) as h:
        ok, rep = h.match_zkey(key.zkey, seed=SEEDS[1])
        assert not ok and (rep.kind, rep.index) == (SIZES, 0)
    with gpu.R1cs(S.write_r1cs(S.R1CS(n_vars=163, n_public=2, n_constraints=300))) as h:
        ok, rep = h.match_zkey(key.zkey, seed=SEEDS[1])
        assert not ok and (rep.kind, rep.index) == (SIZES, 2)
    # a circuit of the same sizes but other matrices: rows differ
    same_size, _ = S.random_circuit(150, 2, 10, seed=12)
    same_size.n_constraints = 153
    with gpu.R1cs(S.write_r1cs(same_size)) as h:
        ok, rep = h.match_zkey(key.zkey, seed=SEEDS[1])
        want = model(same_size, key.recs)
        assert not ok and (rep.kind, rep.index, rep.rows_a, rep.rows_b) == want and want[2] > 100


def test_errors(gpu, key):
    with pytest.raises(gpu.ProverError, match=r"\(-2\)"):
        key.cir.h.match_zkey(key.zkey[:1000], seed=SEEDS[0])
    with pytest.raises(gpu.ProverError, match=r"\(-2\).*out of range"):
        key.cir.h.match_zkey(with_records(key.zkey, key.recs + [(0, 256, 0, 1)]), seed=SEEDS[0])
    with pytest.raises(ValueError):
        key.cir.h.match_zkey(key.zkey, seed=b"short")
    ok, _ = key.cir.h.match_zkey(key.zkey, seed=SEEDS[0])
    assert ok
