"""groth16_zkey_contributions — the host's audit of section 10 — against the Python model of tests/zkey_contribute_model.py.  The
keys are the synthesiser's (γ = 1, δ chosen here), section 10 is the MODEL's bytes, never the library's: chains of 0, 1, 2 and 3
records that must hold, and CONSTRUCTED faults, each with the kind and index stated here and by the model.  Host only: the call
initialises no GPU — this file runs, and passes, on a machine that has none."""
import struct

import pytest

import zkey_contribute_model as ZM
import zkey_new_circuits as ZC

R = ZM.R
SECRETS = [bytes([i]) * 32 for i in (1, 2, 3)]
NAMES = [b"alice", b"", b"carol \xc3\xa9"]


class World:
    def __init__(self, K, O, S):
        self.K, self.S = K, S
        G = {g: O.ec_to_affine(g, O.ec_generator(g)) for g in ("g1", "g2")}
        self.fbm = lambda g, sc: O.fixed_base_mul(g, G[g], sc)
        self.to_mont = lambda a: O.fq_convert_montgomery(a, True)
        self.toxic = S.toxic_waste()[:3]
        self.circuit = S.squaring_chain(7)[0]
        self.g1 = ZM.G1Bytes(O)
        self.dlog = {self.g1(1): 1, bytes(64): 0}
        self._keys = {}
        # the chain: key[i] after i contributions, its header's δ = d[i], its section 10 the model's
        self.d, self.keys, self.recs, self.trace = [1], [self.bare(1)], [], []
        for secret, name in zip(SECRETS, NAMES):
            prev, delta = self.keys[-1], ZM.delta_of(secret)
            rec, _, kcz = ZM.make_record(ZM.chain_hash(prev, self.recs, self.g1), self.g1(self.d[-1]), self.d[-1], secret, delta, name, self.g1)
            self.note(rec, self.d[-1], delta, kcz[0])
            self.trace.append((self.d[-1], delta) + kcz)
            self.recs.append(rec)
            self.d.append(self.d[-1] * delta % R)
            self.keys.append(ZM.with_section(self.bare(self.d[-1]), 10, ZM.join_records(self.recs)))

    def note(self, rec, d_before, delta, k):
        self.dlog[rec[:64]] = d_before * delta % R
        self.dlog[rec[64:128]] = k * d_before % R

    def bare(self, delta, circuit=None):
        """setup()'s key with γ = 1 and this δ; its section 10 holds a zero count"""
        key = (delta, id(circuit))
        if key not in self._keys:
            self._keys[key] = self.S.setup(circuit or self.circuit, self.fbm, points_to_mont=self.to_mont, toxic=self.toxic + (1, delta))[0]
        return self._keys[key]

    def audit(self, key):
        ok, rep = self.K.zkey_contributions(key)
        return (ok, rep.count, rep.kind, rep.index), rep


@pytest.fixture(scope="module")
def world(K, O, S):
    return World(K, O, S)


def test_the_model_is_a_schnorr_proof_in_the_exponent(world):
    """z·d = k·d + c·(d·δ′): the equation the audit checks on points, on their logarithms"""
    assert len(world.trace) == 3
    for d, delta, k, c, z in world.trace:
        assert 0 < delta < R and 0 < k < R and 0 < c < 1 << 128 and z == (k + c * delta) % R
        assert (z * d - k * d - c * (d * delta % R)) % R == 0
    assert len({t[1] for t in world.trace}) == 3 and len({t[2] for t in world.trace}) == 3
    assert ZM.delta_of(SECRETS[0]) == ZM.W(SECRETS[0] + b"icicle-snark zkey contribution v1")
    # the header is the synthesiser's: δ₁ = d·G₁, and h₀ does not move along the chain
    for i, key in enumerate(world.keys):
        assert ZC.payload(key, 2)[468:532] == world.g1(world.d[i]) and ZM.h0(key) == ZM.h0(world.keys[0])


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_a_chain_of_the_models_records_holds(world, n):
    key = world.keys[n]
    assert ZM.audit(key, world.dlog, world.g1) == (True, n, 0, 0)
    verdict, rep = world.audit(key)
    assert verdict == (True, n, 0, 0)
    assert rep.records == [(rec[:64], name) for rec, name in zip(world.recs[:n], NAMES)]
    if n == 0:                                                      # without section 10: zero records as well
        secs, order = ZC.sections(key)
        bare = key[:8] + struct.pack("<I", 9) + b"".join(key[secs[s][0] - 12:secs[s][0] + secs[s][1]] for s in order if s != 10)
        assert 10 not in ZC.sections(bare)[0] and world.audit(bare)[0] == (True, 0, 0, 0)


def _flip(b, byte, bit=0):
    e = bytearray(b)
    e[byte] ^= 1 << bit
    return bytes(e)


def _cases(w):
    """name → (key, delta2_matches, the verdict stated here)"""
    k3, recs = w.keys[3], w.recs
    sec = lambda rs: ZM.join_records(rs)
    put = lambda key, payload: ZM.with_section(key, 10, payload)
    out = {}
    out["one bit of z, record 2"] = (put(k3, sec([recs[0], _flip(recs[1], 128 + 7, 3), recs[2]])), True, (ZM.POK, 2))
    out["one bit of a name, record 1"] = (put(k3, sec([_flip(recs[0], 164 + 2), recs[1], recs[2]])), True, (ZM.POK, 1))
    swapped = recs[2][64:128] + recs[2][:64] + recs[2][128:]
    out["R and after1 swapped, record 3"] = (put(k3, sec([recs[0], recs[1], swapped])), True, (ZM.POK, 3))
    # a record made for another circuit's key (h₀ differs) under the same secret: the same δ′, so the header agrees
    other = w.bare(1, w.S.squaring_chain(6)[0])
    assert ZM.h0(other) != ZM.h0(w.keys[0])
    delta = ZM.delta_of(SECRETS[0])
    rec, _, kcz = ZM.make_record(ZM.h0(other), w.g1(1), 1, SECRETS[0], delta, NAMES[0], w.g1)
    w.note(rec, 1, delta, kcz[0])
    assert rec[:64] == recs[0][:64] and rec != recs[0]
    out["a record of another key"] = (put(w.keys[1], sec([rec])), True, (ZM.POK, 1))
    out["records reordered"] = (put(w.keys[2], sec([recs[1], recs[0]])), True, (ZM.POK, 1))
    out["the last after1 is not the header's"] = (put(w.keys[2], sec(recs[:1])), True, (ZM.HEADER, 0))
    out["count 0, delta1 not G1"] = (w.bare(5), True, (ZM.HEADER, 0))
    hdr, hdr5 = ZC.payload(w.keys[1], 2), ZC.payload(w.bare(5), 2)
    out["delta2 of another delta"] = (ZM.with_section(w.keys[1], 2, hdr[:532] + hdr5[532:660]), False, (ZM.PAIR, 0))
    big = recs[1][:64] + ZM.Q.to_bytes(32, "little") + recs[1][96:]
    out["a coordinate not below q, record 2"] = (put(k3, sec([recs[0], big, recs[2]])), True, (ZM.POINT, 2))
    off = recs[0][:32] + _flip(recs[0][32:64], 0) + recs[0][64:]
    out["after1 off the curve, record 1"] = (put(w.keys[1], sec([off])), True, (ZM.POINT, 1))
    out["after1 the identity"] = (put(w.keys[1], sec([bytes(64) + recs[0][64:]])), True, (ZM.POINT, 1))
    out["count larger than the bytes hold"] = (put(k3, struct.pack("<I", 1000) + sec(recs)[4:]), True, (ZM.SECTION, 0))
    out["the last record cut short"] = (put(k3, sec(recs)[:-10]), True, (ZM.SECTION, 3))
    longer = recs[2][:160] + struct.pack("<I", len(NAMES[2]) + 1) + recs[2][164:]
    out["name_len runs past the section"] = (put(k3, sec([recs[0], recs[1], longer])), True, (ZM.SECTION, 3))
    out["name_len 256"] = (put(w.keys[1], sec([recs[0][:160] + struct.pack("<I", 256) + bytes(256)])), True, (ZM.SECTION, 1))
    out["bytes behind the last record"] = (put(k3, sec(recs) + b"\0"), True, (ZM.SECTION, 3))
    out["z not below r"] = (put(w.keys[1], sec([recs[0][:128] + R.to_bytes(32, "little") + recs[0][160:]])), True, (ZM.POK, 1))
    return out


CASES = ["one bit of z, record 2", "one bit of a name, record 1", "R and after1 swapped, record 3", "a record of another key", "records reordered",
         "the last after1 is not the header's", "count 0, delta1 not G1", "delta2 of another delta", "a coordinate not below q, record 2",
         "after1 off the curve, record 1", "after1 the identity", "count larger than the bytes hold", "the last record cut short",
         "name_len runs past the section", "name_len 256", "bytes behind the last record", "z not below r"]


@pytest.fixture(scope="module")
def cases(world):
    c = _cases(world)
    assert sorted(c) == sorted(CASES)
    return c


@pytest.mark.parametrize("name", CASES)
def test_a_constructed_fault_gives_its_kind_and_index(world, cases, name):
    key, pair, (kind, index) = cases[name]
    model = ZM.audit(key, world.dlog, world.g1, delta2_matches=pair)
    assert (model[0], model[2], model[3]) == (False, kind, index), name
    verdict, rep = world.audit(key)
    assert verdict == model, name
    # the records whose bounds hold come back whatever the verdict
    if kind != ZM.SECTION:
        assert len(rep.records) == rep.count


def test_a_malformed_key_is_an_error_not_a_verdict(world):
    K = world.K
    with pytest.raises(K.ProverError, match=r"\(-2\)"):
        K.zkey_contributions(world.keys[1][:200])
    secs, order = ZC.sections(world.keys[1])
    twice = world.keys[1][:8] + struct.pack("<I", 11) + world.keys[1][12:] + world.keys[1][secs[10][0] - 12:secs[10][0] + secs[10][1]]
    assert world.audit(twice)[0] == (False, 0, ZM.SECTION, 0)          # section 10 twice
