"""Section 10 as groth16_zkey_contribute writes it and groth16_zkey_contributions audits it (include/groth16_prover.h), restated
with hashlib.sha256 and Python integers: the secrets' derivation W, the hash chain, the Schnorr record, the audit's verdict.  Test
infrastructure (tests/test_zkey_contributions_host.py, tests/test_gpu_zkey_contribute.py).  Every δ₁ here has a known discrete
logarithm d (δ₁ = d·G₁), so the record's points are (d·δ′)·G₁ and (k·d)·G₁ from the oracle's generator multiplication — nothing
here comes from the library under test."""
import hashlib
import struct

import zkey_new_circuits as ZC

R = ZC.R
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
MONT = 1 << 256
TAG = b"icicle-snark zkey contribution v1"
FIXED = 164
SECTION, POINT, POK, HEADER, PAIR = 1, 2, 3, 4, 5
FULL = ZC.FULL
# the scalars the walk must survive (tests/test_zkey_contribute29.py states why each is there)
EDGE_SCALARS = [1, 2, 3, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 1 << 127, (1 << 32) - 1, 1 << 32, 3 << 252, FULL]


def sha(x):
    return hashlib.sha256(x).digest()


def W(x):
    return int.from_bytes(sha(x + b"\0") + sha(x + b"\1"), "big") % R


def delta_of(secret):
    return W(secret + TAG)


def naf(k):
    """digits d_0, d_1, … ∈ {−1, 0, 1} of the non-adjacent form of k ≥ 0, by the textbook's rule (k mod 4)"""
    out = []
    while k:
        d = 0
        if k & 1:
            d = 2 - (k & 3)
            k -= d
        out.append(d)
        k >>= 1
    return out


class G1Bytes:
    """k·G₁ in the file's bytes (affine, Montgomery form, the identity all zero) through the oracle, memoised"""

    def __init__(self, O):
        import groth16_dlog_model as M
        self.pts = M.Points(O)

    def prefetch(self, ks):
        self.pts.need("g1", [k % R for k in ks if k % R])
        self.pts.resolve()

    def __call__(self, k):
        k %= R
        if k == 0:
            return bytes(64)
        self.pts.need("g1", [k])
        self.pts.resolve()
        return b"".join((c * MONT % Q).to_bytes(32, "little") for c in self.pts.g1(k))


def h0(key):
    return sha(TAG + ZC.payload(key, 2)[:468] + ZC.payload(key, 3))


def challenge(e):
    return int.from_bytes(e[:16], "little") or 1


def make_record(h_prev, before1, d_before, secret, delta, name, g1):
    """→ (record bytes, h_i, (k, c, z)); before1: the 64 bytes hashed as δ₁ before, d_before its discrete logarithm"""
    k = W(secret + delta.to_bytes(32, "little") + h_prev + before1)
    assert k and delta
    after1, commit = g1(d_before * delta), g1(k * d_before)
    e = sha(h_prev + before1 + after1 + commit + struct.pack("<I", len(name)) + name)
    c = challenge(e)
    z = (k + c * delta) % R
    return after1 + commit + z.to_bytes(32, "little") + struct.pack("<I", len(name)) + name, e, (k, c, z)


def split_records(p10):
    """section 10's payload → list of record bytes (asserting the bounds)"""
    n, pos, out = struct.unpack_from("<I", p10, 0)[0], 4, []
    for _ in range(n):
        ln = FIXED + struct.unpack_from("<I", p10, pos + 160)[0]
        out.append(p10[pos:pos + ln])
        pos += ln
    assert pos == len(p10)
    return out


def join_records(recs):
    return struct.pack("<I", len(recs)) + b"".join(recs)


def with_section(image, sid, payload):
    """the container with section `sid` replaced in place, or appended behind the last one"""
    secs, order = ZC.sections(image)
    if sid not in secs:
        order = order + [sid]
    body = b"".join(struct.pack("<IQ", s, len(payload) if s == sid else secs[s][1]) + (payload if s == sid else image[secs[s][0]:secs[s][0] + secs[s][1]]) for s in order)
    return image[:8] + struct.pack("<I", len(order)) + body


def _e(h, before, rec):
    """e_i of a record's bytes after1 ‖ R ‖ z ‖ name_len ‖ name: z is not hashed"""
    return sha(h + before + rec[:128] + rec[160:])


def chain_hash(key, recs, g1):
    """h_i behind the records there are, as the audit hashes them: record 1's before1 is G₁"""
    h, before = h0(key), g1(1)
    for rec in recs:
        h = _e(h, before, rec)
        before = rec[:64]
    return h


def contribute(key, d_header, secret, name, g1, delta=None):
    """what groth16_zkey_contribute must write as section 10 of `key` (its header's δ₁ = d_header·G₁) → (payload, δ′)"""
    delta = delta_of(secret) if delta is None else delta
    recs = split_records(ZC.payload(key, 10)) if 10 in ZC.sections(key)[0] else []
    before1 = ZC.payload(key, 2)[468:532]
    assert before1 == g1(d_header)
    rec, _, _ = make_record(chain_hash(key, recs, g1), before1, d_header, secret, delta, name, g1)
    return join_records(recs + [rec]), delta


def on_curve(b):
    x, y = (int.from_bytes(b[i:i + 32], "little") for i in (0, 32))
    if x >= Q or y >= Q:
        return False
    if x == 0 and y == 0:
        return True
    inv = pow(MONT, -1, Q)
    x, y = x * inv % Q, y * inv % Q
    return (y * y - x * x * x - 3) % Q == 0


def audit(key, dlog, g1, delta2_matches=True):
    """the verdict groth16_zkey_contributions must give: (ok, count, kind, index).  dlog: {64 point bytes: discrete logarithm} for
    every point of the records (the tests know them all); delta2_matches: whether the header's δ₂ has δ₁'s logarithm."""
    secs = ZC.sections(key)[0]
    p10 = ZC.payload(key, 10) if 10 in secs else struct.pack("<I", 0)
    if len(p10) < 4:
        return (False, 0, SECTION, 0)
    n = struct.unpack_from("<I", p10, 0)[0]
    if n * FIXED > len(p10) - 4:
        return (False, 0, SECTION, 0)
    pos, recs = 4, []
    for i in range(n):
        if len(p10) - pos < FIXED:
            return (False, n, SECTION, i + 1)
        nl = struct.unpack_from("<I", p10, pos + 160)[0]
        if nl > 255 or len(p10) - pos - FIXED < nl:
            return (False, n, SECTION, i + 1)
        recs.append(p10[pos:pos + FIXED + nl])
        pos += FIXED + nl
    if pos != len(p10):
        return (False, n, SECTION, n)
    h, before = h0(key), g1(1)
    for i, rec in enumerate(recs):
        after1, commit, z = rec[:64], rec[64:128], int.from_bytes(rec[128:160], "little")
        if not on_curve(after1) or not on_curve(commit) or after1 == bytes(64):
            return (False, n, POINT, i + 1)
        h = _e(h, before, rec)
        c = challenge(h)
        if z >= R or (z * dlog[before] - dlog[commit] - c * dlog[after1]) % R:
            return (False, n, POK, i + 1)
        before = after1
    if before != ZC.payload(key, 2)[468:532]:
        return (False, n, HEADER, 0)
    if not delta2_matches:
        return (False, n, PAIR, 0)
    return (True, n, 0, 0)
