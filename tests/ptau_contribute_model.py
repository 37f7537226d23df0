"""What groth16_ptau_new and groth16_ptau_contribute must write and groth16_ptau_contributions must say (include/groth16_prover.h),
restated with hashlib.sha256 and Python integers: the secrets' derivation W with its labels, the hash chain, the three Schnorr
proofs of a record, the audit's verdict, and the contributed file — tests/ptau_prepare_model.py's write_unprepared for sections 1 to
6 of (τ·τ′, α·α′, β·β′), this module's section 7.  Test infrastructure (tests/test_ptau_contribute29.py,
tests/test_ptau_contributions_host.py, tests/test_gpu_ptau_contribute.py).  Every point here has a known discrete logarithm and
comes from the oracle's generator multiplication — nothing comes from the library under test."""
import hashlib
import struct

import ptau_prepare_model as PM

R, Q = PM.R, PM.Q
MONT = 1 << 256
TAG = b"icicle-snark ptau contribution v1"
FIXED = 740
TAU1, ALPHA1, BETA1, TAU2, BETA2, R_TAU, Z_TAU, NAME_LEN = 0, 64, 128, 192, 320, 448, 640, 736
SECTION, POINT, POK, HEADER, PAIR = 1, 2, 3, 4, 5
LABELS = (b"\1", b"\2", b"\3")                                              # τ, α, β


def sha(x):
    return hashlib.sha256(x).digest()


def W(x):
    return int.from_bytes(sha(x + b"\0") + sha(x + b"\1"), "big") % R


def secrets_of(secret):
    """(τ′, α′, β′) of a participant's 32 bytes"""
    return tuple(W(secret + TAG + lab) for lab in LABELS)


def challenge(e):
    return int.from_bytes(e[:16], "little") or 1


def table_bits(power):
    return (power + 2) // 2


class PointBytes:
    """k·G₁ / k·G₂ in the file's bytes (affine, Montgomery form, the identity all zero) through the oracle, memoised"""

    def __init__(self, O):
        import groth16_dlog_model as M
        self.pts = M.Points(O)

    def prefetch(self, g1=(), g2=()):
        self.pts.need("g1", [k % R for k in g1 if k % R])
        self.pts.need("g2", [k % R for k in g2 if k % R])
        self.pts.resolve()

    def g1(self, k):
        k %= R
        if k == 0:
            return bytes(64)
        self.prefetch(g1=[k])
        return b"".join((c * MONT % Q).to_bytes(32, "little") for c in self.pts.g1(k))

    def g2(self, k):
        k %= R
        if k == 0:
            return bytes(128)
        self.prefetch(g2=[k])
        return b"".join((c * MONT % Q).to_bytes(32, "little") for c in self.pts.g2(k))


def h0(image):
    return sha(TAG + PM.payload(image, 1))


def generators(pb):
    """record 0: (G₁, G₁, G₁, G₂, G₂) in a record's order"""
    return pb.g1(1) * 3 + pb.g2(1) * 2


def make_record(h_prev, before, d_before, held, primes, secret, name, pb, g2_after=None):
    """→ (record bytes, h_i, [(k, c, z)] for τ, α, β).  before: the 192 bytes hashed as (tau1, alpha1, beta1) before, d_before
    their discrete logarithms; held: the logarithms (τ, α, β) of the points the secrets multiply — what the FILE holds (at power 0
    its τ is the chain's); primes: (τ′, α′, β′); g2_after: logarithms of (tau2, beta2) when a test wants them NOT to be tau1's and beta1's."""
    ks = [W(secret + x.to_bytes(32, "little") + h_prev + before[64 * i:64 * i + 64] + LABELS[i]) for i, x in enumerate(primes)]
    assert all(ks) and all(primes)
    after = [t * x % R for t, x in zip(held, primes)]
    t2, b2 = g2_after or (after[0], after[2])
    pb.prefetch(g1=after + [k * d for k, d in zip(ks, d_before)], g2=[t2, b2])
    points = b"".join(pb.g1(a) for a in after) + pb.g2(t2) + pb.g2(b2)
    commits = b"".join(pb.g1(k * d) for k, d in zip(ks, d_before))
    tail = struct.pack("<I", len(name)) + name
    e = sha(h_prev + before + points + commits + tail)
    c = challenge(e)
    zs = [(k + c * x) % R for k, x in zip(ks, primes)]
    return points + commits + b"".join(z.to_bytes(32, "little") for z in zs) + tail, e, [(k, c, z) for k, z in zip(ks, zs)]


def split_records(p7):
    """section 7's payload → list of record bytes (asserting the bounds)"""
    n, pos, out = struct.unpack_from("<I", p7, 0)[0], 4, []
    for _ in range(n):
        ln = FIXED + struct.unpack_from("<I", p7, pos + NAME_LEN)[0]
        out.append(p7[pos:pos + ln])
        pos += ln
    assert pos == len(p7)
    return out


def join_records(recs):
    return struct.pack("<I", len(recs)) + b"".join(recs)


def _e(h, before, rec):
    """e_i of a record's bytes: the responses are not hashed"""
    return sha(h + before + rec[:Z_TAU] + rec[NAME_LEN:])


def chain_hash(image, recs, pb):
    h, before = h0(image), generators(pb)[:192]
    for rec in recs:
        h = _e(h, before, rec)
        before = rec[:192]
    return h


def contribute_section7(image, d_before, held, primes, secret, name, pb):
    """what groth16_ptau_contribute must write as section 7 of `image` → (payload, the record's (k, c, z) triples).  d_before: the
    logarithms of the last record's (tau1, alpha1, beta1), (1, 1, 1) without one; held: those of the file's points"""
    recs = split_records(PM.payload(image, 7))
    before = recs[-1][:192] if recs else generators(pb)[:192]
    rec, _, kcz = make_record(chain_hash(image, recs, pb), before, d_before, held, primes, secret, name, pb)
    return join_records(recs + [rec]), kcz


def expected_contributed(raw, power, toxic, primes, secret, name, fbm, to_mont, pb, d_before=None):
    """the whole file groth16_ptau_contribute must write for `raw` — an unprepared file whose points have the logarithms `toxic` =
    (τ, α, β) — and (τ′, α′, β′) = primes: write_unprepared(power, τ·τ′, α·α′, β·β′) in sections 1 to 6, the model's section 7.
    d_before defaults to toxic when the file has records (a chain that started at the generators) and to (1, 1, 1) without."""
    if d_before is None:
        d_before = toxic if split_records(PM.payload(raw, 7)) else (1, 1, 1)
    new = tuple(t * x % R for t, x in zip(toxic, primes))
    p7, _ = contribute_section7(raw, d_before, toxic, primes, secret, name, pb)
    return PM.with_payload(PM.write_unprepared(power, *new, fbm, to_mont), 7, p7)


def on_curve_g1(b):
    x, y = (int.from_bytes(b[i:i + 32], "little") for i in (0, 32))
    if x >= Q or y >= Q:
        return False
    if x == 0 and y == 0:
        return True
    inv = pow(MONT, -1, Q)
    x, y = x * inv % Q, y * inv % Q
    return (y * y - x * x * x - 3) % Q == 0


def audit(image, power, dlog, g2log, pb):
    """the verdict groth16_ptau_contributions must give: (ok, count, kind, index).  dlog: {64 point bytes: logarithm} for every G1
    point of the records, g2log: {128 point bytes: logarithm} for every G2 point that is in the subgroup — a G2 point that is not
    in it (off the curve, outside the subgroup, a coordinate ≥ q) is a POINT fault; the tests know them all."""
    p7 = PM.payload(image, 7)
    if len(p7) < 4:
        return (False, 0, SECTION, 0)
    n = struct.unpack_from("<I", p7, 0)[0]
    if n * FIXED > len(p7) - 4:
        return (False, 0, SECTION, 0)
    pos, recs = 4, []
    for i in range(n):
        if len(p7) - pos < FIXED:
            return (False, n, SECTION, i + 1)
        nl = struct.unpack_from("<I", p7, pos + NAME_LEN)[0]
        if nl > 255 or len(p7) - pos - FIXED < nl:
            return (False, n, SECTION, i + 1)
        recs.append(p7[pos:pos + FIXED + nl])
        pos += FIXED + nl
    if pos != len(p7):
        return (False, n, SECTION, n)
    h, last = h0(image), generators(pb)
    for i, rec in enumerate(recs):
        g1s = [rec[o:o + 64] for o in (TAU1, ALPHA1, BETA1, R_TAU, R_TAU + 64, R_TAU + 128)]
        tau2, beta2 = rec[TAU2:TAU2 + 128], rec[BETA2:BETA2 + 128]
        if not all(on_curve_g1(p) for p in g1s) or bytes(64) in g1s[:3] or tau2 not in g2log or beta2 not in g2log or not g2log[tau2] or not g2log[beta2]:
            return (False, n, POINT, i + 1)
        h = _e(h, last[:192], rec)
        c = challenge(h)
        for x in range(3):
            z = int.from_bytes(rec[Z_TAU + 32 * x:Z_TAU + 32 * x + 32], "little")
            if z >= R or (z * dlog[last[64 * x:64 * x + 64]] - dlog[g1s[3 + x]] - c * dlog[g1s[x]]) % R:
                return (False, n, POK, i + 1)
        if dlog[g1s[0]] != g2log[tau2] or dlog[g1s[2]] != g2log[beta2]:
            return (False, n, PAIR, i + 1)
        last = rec[:448]
    held = [(ALPHA1, PM.payload(image, 4)[:64]), (BETA1, PM.payload(image, 5)[:64]), (BETA2, PM.payload(image, 6))]
    if power >= 1:
        held += [(TAU1, PM.payload(image, 2)[64:128]), (TAU2, PM.payload(image, 3)[128:256])]
    if any(last[o:o + len(p)] != p for o, p in held):
        return (False, n, HEADER, 0)
    return (True, n, 0, 0)
