"""The random beacon of both ceremony phases as groth16_ptau_beacon / groth16_zkey_beacon must write it and
groth16_ptau_contributions / groth16_zkey_contributions must judge it (include/groth16_prover.h), restated with
hashlib.sha256 and Python integers over tests/ptau_contribute_model.py and tests/zkey_contribute_model.py: the digest (2^iter_exp
sequential hashes), the secrets (a contribution's with secret := digest), the record (bit 31 of the stored name_len word, beacon_hash
and iter_exp behind the name, e_i over all of it), the expected files from the toxic values, and audits that know every discrete
logarithm.  Test infrastructure (tests/test_beacon_host.py, tests/test_gpu_beacon.py).  Nothing here comes from the library under
test; every point comes from the oracle's generator multiplication."""
import functools
import hashlib
import struct

import ptau_contribute_model as CM
import ptau_prepare_model as PM
import zkey_contribute_model as ZM
import zkey_new_circuits as ZC

R = CM.R
FLAG = 1 << 31
TRAILER = 36
ITER_EXP_MAX = 24
WORK_MAX = 1 << 25
SECTION, POINT, POK, HEADER, PAIR, BEACON = 1, 2, 3, 4, 5, 6
LAYOUTS = {"ptau": (CM.FIXED, CM.NAME_LEN), "zkey": (ZM.FIXED, 160)}       # (fixed bytes of a record, offset of name_len in them)

sha = CM.sha


@functools.lru_cache(maxsize=None)
def digest(beacon_hash, iter_exp):
    """d₀ = beacon_hash, d_{j+1} = SHA-256(d_j); d at j = 2^iter_exp (iter_exp = 0: one hash)"""
    d = beacon_hash
    for _ in range(1 << iter_exp):
        d = hashlib.sha256(d).digest()
    return d


def tail(name, beacon):
    """a record from its name_len word on; beacon: None or (beacon_hash, iter_exp)"""
    if beacon is None:
        return struct.pack("<I", len(name)) + name
    return struct.pack("<I", len(name) | FLAG) + name + beacon[0] + struct.pack("<I", beacon[1])


def split_records(payload, layout):
    """a section's payload → list of record bytes, beacon records with their trailer (asserting the bounds)"""
    fixed, off = LAYOUTS[layout]
    n, pos, out = struct.unpack_from("<I", payload, 0)[0], 4, []
    for _ in range(n):
        word = struct.unpack_from("<I", payload, pos + off)[0]
        ln = fixed + (word & ~FLAG) + (TRAILER if word & FLAG else 0)
        out.append(payload[pos:pos + ln])
        pos += ln
    assert pos == len(payload)
    return out


def beacon_of(rec, layout):
    """(beacon_hash, iter_exp) of a record's bytes, None for a participant's"""
    fixed, off = LAYOUTS[layout]
    word = struct.unpack_from("<I", rec, off)[0]
    if not word & FLAG:
        return None
    t = rec[fixed + (word & ~FLAG):]
    return t[:32], struct.unpack_from("<I", t, 32)[0]


def beacons_of(recs, layout):
    """what .beacons of the audit's report must be: {record number from 1: (beacon_hash, iter_exp)}"""
    return {i + 1: beacon_of(rec, layout) for i, rec in enumerate(recs) if beacon_of(rec, layout)}


join_records = CM.join_records


# ---- the .ptau ---------------------------------------------------------------------------------------------------------------------
def ptau_record(h_prev, before, d_before, held, name, pb, beacon=None, secret=None, primes=None):
    """→ (record bytes, h_i, [(k, c, z)], (τ′, α′, β′)): tests/ptau_contribute_model.py's make_record with the beacon's tail.  beacon:
    (beacon_hash, iter_exp), and the secret is its digest unless `secret` says otherwise (a record whose digest nobody is to
    compute); None: a participant's record of `secret`.  primes: the secrets themselves where they are NOT to be the derived ones —
    the proofs of knowledge stay honest."""
    if secret is None:
        secret = digest(*beacon)
    primes = primes or CM.secrets_of(secret)
    ks = [CM.W(secret + x.to_bytes(32, "little") + h_prev + before[64 * i:64 * i + 64] + CM.LABELS[i]) for i, x in enumerate(primes)]
    assert all(ks) and all(primes)
    after = [t * x % R for t, x in zip(held, primes)]
    pb.prefetch(g1=after + [k * d for k, d in zip(ks, d_before)], g2=[after[0], after[2]])
    points = b"".join(pb.g1(a) for a in after) + pb.g2(after[0]) + pb.g2(after[2])
    commits = b"".join(pb.g1(k * d) for k, d in zip(ks, d_before))
    t = tail(name, beacon)
    e = sha(h_prev + before + points + commits + t)
    c = CM.challenge(e)
    zs = [(k + c * x) % R for k, x in zip(ks, primes)]
    return points + commits + b"".join(z.to_bytes(32, "little") for z in zs) + t, e, [(k, c, z) for k, z in zip(ks, zs)], tuple(primes)


def expected_ptau(raw, power, toxic, name, fbm, to_mont, pb, beacon=None, secret=None, primes=None, d_before=None):
    """→ (the whole file groth16_ptau_beacon — or, beacon None, groth16_ptau_contribute behind beacon records — must write for `raw`,
    an unprepared file whose points have the logarithms `toxic` = (τ, α, β); the secrets applied): write_unprepared over the products
    in sections 1 to 6, section 7 with the model's record appended.  As expected_contributed of tests/ptau_contribute_model.py."""
    recs = split_records(PM.payload(raw, 7), "ptau")
    if d_before is None:
        d_before = toxic if recs else (1, 1, 1)
    before = recs[-1][:192] if recs else CM.generators(pb)[:192]
    rec, _, _, primes = ptau_record(CM.chain_hash(raw, recs, pb), before, d_before, toxic, name, pb, beacon, secret, primes)
    new = tuple(t * x % R for t, x in zip(toxic, primes))
    return PM.with_payload(PM.write_unprepared(power, *new, fbm, to_mont), 7, join_records(recs + [rec])), primes


def audit_ptau(image, power, dlog, g2log, pb):
    """the verdict groth16_ptau_contributions must give, beacon records included: (ok, count, kind, index).  dlog, g2log as
    tests/ptau_contribute_model.py's audit takes them.  Per record POINT, POK, BEACON, PAIR; HEADER at the end."""
    p7 = PM.payload(image, 7)
    fixed, off = LAYOUTS["ptau"]
    if len(p7) < 4:
        return (False, 0, SECTION, 0)
    n = struct.unpack_from("<I", p7, 0)[0]
    if n * fixed > len(p7) - 4:
        return (False, 0, SECTION, 0)
    pos, recs = 4, []
    for i in range(n):
        if len(p7) - pos < fixed:
            return (False, n, SECTION, i + 1)
        word = struct.unpack_from("<I", p7, pos + off)[0]
        nl, behind = word & ~FLAG, (word & ~FLAG) + (TRAILER if word & FLAG else 0)
        if nl > 255 or len(p7) - pos - fixed < behind:
            return (False, n, SECTION, i + 1)
        recs.append(p7[pos:pos + fixed + behind])
        pos += fixed + behind
    if pos != len(p7):
        return (False, n, SECTION, n)
    h, last, work = CM.h0(image), CM.generators(pb), 0
    for i, rec in enumerate(recs):
        g1s = [rec[o:o + 64] for o in (CM.TAU1, CM.ALPHA1, CM.BETA1, CM.R_TAU, CM.R_TAU + 64, CM.R_TAU + 128)]
        tau2, beta2 = rec[CM.TAU2:CM.TAU2 + 128], rec[CM.BETA2:CM.BETA2 + 128]
        if not all(CM.on_curve_g1(p) for p in g1s) or bytes(64) in g1s[:3] or tau2 not in g2log or beta2 not in g2log or not g2log[tau2] or not g2log[beta2]:
            return (False, n, POINT, i + 1)
        h = CM._e(h, last[:192], rec)
        c = CM.challenge(h)
        for x in range(3):
            z = int.from_bytes(rec[CM.Z_TAU + 32 * x:CM.Z_TAU + 32 * x + 32], "little")
            if z >= R or (z * dlog[last[64 * x:64 * x + 64]] - dlog[g1s[3 + x]] - c * dlog[g1s[x]]) % R:
                return (False, n, POK, i + 1)
        b = beacon_of(rec, "ptau")
        if b:
            if b[1] > ITER_EXP_MAX:
                return (False, n, BEACON, i + 1)
            work += 1 << b[1]
            if work > WORK_MAX:
                return (False, n, BEACON, i + 1)
            primes = CM.secrets_of(digest(*b))
            if not all(primes) or any(dlog[g1s[x]] != primes[x] * dlog[last[64 * x:64 * x + 64]] % R for x in range(3)):
                return (False, n, BEACON, i + 1)
        if dlog[g1s[0]] != g2log[tau2] or dlog[g1s[2]] != g2log[beta2]:
            return (False, n, PAIR, i + 1)
        last = rec[:448]
    held = [(CM.ALPHA1, PM.payload(image, 4)[:64]), (CM.BETA1, PM.payload(image, 5)[:64]), (CM.BETA2, PM.payload(image, 6))]
    if power >= 1:
        held += [(CM.TAU1, PM.payload(image, 2)[64:128]), (CM.TAU2, PM.payload(image, 3)[128:256])]
    if any(last[o:o + len(p)] != p for o, p in held):
        return (False, n, HEADER, 0)
    return (True, n, 0, 0)


# ---- the .zkey ---------------------------------------------------------------------------------------------------------------------
def zkey_record(h_prev, before1, d_before, name, g1, beacon=None, secret=None, delta=None):
    """→ (record bytes, h_i, (k, c, z), δ′): tests/zkey_contribute_model.py's make_record with the beacon's tail; the arguments as
    ptau_record's"""
    if secret is None:
        secret = digest(*beacon)
    delta = delta or ZM.delta_of(secret)
    k = ZM.W(secret + delta.to_bytes(32, "little") + h_prev + before1)
    assert k and delta
    after1, commit = g1(d_before * delta), g1(k * d_before)
    t = tail(name, beacon)
    e = sha(h_prev + before1 + after1 + commit + t)
    c = ZM.challenge(e)
    z = (k + c * delta) % R
    return after1 + commit + z.to_bytes(32, "little") + t, e, (k, c, z), delta


def zkey_records(key):
    return split_records(ZC.payload(key, 10), "zkey") if 10 in ZC.sections(key)[0] else []


def expected_section10(key, d_header, name, g1, beacon=None, secret=None, delta=None):
    """→ (what groth16_zkey_beacon — or, beacon None, groth16_zkey_contribute behind beacon records — must write as section 10 of
    `key`, whose header's δ₁ = d_header·G₁; δ′)"""
    recs = zkey_records(key)
    before1 = ZC.payload(key, 2)[468:532]
    assert before1 == g1(d_header)
    rec, _, _, delta = zkey_record(ZM.chain_hash(key, recs, g1), before1, d_header, name, g1, beacon, secret, delta)
    return join_records(recs + [rec]), delta


def audit_zkey(key, dlog, g1, delta2_matches=True):
    """the verdict groth16_zkey_contributions must give, beacon records included: (ok, count, kind, index).  Per record POINT, POK,
    BEACON; HEADER and PAIR at the end."""
    fixed, off = LAYOUTS["zkey"]
    p10 = ZC.payload(key, 10) if 10 in ZC.sections(key)[0] else struct.pack("<I", 0)
    if len(p10) < 4:
        return (False, 0, SECTION, 0)
    n = struct.unpack_from("<I", p10, 0)[0]
    if n * fixed > len(p10) - 4:
        return (False, 0, SECTION, 0)
    pos, recs = 4, []
    for i in range(n):
        if len(p10) - pos < fixed:
            return (False, n, SECTION, i + 1)
        word = struct.unpack_from("<I", p10, pos + off)[0]
        nl, behind = word & ~FLAG, (word & ~FLAG) + (TRAILER if word & FLAG else 0)
        if nl > 255 or len(p10) - pos - fixed < behind:
            return (False, n, SECTION, i + 1)
        recs.append(p10[pos:pos + fixed + behind])
        pos += fixed + behind
    if pos != len(p10):
        return (False, n, SECTION, n)
    h, before, work = ZM.h0(key), g1(1), 0
    for i, rec in enumerate(recs):
        after1, commit, z = rec[:64], rec[64:128], int.from_bytes(rec[128:160], "little")
        if not ZM.on_curve(after1) or not ZM.on_curve(commit) or after1 == bytes(64):
            return (False, n, POINT, i + 1)
        h = ZM._e(h, before, rec)
        c = ZM.challenge(h)
        if z >= R or (z * dlog[before] - dlog[commit] - c * dlog[after1]) % R:
            return (False, n, POK, i + 1)
        b = beacon_of(rec, "zkey")
        if b:
            if b[1] > ITER_EXP_MAX:
                return (False, n, BEACON, i + 1)
            work += 1 << b[1]
            if work > WORK_MAX:
                return (False, n, BEACON, i + 1)
            delta = ZM.delta_of(digest(*b))
            if not delta or dlog[after1] != delta * dlog[before] % R:
                return (False, n, BEACON, i + 1)
        before = after1
    if before != ZC.payload(key, 2)[468:532]:
        return (False, n, HEADER, 0)
    if not delta2_matches:
        return (False, n, PAIR, 0)
    return (True, n, 0, 0)
