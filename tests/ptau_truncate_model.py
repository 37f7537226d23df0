"""What groth16_ptau_truncate must write and what groth16_ptau_contributions must say about it (include/groth16_prover.h), restated
over tests/ptau_prepare_model.py and tests/ptau_contribute_model.py, both unchanged: the file of power p is THE MODEL'S OWN file of
power p for the same (τ, α, β) — write_unprepared, expected_prepared — with section 1's ceremonyPower set to P and section 7 taken
from the input; nothing here subtracts a point or copies a prefix of a prepared section.  cut_unprepared is the other statement,
slices of the input's bytes, for inputs the model has no logarithms for (unknown sections).  h0 is the chain's start under the
truncation rule.  Test infrastructure (tests/test_ptau_truncate_host.py, tests/test_gpu_ptau_truncate.py)."""
import struct

import ptau_contribute_model as CM
import ptau_prepare_model as PM

R, Q = PM.R, PM.Q
CUBE_ROOT = pow(5, (R - 1) // 3, R)                                         # ω₃: 1 + ω₃ + ω₃² = 0 (5 generates the field's units)


def header(power, ceremony_power):
    return struct.pack("<I", 32) + Q.to_bytes(32, "little") + struct.pack("<II", power, ceremony_power)


def powers(image):
    return struct.unpack_from("<II", PM.payload(image, 1), 36)


def patched(small, ceremony_power, section7):
    """the model's file of a lower power made the truncation of a file of `ceremony_power`: ceremonyPower, and the input's section 7"""
    p = powers(small)[0]
    return PM.with_payload(PM.with_payload(small, 1, header(p, ceremony_power)), 7, section7)


def expected(full, p, toxic, fbm, to_mont, prepared):
    """truncate(full, p) for a file of the model's with logarithms `toxic`; p = P: the file itself"""
    P = powers(full)[0]
    if p == P:
        return full
    small = PM.write_unprepared(p, *toxic, fbm, to_mont)
    if prepared:
        small = PM.expected_prepared(small, p, *toxic, fbm, to_mont)
    return patched(small, powers(full)[1], PM.payload(full, 7))


def cut_bytes(sid, p, size, prepared):
    n = 1 << p
    if sid in (2, 3, 4, 5):
        return {2: (2 * n - 1) * 64, 3: n * 128, 4: n * 64, 5: n * 64}[sid]
    if prepared and sid in (12, 13, 14, 15):
        return (4 * n - 1) * 64 if sid == 12 else (2 * n - 1) * PM.ELEM[sid]
    return size


def truncated_size(image, p):
    secs, order = PM.sections(image)
    if p == powers(image)[0]:
        return len(image)
    return 12 + sum(12 + cut_bytes(s, p, secs[s][1], 12 in secs) for s in order)


def cut_unprepared(image, p):
    """an UNPREPARED file cut by slices: every section in the input's order, the point sections' prefixes, section 1's power"""
    secs, order = PM.sections(image)
    P, C = powers(image)
    if p == P:
        return image
    assert 12 not in secs and p < P
    out = image[:12]
    for s in order:
        off, ln = secs[s]
        body = header(p, C) if s == 1 else image[off:off + cut_bytes(s, p, ln, False)]
        out += struct.pack("<IQ", s, len(body)) + body
    return out


def hashed_header(image):
    """what h₀ hashes as section 1: the payload, its power field replaced by ceremonyPower when power is below it"""
    p, c = powers(image)
    return header(c, c) if p < c else PM.payload(image, 1)


def h0(image):
    return CM.sha(CM.TAG + hashed_header(image))


def audit(image, dlog, g2log, pb):
    """CM.audit under the truncation rule: the chain over the hashed header, the HEADER rule over the file's own power"""
    return CM.audit(PM.with_payload(image, 1, hashed_header(image)), powers(image)[0], dlog, g2log, pb)
