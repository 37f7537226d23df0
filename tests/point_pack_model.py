"""What groth16_points_pack / groth16_points_unpack and groth16_ptau_pack / groth16_ptau_unpack must write (include/groth16_prover.h,
DESIGN §7j), restated with Python integers: the sign rule, the packed word of a G1 and of a G2 point, a square root in Fq and one in
Fq2 — the two-exponentiation algorithm for q ≡ 3 (mod 4), NOT the complex method the library uses — the inverse of both encodings
with its refusals, and the packed file over any image tests/ptau_contribute_model.py or tests/ptau_prepare_model.py writes.  Test
infrastructure (tests/test_point_pack29.py, tests/test_ptau_pack_host.py, tests/test_gpu_ptau_pack.py): nothing here comes from the
library under test."""
import struct

import ptau_prepare_model as PM

Q, R = PM.Q, PM.R
MONT = 1 << 256
MONT_INV = pow(MONT, -1, Q)
SOUND, NONCANONICAL, OFF_CURVE, OFF_SUBGROUP = 0, 1, 2, 3
SIGN_BIT, IDENTITY_BIT = 1 << 255, 1 << 254
D82 = pow(82, -1, Q)
B_TWIST = (27 * D82 % Q, -3 * D82 % Q)                                      # 3/ξ, ξ = 9 + u
POINT_BYTES = {2: 64, 3: 128, 4: 64, 5: 64, 6: 128, 12: 64, 13: 128, 14: 64, 15: 64}   # a packed element has half of it
KIND_TEXT = {NONCANONICAL: "a coordinate is not below q", OFF_CURVE: "the point is not on the curve", OFF_SUBGROUP: "the point is outside the subgroup"}


def to_file(x):
    return x * MONT % Q


def from_file(v):
    return v * MONT_INV % Q


# ---- signs
def sign_fq(y):
    """y: the STANDARD-form integer, 0 <= y < q"""
    return 1 if y > (Q - 1) // 2 else 0


def sign_fq2(y):
    return sign_fq(y[1]) if y[1] else sign_fq(y[0])


# ---- roots
def sqrt_fq(a):
    """a root of a mod q, or None"""
    r = pow(a, (Q + 1) // 4, Q)
    return r if r * r % Q == a % Q else None


def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def f2pow(a, e):
    r = (1, 0)
    for bit in bin(e)[2:]:
        r = f2mul(r, r)
        if bit == "1":
            r = f2mul(r, a)
    return r


def sqrt_fq2(a):
    """a root of a in Fq[u]/(u² + 1), or None: Adj and Rodríguez-Henríquez, "Square root computation over even extension fields",
    algorithm 9 (q ≡ 3 mod 4) — two exponentiations in Fq2"""
    a = (a[0] % Q, a[1] % Q)
    if a == (0, 0):
        return (0, 0)
    a1 = f2pow(a, (Q - 3) // 4)
    alpha = f2mul(a1, f2mul(a1, a))
    a0 = f2mul((alpha[0], -alpha[1] % Q), alpha)
    if a0 == (Q - 1, 0):
        return None
    x0 = f2mul(a1, a)
    x = f2mul((0, 1), x0) if alpha == (Q - 1, 0) else f2mul(f2pow(((1 + alpha[0]) % Q, alpha[1]), (Q - 1) // 2), x0)
    assert f2mul(x, x) == a
    return x


def g1_rhs(x):
    return (x * x * x + 3) % Q


def g2_rhs(x):
    c = f2mul(f2mul(x, x), x)
    return ((c[0] + B_TWIST[0]) % Q, (c[1] + B_TWIST[1]) % Q)


# ---- one point
def _ints(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _bytes(vs):
    return b"".join(int(v).to_bytes(32, "little") for v in vs)


def pack_g1(point):
    """64 file bytes of a SOUND point → its 32 packed bytes"""
    vx, vy = _ints(point)
    if vx == 0 and vy == 0:
        return _bytes([IDENTITY_BIT])
    return _bytes([vx | (SIGN_BIT if sign_fq(from_file(vy)) else 0)])


def pack_g2(point):
    """128 file bytes of a SOUND point → its 64 packed bytes"""
    v = _ints(point)
    if not any(v):
        return _bytes([0, IDENTITY_BIT])
    return _bytes([v[0], v[1] | (SIGN_BIT if sign_fq2((from_file(v[2]), from_file(v[3]))) else 0)])


def unpack_g1(word):
    """32 packed bytes → (kind, 64 file bytes | None)"""
    (w,) = _ints(word)
    sign, flag, vx = w >> 255, (w >> 254) & 1, w & (IDENTITY_BIT - 1)
    if flag:
        return (SOUND, bytes(64)) if w == IDENTITY_BIT else (NONCANONICAL, None)
    if vx >= Q:
        return (NONCANONICAL, None)
    y = sqrt_fq(g1_rhs(from_file(vx)))
    if y is None:
        return (OFF_CURVE, None)
    if y == 0 and sign:
        return (NONCANONICAL, None)
    if sign_fq(y) != sign:
        y = -y % Q
    return (SOUND, _bytes([vx, to_file(y)]))


def unpack_g2(word, in_subgroup):
    """64 packed bytes → (kind, 128 file bytes | None).  in_subgroup((x, y)) → bool decides step 7 (the caller's integers: r·P = O)"""
    v0, w = _ints(word)
    sign, flag, v1 = w >> 255, (w >> 254) & 1, w & (IDENTITY_BIT - 1)
    if flag:
        return (SOUND, bytes(128)) if (v0, w) == (0, IDENTITY_BIT) else (NONCANONICAL, None)
    if v0 >= Q or v1 >= Q:
        return (NONCANONICAL, None)
    x = (from_file(v0), from_file(v1))
    y = sqrt_fq2(g2_rhs(x))
    if y is None:
        return (OFF_CURVE, None)
    if y == (0, 0) and sign:
        return (NONCANONICAL, None)
    if sign_fq2(y) != sign:
        y = (-y[0] % Q, -y[1] % Q)
    if not in_subgroup((x, y)):
        return (OFF_SUBGROUP, None)
    return (SOUND, _bytes([v0, v1, to_file(y[0]), to_file(y[1])]))


def pack_points(buf, g2):
    size, f = (128, pack_g2) if g2 else (64, pack_g1)
    assert len(buf) % size == 0
    return b"".join(f(buf[i:i + size]) for i in range(0, len(buf), size))


# ---- the packed file
def packed_section_bytes(power, sid):
    N = 1 << power
    return {2: (2 * N - 1) * 32, 3: N * 64, 4: N * 32, 5: N * 32, 6: 64, 12: (4 * N - 1) * 32, 13: (2 * N - 1) * 64, 14: (2 * N - 1) * 32, 15: (2 * N - 1) * 32}[sid]


def packed_size(power, prepared, other_bytes=44 + 4, other_sections=2):
    """the packed file of a .ptau whose sections besides the point sections (1 and 7 of a fresh file) hold other_bytes"""
    ids = [2, 3, 4, 5, 6] + ([12, 13, 14, 15] if prepared else [])
    return 12 + 12 * (len(ids) + other_sections) + other_bytes + sum(packed_section_bytes(power, s) for s in ids)


def unpacked_size(power, prepared, other_bytes=44 + 4, other_sections=2):
    ids = [2, 3, 4, 5, 6] + ([12, 13, 14, 15] if prepared else [])
    return 12 + 12 * (len(ids) + other_sections) + other_bytes + 2 * sum(packed_section_bytes(power, s) for s in ids)


def pack_file(image):
    """the packed file of a sound .ptau image: magic ptaz, version 1, the sections in the image's order, the point sections packed,
    every other section byte for byte"""
    secs, order = PM.sections(image)
    out = b"ptaz" + struct.pack("<II", 1, len(order))
    for sid in order:
        p = image[secs[sid][0]:secs[sid][0] + secs[sid][1]]
        if sid in POINT_BYTES:
            p = pack_points(p, POINT_BYTES[sid] == 128)
        out += struct.pack("<IQ", sid, len(p)) + p
    return out
