"""What groth16_ptau_verify must answer (include/groth16_prover.h), restated with Python integers in the exponent: a writer of a
powers-of-tau file, prepared or not, from ARBITRARY discrete-logarithm lists per section; the exact truth about such lists — no
randomness: generators are 1, the logarithms of P_1 and Q_1 are equal, s[i+1] = τ₂·s[i] for every i, each block equals the direct
O(n²) inverse transform of its source — as (ok, kind, mask, fault); and the seed-derived values of the randomised Lagrange equation
(x, μ_p, λ_e, d_i) for the checked host build and the identity's own test.  Test infrastructure (tests/test_ptau_verify_model.py,
tests/test_ptau_verify29.py, tests/test_gpu_ptau_verify.py); points come from ptau_prepare_model's helpers."""
import hashlib
import struct

import ptau_prepare_model as PM

R = PM.R
TAG = b"icicle-snark ptau verify v1"
GENERATORS, TAU_PAIR, BETA_PAIR, TAU_G1, TAU_G2, ALPHA_TAU, BETA_TAU, LAGRANGE_12, LAGRANGE_13, LAGRANGE_14, LAGRANGE_15, POINT, IDENTITY = range(1, 14)
KIND_NAMES = ["", "GENERATORS", "TAU_PAIR", "BETA_PAIR", "TAU_G1", "TAU_G2", "ALPHA_TAU", "BETA_TAU", "LAGRANGE_12", "LAGRANGE_13", "LAGRANGE_14",
              "LAGRANGE_15", "POINT", "IDENTITY"]


def bit(kind):
    return 1 << (kind - 1)


# ---- files from discrete logarithms
def sound_logs(power, tau, alpha, beta, prepared):
    """the logarithms of a sound file: {2, 3, 4, 5, 6} and, prepared, {12, 13, 14, 15}"""
    logs = {k: list(v) for k, v in PM.source_scalars(power, tau, alpha, beta).items()}
    logs[6] = [beta % R]
    if prepared:
        logs.update({k: list(v) for k, v in PM.prepared_scalars(power, tau, alpha, beta).items()})
    return logs


def write_file(power, logs, fbm, to_mont, section7=struct.pack("<I", 0)):
    """the file whose section s holds logs[s][i]·G; sections 12 … 15 are written when logs has them (any of them)"""
    secs = [(1, PM._header(power))]
    for s in (2, 3, 4, 5, 6):
        secs.append((s, PM._points("g2" if s in (3, 6) else "g1", logs[s], fbm, to_mont)))
    secs.append((7, section7))
    for s in (12, 13, 14, 15):
        if s in logs:
            secs.append((s, PM._points("g2" if s == 13 else "g1", logs[s], fbm, to_mont)))
    return b"ptau" + struct.pack("<II", 1, len(secs)) + b"".join(PM._section(s, p) for s, p in secs)


# ---- the exact truth
def _follows(s, ratio):
    return all(s[i + 1] % R == ratio * s[i] % R for i in range(len(s) - 1))


def truth(power, logs):
    """(ok, kind, mask, fault): fault = (section, element) for IDENTITY, None otherwise.  An identity (logarithm 0) in sections 6, 2,
    3, 4, 5 — in this order, the lowest element — ends the verdict with mask 0; else one bit per equation that fails in truth."""
    N = 1 << power
    assert [len(logs[s]) for s in (2, 3, 4, 5, 6)] == [2 * N - 1, N, N, N, 1]
    for s in (6, 2, 3, 4, 5):
        for i, v in enumerate(logs[s]):
            if v % R == 0:
                return False, IDENTITY, 0, (s, i)
    mask = 0
    if logs[2][0] % R != 1 or logs[3][0] % R != 1:
        mask |= bit(GENERATORS)
    if (logs[5][0] - logs[6][0]) % R:
        mask |= bit(BETA_PAIR)
    if power >= 1:
        tau2 = logs[3][1]
        if (logs[2][1] - tau2) % R:
            mask |= bit(TAU_PAIR)
        for s, kind in ((2, TAU_G1), (3, TAU_G2), (4, ALPHA_TAU), (5, BETA_TAU)):
            if not _follows(logs[s], tau2):
                mask |= bit(kind)
    if 12 in logs:
        for k, sid in enumerate((12, 13, 14, 15)):
            src, blocks = logs[PM.SOURCE[sid]], power + (2 if sid == 12 else 1)
            assert len(logs[sid]) == (1 << blocks) - 1
            want = []
            for p in range(blocks):
                want += PM.inverse_transform(src[:1 << p], p)
            if [v % R for v in logs[sid]] != want:
                mask |= bit(LAGRANGE_12 + k)
    kind = next((k for k in range(1, 12) if mask & bit(k)), 0)
    return mask == 0, kind, mask, None


# ---- the randomised Lagrange equation's values
def coefficient(seed, i):
    """sha256.h's combined_coefficient: the first 16 bytes of SHA-256(seed ‖ LE64(i)), little-endian, 0 → 1"""
    return int.from_bytes(hashlib.sha256(seed + i.to_bytes(8, "little")).digest()[:16], "little") or 1


def x_of(seed, power):
    """(x, c): the first c whose digest, big-endian mod r, is not 0 and lies in no domain up to 2^(power+1)"""
    c = 0
    while True:
        x = int.from_bytes(hashlib.sha256(seed + TAG + struct.pack("<I", c)).digest(), "big") % R
        if x and pow(x, 2 << power, R) != 1:
            return x, c
        c += 1


def mu_of(seed, p):
    return coefficient(seed, (1 << 32) + p)


def block_of(e):
    return (e + 1).bit_length() - 1


def lam(power, e, x, mu):
    """λ_e; mu: p → μ_p"""
    p = block_of(e)
    j = e + 1 - (1 << p)
    w = pow(PM.omega(power + 1), j << (power + 1 - p), R)
    return mu(p) * (pow(x, 1 << p, R) - 1) * pow(x - w, -1, R) % R


def t_of(q, pmax, x, mu):
    return sum(mu(p) * pow(x, 1 << p, R) for p in range(q, pmax + 1)) % R


def d_of(i, pmax, x, mu):
    """d_i; q = the least p with 2^p > i is i's bit length"""
    return pow(pow(x, -1, R), i + 1, R) * t_of(i.bit_length(), pmax, x, mu) % R


def lagrange_sides(power, sid, src, blk, x, mu):
    """(Σ_e λ_e·b_e, Σ_i d_i·s_i) mod r for one section's logarithms"""
    pmax = power + 1 if sid == 12 else power
    n = min(len(src), 1 << pmax)
    return (sum(lam(power, e, x, mu) * b for e, b in enumerate(blk)) % R, sum(d_of(i, pmax, x, mu) * src[i] for i in range(n)) % R)


def cancelling_errors(p, j, delta):
    """{element: error} over blocks p and p + 1 of a prepared section: δ at (p, j) and −g(ω_2n^k)·ω_2n^k/(2n)·δ at every k of block
    p + 1, g(X) = (X^n − 1)/(X − ω_p^j) = Σ_m (ω_p^j)^(n−1−m)·X^m, n = 2^p.  With equal multipliers the two blocks' contributions to
    the left side cancel for every x."""
    n = 1 << p
    c = pow(PM.omega(p), j, R)
    w2 = PM.omega(p + 1)
    out = {n - 1 + j: delta % R}
    inv2n = pow(2 * n, -1, R)
    for k in range(2 * n):
        wk = pow(w2, k, R)
        g = sum(pow(c, n - 1 - m, R) * pow(wk, m, R) for m in range(n)) % R
        out[2 * n - 1 + k] = -g * wk * inv2n * delta % R
    return out
