"""Edge and uniform inputs for ANY 254-bit prime field of the project (Fr and Fq), as Python integers.

`edge_field(p)` generalises `fr_inputs.edge_fr` (which delegates here): the same positions for every modulus — the ends of the
field, its middle, 2^253, the borders of the three limb widths the kernels use (64-bit host limbs, 32-bit device limbs, 29-bit
lazy limbs), the same borders seen from p, all-ones low limbs under the top limb — followed by the positions that exist only for
the modulus given: for Fq, values in [r, q), which no list derived from Fr contains."""
import numpy as np

R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583


def common_positions(p: int) -> list:
    """the positions every modulus gets, in the order fr_inputs.edge_fr has always listed them"""
    half = (p - 1) // 2
    vals = [0, 1, 2, p - 1, p - 2, half - 1, half, half + 1, (1 << 253) - 1, 1 << 253, (1 << 253) + 1, (1 << 32) - 1]
    for w in (64, 32, 29):
        for k in range(1, 254 // w + 1):
            vals += [(1 << (w * k)) - 1, (1 << (w * k)) + 1]
    vals += [p - (1 << 64), p - (1 << 64) - 1, p - (1 << 128) + 1, p - (1 << 192) - 1]      # the same borders seen from p
    vals += [(1 << 253) | ((1 << 192) - 1), (p >> 64 << 64) - 1, p >> 64 << 64]           # all-ones low limbs under the top limb
    return _dedup(vals, p)


def modulus_positions(p: int) -> list:
    """positions that depend on the modulus itself: the low 32-bit and 29-bit limbs of p alone and their neighbours (where the
    final subtraction's borrow chain starts), p with one limb cleared, the Montgomery constants 2^256, 2^261 and 2^512 mod p and
    their negatives, and for Fq the whole gap [r, q) that an Fr-derived list never reaches"""
    vals = [p & 0xFFFFFFFF, (p & 0xFFFFFFFF) - 1, (p & 0xFFFFFFFF) + 1, p & ((1 << 29) - 1), p & ((1 << 64) - 1), p >> 32 << 32, (p >> 32 << 32) - 1,
            p - (1 << 32), p - (1 << 32) + 1, p - (1 << 29), p - (1 << 29) - 1, p - (1 << 224), p - (1 << 232) - 1]
    for k in range(8):
        vals.append(p & ~(0xFFFFFFFF << (32 * k)))                                          # p with 32-bit limb k cleared
    for e in (256, 261, 512):
        m = pow(2, e, p)
        vals += [m, p - m]
    if p > R_MOD:
        r, gap = R_MOD, p - R_MOD
        vals += [r, r + 1, r + 2, r + gap // 2, r + (1 << 64), r + (1 << 96) - 1, r + (1 << 126) + 1, p - 3, p - (1 << 100)]
    return _dedup(vals, p)


def _dedup(vals, p, seen=()):
    out = []
    for v in vals:
        assert 0 <= v < p, hex(v)
        if v not in out and v not in seen:
            out.append(v)
    return out


def edge_field(p: int) -> list:
    common = common_positions(p)
    return common + _dedup(modulus_positions(p), p, seen=common)


def rand_field(rng: np.random.Generator, n: int, p: int) -> list:
    """n Python integers uniform in [0, p): 254 random bits, redrawn while ≥ p"""
    out = []
    while len(out) < n:
        raw = rng.integers(0, 256, size=(2 * (n - len(out)) + 8, 32), dtype=np.uint8)
        raw[:, 31] &= 0x3F
        for row in raw:
            v = int.from_bytes(row.tobytes(), "little")
            if v < p and len(out) < n:
                out.append(v)
    return out


def ints_to_words(xs) -> np.ndarray:
    """integers below 2^256 → (n, 4) uint64 array of packed 32-byte little-endian words"""
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4).copy()


def words_to_ints(a: np.ndarray) -> list:
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1, 32)
    return [int.from_bytes(r.tobytes(), "little") for r in raw]
