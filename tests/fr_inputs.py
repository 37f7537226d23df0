"""BN254 scalar-field inputs for the GPU tests that cover the WHOLE field.

The generators of the older tests (`rand_fr` in test_gpu_ops.py and friends) mask the top limb to 61 bits: every value they
produce is below 2^253, while r ≈ 2^253.6 — about a third of the field never reaches the kernels.  The helpers here draw
uniformly from [0, r) and list the values where limb arithmetic goes wrong.  Arrays are numpy uint64 of shape (n, 4),
little-endian limbs, standard form — what the C ABI takes."""
import numpy as np

from field_inputs import common_positions

R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
_R_LIMBS = [np.uint64((R_MOD >> (64 * k)) & ((1 << 64) - 1)) for k in range(4)]


def below_r(a: np.ndarray) -> np.ndarray:
    """boolean mask: a[i] < r, compared limb by limb from the top"""
    lt = np.zeros(len(a), dtype=bool)
    eq = np.ones(len(a), dtype=bool)
    for k in (3, 2, 1, 0):
        lt |= eq & (a[:, k] < _R_LIMBS[k])
        eq &= a[:, k] == _R_LIMBS[k]
    return lt


def rand_fr_full(rng: np.random.Generator, n: int) -> np.ndarray:
    """n values uniform in [0, r): 254 random bits each, redrawn while ≥ r (about one draw in four is)"""
    out = np.empty((n, 4), dtype=np.uint64)
    todo = np.arange(n)
    while len(todo):
        a = rng.integers(0, (1 << 64) - 1, size=(len(todo), 4), dtype=np.uint64, endpoint=True)
        a[:, 3] &= np.uint64((1 << 62) - 1)
        ok = below_r(a)
        out[todo[ok]] = a[ok]
        todo = todo[~ok]
    return out


def edge_fr() -> list:
    """Python integers in [0, r) at the places where carries, borrows, the final subtraction of r and the signed recodings
    change behaviour: the ends of the field, its middle, 2^253 (the first bit the older generators never set), and the
    boundaries of the three limb widths the kernels use (64-bit host limbs, 32-bit device limbs, 29-bit lazy limbs)."""
    return common_positions(R_MOD)   # the list is pinned by tests/test_fr_inputs.py; other moduli: field_inputs.edge_field


def ints_to_arr(xs) -> np.ndarray:
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4).copy()


def edge_fr_arr() -> np.ndarray:
    return ints_to_arr(edge_fr())
