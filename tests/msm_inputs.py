"""Scalar vectors for the MSM sweeps (tests/test_gpu_msm_plans.py, the prover's table path in tests/test_gpu_prove.py): the values
at which the signed-digit recoding of csrc/msm_recode.h can go wrong, for a GIVEN window geometry, planted where the digit sorts
change tiles.

A geometry is (c, W, wide): W windows, the first `wide` of them c bits wide at bit c·w, the others c − 1 bits wide at
c·wide + (c − 1)(w − wide) (MsmGeom, csrc/msm_plan.h).  `geometry(L, tab)` restates the host plan msm_geometry for automatic c;
tests/test_msm_recode_host.py holds it against the C++.  Plain helpers, Python integers and numpy (n, 4) uint64 arrays in standard
form — what the C ABI takes."""
import numpy as np

from fr_inputs import R_MOD, below_r, edge_fr, ints_to_arr, rand_fr_full

HALF = (R_MOD - 1) // 2
SORT_TILE, PA_SCALARS = 1024, 4096        # S2_TILE and PA_SCALARS of csrc/msm_sort.hip: scalars per workgroup of the digit sorts

# ---- the geometries the sweeps run (automatic c) -------------------------------------------------------------------------------
# table mode behind bn254_msm / bn254_g2_msm: L → (c, W, wide), the smallest L of every bracket
TABLE_GEOMS = {32768: (15, 17, 16), 32769: (16, 16, 14), 65537: (17, 15, 14), 262145: (19, 14, 2), 524289: (20, 13, 7)}
# the classic layout of the first call over those lengths …
TABLE_FIRST_CALL_GEOMS = {32768: (11, 24, 24), 32769: (12, 22, 22), 65537: (13, 20, 20), 262145: (15, 17, 16), 524289: (16, 16, 14)}
# … and of the classic sweep (host-resident bases)
CLASSIC_GEOMS = {257: (5, 51, 50), 1025: (7, 37, 37), 2049: (8, 32, 30), 4097: (9, 29, 29), 131073: (14, 19, 19)}
# the prover's witness tables (witness_table_geometry, csrc/prover/cache.cpp): wires → geometry
WITNESS_GEOMS = {33_002: (16, 16, 14), 262_202: (18, 15, 0)}


def _ilog2_ceil(x):
    l = 0
    while (1 << l) < x:
        l += 1
    return l


def _tab_low_bits(c, ib, W):
    for pb in (13, 14):
        low = max(0, (c - 1) - pb)
        if low <= 7 and ib + _ilog2_ceil(W) + low <= 31:
            return low
    return -1


def geometry(L, tab=0):
    """msm_geometry(L, 0, tab) for full-width scalars without precomputed bases, as a dict (c, W, wide, tab, NB, nbuckets); tab = 1:
    the table mode's own width, tab > 1: the table mode with digits of `tab` bits"""
    c = min(max(_ilog2_ceil(L or 1) - 4, 4), 16)
    if tab:
        ib, ct = _ilog2_ceil(L or 1), 0
        for t in range(min(c + 4, 20), c, -1):
            if _tab_low_bits(t, ib, 254 // t + 1) >= 0:
                ct = t
                break
        while ct > c + 1 and 254 // (ct - 1) + 1 == 254 // ct + 1:
            ct -= 1
        if 1 < tab <= 20 and _tab_low_bits(tab, ib, 254 // tab + 1) >= 0:
            ct = tab
        if ct:
            c = ct
        else:
            tab = 0
    W, NB = 254 // c + 1, 1 << (c - 1)
    spare = W * c - 254
    wide = W - min(spare, W) if c >= 5 and (tab or spare <= 3) else W
    return dict(c=c, W=W, wide=wide, tab=1 if tab else 0, NB=NB, nbuckets=NB if tab else W * NB)


def witness_geometry(wires):
    """witness_table_geometry(wires): the table width, narrowed while a bucket would hold fewer than 28 entries (never below 17)"""
    g = geometry(wires, 1)
    if not g["tab"]:
        return g
    c = g["c"]
    while c > 17 and ((wires * (254 // c + 1)) >> (c - 1)) < 28:
        c -= 1
    if c != g["c"]:
        h = geometry(wires, c)
        if h["tab"] and h["c"] == c:
            return h
    return g


# ---- windows, digits, edge values ----------------------------------------------------------------------------------------------
def windows(c, W, wide):
    """[(bit_w, cw)]: where window w starts and how wide it is"""
    return [(c * w, c) if w < wide else (c * wide + (c - 1) * (w - wide), c - 1) for w in range(W)]


def signed_digits(s, c, W, wide):
    """(neg, s', [d_w], rest) as the header of csrc/msm_sort.hip states the recoding: s above (r − 1)/2 is replaced by r − s,
    t = s' + H with H = Σ_w 2^(bit_w + cw − 1), d_w = ((t >> bit_w) & (2^cw − 1)) − 2^(cw − 1); rest = what t holds above the
    top window"""
    win = windows(c, W, wide)
    neg = s > HALF
    sp = R_MOD - s if neg else s
    t = sp + sum(1 << (b + cw - 1) for b, cw in win)
    digits = [((t >> b) & ((1 << cw) - 1)) - (1 << (cw - 1)) for b, cw in win]
    return neg, sp, digits, t >> (win[-1][0] + win[-1][1])


def window_edges(c, W, wide):
    """for every window, reduced mod r: 2^bit_w (digit 1 of window w alone: in table mode 2^bit_w·P is row w of the table),
    2^(bit_w + cw − 1) (digit −2^(cw − 1) — the last bucket — with a carry into the next window) and 2^(bit_w + cw − 1) − 1
    (all ones below); and r − v of each"""
    vals = []
    for b, cw in windows(c, W, wide):
        vals += [(1 << b) % R_MOD, (1 << (b + cw - 1)) % R_MOD, ((1 << (b + cw - 1)) - 1) % R_MOD]
    return vals + [(R_MOD - v) % R_MOD for v in vals]


def recode_limits():
    """the scalars of test_msm_edge_scalars (tests/test_gpu_ops.py): around the negation threshold, around 2^253, r − 1, all-ones
    low parts, and r − v of each"""
    vals = [HALF, HALF + 1, HALF - 1, (1 << 253) - 1, 1 << 253, (1 << 253) + 1, R_MOD - 1, R_MOD - 2, 1, 0, (1 << 252) - 1,
            (HALF >> 230 << 230) - 1, (1 << 240) - 1, ((1 << 253) - 1) ^ (1 << 19)]
    return vals + [(R_MOD - v) % R_MOD for v in vals]


def _geoms(geom):
    return [tuple(geom)] if isinstance(geom[0], int) else [tuple(g) for g in geom]


def edge_list(geom):
    """the values to plant for one geometry (c, W, wide) or several, in order: window edges of each geometry, fr_inputs.edge_fr(),
    recode_limits(); every value once"""
    vals = []
    for g in _geoms(geom):
        vals += window_edges(*g)
    vals += edge_fr() + recode_limits()
    seen, out = set(), []
    for v in vals:
        assert 0 <= v < R_MOD
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def edge_plan(L, geom, rot=0):
    """[(index, value)] of the planted entries: the edge list from index 0 onward, across 1023 | 1024 (the LDS-staged sort's tile),
    across 4095 | 4096 (the two-level sort's PA_SCALARS) and ending at L − 1; a stretch in the middle that would overlap its
    neighbours is left out (the one at the end then crosses the border, at the lengths the sweeps use).  `rot` rotates the list, a
    different amount per stretch, so that different values meet the borders; where the list is longer than the vector, one stretch
    of L values fills it and the caller covers the list with several `rot`."""
    E = edge_list(geom)
    n = len(E)
    if n >= L:
        return [(i, E[(rot + i) % n]) for i in range(L)]
    starts, end_start = [0], L - n
    for border in (SORT_TILE, PA_SCALARS):
        s = border - n // 2
        if s >= starts[-1] + n and s + n <= end_start:
            starts.append(s)
    if end_start >= starts[-1] + n:
        starts.append(end_start)
    return [(s + i, E[(rot + k * (n // 4 + 1) + i) % n]) for k, s in enumerate(starts) for i in range(n)]


def edge_vector(rng, L, geom, rot=0):
    """(L, 4) uint64: uniform over [0, r) with edge_plan(L, geom, rot) planted"""
    sc = rand_fr_full(rng, L)
    plan = edge_plan(L, geom, rot)
    sc[[i for i, _ in plan]] = ints_to_arr([v for _, v in plan])
    return sc


def skewed_vector(rng, L):
    """the mixture of test_msm_skewed_scalars (tests/test_gpu_ops.py) over the whole field: 4/10 zeros, 3/10 ones, 1/10 small bytes
    (2 … 9), 1/10 r − 1 and 1/10 dense in [0, r).  From 32768 scalars on at least 3·1024 entries equal 1 (a 3/10 share of 32768 is
    about 9800): bucket 0 — of window 0 in the classic layout — is then a large bucket of several 1024-entry work items."""
    sc = rand_fr_full(rng, L)
    kind = rng.integers(0, 10, size=L)
    sc[kind < 4] = 0
    sc[(kind >= 4) & (kind < 7)] = np.array([1, 0, 0, 0], dtype=np.uint64)
    small = kind == 7
    sc[small] = 0
    sc[small, 0] = rng.integers(2, 10, size=int(small.sum()), dtype=np.uint64)
    sc[kind == 8] = ints_to_arr([R_MOD - 1])[0]
    ones = int(((sc[:, 0] == 1) & ~sc[:, 1:].any(axis=1)).sum())
    assert L < 32768 or ones >= 3 * 1024, (L, ones)
    return sc
