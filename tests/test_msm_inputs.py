"""tests/msm_inputs.py against Python integers (no GPU): the geometries the MSM sweeps name are what the restated host plan gives,
every planted value recodes exactly in every one of them — the signed digits, taken as the header of csrc/msm_sort.hip states
them, sum to s', stay within their window and leave nothing above the top window — and the vectors hold what they promise where
they promise it."""
import numpy as np
import pytest

import msm_inputs as MI
from fr_inputs import R_MOD, ints_to_arr

GEOMS = sorted(set(MI.TABLE_GEOMS.values()) | set(MI.TABLE_FIRST_CALL_GEOMS.values()) | set(MI.CLASSIC_GEOMS.values()) | set(MI.WITNESS_GEOMS.values()))
# (L, geometries whose edges are planted, rotations) of every edge vector the GPU sweeps draw
SWEEP_VECTORS = [(L, [MI.TABLE_GEOMS[L], MI.TABLE_FIRST_CALL_GEOMS[L]], (0,)) for L in MI.TABLE_GEOMS] + \
                [(L, [g], (0, L)) for L, g in MI.CLASSIC_GEOMS.items()] + [(n, [g], (0,)) for n, g in MI.WITNESS_GEOMS.items()]


def test_the_named_geometries_are_the_plan_s():
    for L, (c, W, wide) in MI.TABLE_GEOMS.items():
        g = MI.geometry(L, 1)
        assert (g["tab"], g["c"], g["W"], g["wide"], g["nbuckets"]) == (1, c, W, wide, 1 << (c - 1)), L
        if L > 32768:
            assert MI.geometry(L - 1, 1)["c"] != c, L                      # the smallest length of its bracket
    for table in (MI.TABLE_FIRST_CALL_GEOMS, MI.CLASSIC_GEOMS):
        for L, (c, W, wide) in table.items():
            g = MI.geometry(L)
            assert (g["tab"], g["c"], g["W"], g["wide"], g["nbuckets"]) == (0, c, W, wide, W << (c - 1)), L
    for wires, (c, W, wide) in MI.WITNESS_GEOMS.items():
        g = MI.witness_geometry(wires)
        assert (g["tab"], g["c"], g["W"], g["wide"]) == (1, c, W, wide), wires
    # narrowed top windows in the classic layout at c = 5, 8, 15, 16; every window narrowed in one witness geometry
    assert {c: W - wide for c, W, wide in set(MI.CLASSIC_GEOMS.values()) | set(MI.TABLE_FIRST_CALL_GEOMS.values())} == \
        {5: 1, 7: 0, 8: 2, 9: 0, 11: 0, 12: 0, 13: 0, 14: 0, 15: 1, 16: 2}
    assert any(wide == 0 and W * (c - 1) >= 254 for c, W, wide in MI.WITNESS_GEOMS.values())


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "c%d_W%d_wide%d" % g)
def test_windows_tile_the_scalar(geom):
    c, W, wide = geom
    win = MI.windows(c, W, wide)
    assert len(win) == W and win[0][0] == 0
    for (b0, w0), (b1, _) in zip(win, win[1:]):
        assert b1 == b0 + w0                                                # no gap, no overlap
    assert all(cw == (c if w < wide else c - 1) for w, (_, cw) in enumerate(win))
    top = win[-1][0] + win[-1][1]
    assert top >= 254                                                       # the windows cover the scalar
    if wide < W:
        assert top == 254 or wide == 0                                      # narrowed: they tile the 254 bits exactly (or every window is narrow)


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "c%d_W%d_wide%d" % g)
def test_every_planted_value_recodes_exactly(geom):
    c, W, wide = geom
    win = MI.windows(c, W, wide)
    vals = set(MI.edge_list(geom))
    for L, geoms, _ in SWEEP_VECTORS:                                       # the lists this geometry meets in the sweeps (edges of a neighbour's windows)
        if geom in geoms:
            vals |= set(MI.edge_list(geoms))
    assert {0, 1, R_MOD - 1, MI.HALF, MI.HALF + 1, 1 << 253} <= vals
    extremes = set()
    for s in sorted(vals):
        neg, sp, digits, rest = MI.signed_digits(s, c, W, wide)
        assert neg == (s > MI.HALF) and sp == (R_MOD - s if neg else s) and sp <= MI.HALF
        assert sum(d << b for d, (b, _) in zip(digits, win)) == sp, hex(s)
        assert all(abs(d) <= 1 << (cw - 1) for d, (_, cw) in zip(digits, win)), hex(s)
        assert rest == 0, hex(s)
        extremes |= {w for w, (d, (_, cw)) in enumerate(zip(digits, win)) if d == -(1 << (cw - 1))}
    # 2^(bit_w + cw − 1) ≤ 2^252 is below (r − 1)/2 and recoded as it stands: window w then holds −2^(cw − 1), the last bucket
    assert extremes >= {w for w, (b, cw) in enumerate(win) if b + cw - 1 <= 252}


def test_window_edges_are_what_they_are_called():
    for c, W, wide in GEOMS:
        win = MI.windows(c, W, wide)
        e = MI.window_edges(c, W, wide)
        assert len(e) == 6 * W
        for w, (b, cw) in enumerate(win):
            one, last, ones = e[3 * w: 3 * w + 3]
            assert (one, last, ones) == ((1 << b) % R_MOD, (1 << (b + cw - 1)) % R_MOD, ((1 << (b + cw - 1)) - 1) % R_MOD)
            assert e[3 * W + 3 * w: 3 * W + 3 * w + 3] == [(R_MOD - v) % R_MOD for v in (one, last, ones)]
            if b + cw - 1 < 253:                                             # below (r − 1)/2: recoded as it stands
                d = MI.signed_digits(one, c, W, wide)[2]
                assert d[w] == 1 and not any(d[:w] + d[w + 1:])
                d = MI.signed_digits(last, c, W, wide)[2]
                assert d[w] == -(1 << (cw - 1)) and d[w + 1] == 1 and not any(d[:w] + d[w + 2:])
                d = MI.signed_digits(ones, c, W, wide)[2]
                if w == 0:
                    assert d[0] == (1 << (cw - 1)) - 1 and not any(d[1:])
                else:                                                        # −1 at the bottom, and the carry runs up to window w
                    assert d[0] == -1 and d[w] == -(1 << (cw - 1)) and d[w + 1] == 1 and not any(d[1:w] + d[w + 2:])


@pytest.mark.parametrize("L,geoms,rots", SWEEP_VECTORS, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_planted_positions_survive(L, geoms, rots):
    E = MI.edge_list(geoms)
    seen = set()
    for rot in rots:
        plan = MI.edge_plan(L, geoms, rot)
        idx = [i for i, _ in plan]
        assert len(set(idx)) == len(idx) and 0 <= min(idx) and max(idx) < L
        assert {0, L - 1} <= set(idx)
        for border in (MI.SORT_TILE, MI.PA_SCALARS):
            if L > border:
                assert {border - 1, border} <= set(idx), (L, border)
        sc = MI.edge_vector(np.random.default_rng(L + rot), L, geoms, rot)
        assert sc.shape == (L, 4) and sc.dtype == np.uint64
        assert np.array_equal(sc[idx], ints_to_arr([v for _, v in plan]))
        seen |= {v for _, v in plan}
        if len(E) < L:
            rest = np.delete(sc, idx, axis=0)                               # the filling covers the whole field
            assert (rest[:, 3] >> np.uint64(61)).any() and MI.below_r(rest).all()
    assert seen == set(E), (L, len(E), len(seen))                           # every value is in some vector of the sweep


def test_skewed_vector():
    for L in (257, 4097, 32768, 65537):
        sc = MI.skewed_vector(np.random.default_rng(L), L)
        assert MI.below_r(sc).all()
        ones = int(((sc[:, 0] == 1) & ~sc[:, 1:].any(axis=1)).sum())
        zeros = int((~sc.any(axis=1)).sum())
        rm1 = int((sc == ints_to_arr([R_MOD - 1])[0]).all(axis=1).sum())
        assert ones > L // 5 and zeros > L // 4 and rm1 > L // 20
        if L >= 32768:
            assert ones >= 3 * 1024
            assert (sc[:, 3] >> np.uint64(61)).any()                        # the dense share reaches above 2^253
