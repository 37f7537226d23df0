"""The rest of the ICICLE surface the wrapper crate binds, through the C ABI on the GPU against
Python-integer / oracle results: vec ops (div, accumulate, Σ, Π, scalar∘vector, batches in both layouts), projective
Montgomery conversion, NTT orderings (kNR/kRN/kRR/kNM/kMN) and columns_batch, batched MSM and msm_precompute_bases.
Semantics follow icicle/backend/cpu/src/field/cpu_vec_ops.cpp, icicle/include/icicle/ntt.h:32-43 and msm.h:21-53."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DIMS = {"g1": (2, 3), "g2": (4, 6)}


def rand_fr(rng, n):
    raw = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    raw[:, 3] &= np.uint64((1 << 61) - 1)
    return raw


def test_vec_div_accumulate_and_reductions(gpu, O):
    K, R = gpu, O.R_MOD
    rng = np.random.default_rng(5)
    n = 3000
    a, b = rand_fr(rng, n), rand_fr(rng, n)
    b[7] = 0                                           # inverse(0) = 0 in the reference ⇒ a/0 = 0
    ai, bi = O.arr_to_ints(a), O.arr_to_ints(b)
    want = [x * pow(y, R - 2, R) % R for x, y in zip(ai, bi)]
    assert np.array_equal(K.vec_op2("div", a, b), O.ints_to_arr(want))
    d = K.DeviceVec.from_host(a)
    K.accumulate_scalars(d, b)
    assert np.array_equal(d.to_host(a.shape), O.ints_to_arr([(x + y) % R for x, y in zip(ai, bi)]))
    d.free()
    for batch, cols in ((1, False), (3, False), (3, True)):
        size = n // batch
        v = a[:size * batch]
        vi = ai[:size * batch]
        rows = [[vi[(bb + i * batch) if cols else (bb * size + i)] for i in range(size)] for bb in range(batch)]
        s = K.reduce_scalars("sum", v, batch_size=batch, columns_batch=cols)
        assert np.array_equal(s, O.ints_to_arr([sum(r) % R for r in rows]))
        p = K.reduce_scalars("product", v, batch_size=batch, columns_batch=cols)
        prods = []
        for r in rows:
            acc = 1
            for x in r:
                acc = acc * x % R
            prods.append(acc)
        assert np.array_equal(p, O.ints_to_arr(prods))
    # a long vector (two-stage reduction, device resident)
    big = rand_fr(rng, 1 << 17)
    dv = K.DeviceVec.from_host(big)
    assert np.array_equal(K.reduce_scalars("sum", dv), O.ints_to_arr([sum(O.arr_to_ints(big)) % R]))
    dv.free()


@pytest.mark.parametrize("cols", [False, True])
def test_scalar_vector_ops(gpu, O, cols):
    K, R = gpu, O.R_MOD
    rng = np.random.default_rng(11)
    batch, size = 4, 257
    v, sc = rand_fr(rng, batch * size), rand_fr(rng, batch)
    vi, si = O.arr_to_ints(v), O.arr_to_ints(sc)
    for name, f in (("add", lambda s, x: (s + x) % R), ("sub", lambda s, x: (s - x) % R), ("mul", lambda s, x: s * x % R)):
        want = [f(si[(k % batch) if cols else (k // size)], x) for k, x in enumerate(vi)]
        assert np.array_equal(K.scalar_vec_op(name, sc, v, batch_size=batch, columns_batch=cols), O.ints_to_arr(want)), name
    # element-wise ops are layout-agnostic: batch 4 in columns layout equals the flat result
    assert np.array_equal(K.vec_op2("mul", v, v, batch_size=batch, columns_batch=cols), K.mul_scalars(v, v))


@pytest.mark.parametrize("grp", ["g1", "g2"])
def test_projective_convert_montgomery(gpu, O, grp):
    K = gpu
    gen = K.ec(grp, "generator")
    pts = np.stack([K.ec(grp, "mul_scalar", gen, k) for k in (1, 2, 12345)])
    m = K.projective_convert_montgomery(grp, pts, True)
    assert np.array_equal(m.reshape(-1, 4), O.fq_convert_montgomery(pts.reshape(-1, 4), True))
    assert np.array_equal(K.projective_convert_montgomery(grp, m, False), pts)


def _bitrev(x, logn):
    idx = np.array([int(format(i, f"0{logn}b")[::-1], 2) if logn else 0 for i in range(1 << logn)])
    return x[idx]


@pytest.mark.parametrize("logn", [3, 10, 12])
def test_ntt_orderings_and_columns_batch(gpu, O, logn):
    K = gpu
    K.release_domain()
    K.initialize_domain(K.get_root_of_unity(1 << 13))
    rng = np.random.default_rng(logn)
    n = 1 << logn
    x = rand_fr(rng, n)
    NN, NR, RN, RR, NM, MN = range(6)
    for inverse in (False, True):
        want = O.fr_ntt(x, inverse, domain_log=13)
        assert np.array_equal(K.ntt(x, inverse, ordering=NR), _bitrev(want, logn))
        assert np.array_equal(K.ntt(_bitrev(x, logn), inverse, ordering=RN), want)
        assert np.array_equal(K.ntt(_bitrev(x, logn), inverse, ordering=RR), _bitrev(want, logn))
        assert np.array_equal(K.ntt(x, inverse, ordering=NM), _bitrev(want, logn))       # radix-2 convention: M = R
        assert np.array_equal(K.ntt(_bitrev(x, logn), inverse, ordering=MN), want)
    # NR then RN round-trips without any reordering by the caller (the use the mixed orders exist for)
    assert np.array_equal(K.ntt(K.ntt(x, False, ordering=NM), True, ordering=MN), x)
    # columns_batch: element i of batch b at b + i·batch
    batch = 3
    xb = rand_fr(rng, batch * n)
    rows = O.fr_ntt(xb, False, batch=batch, domain_log=13).reshape(batch, n, 4)
    cols_in = np.ascontiguousarray(xb.reshape(batch, n, 4).transpose(1, 0, 2)).reshape(-1, 4)
    got = K.ntt(cols_in, False, batch_size=batch, columns_batch=True).reshape(n, batch, 4)
    assert np.array_equal(got.transpose(1, 0, 2), rows)
    d = K.DeviceVec.from_host(cols_in)                                                      # in place, on device, reversed output
    K.ntt(d, False, batch_size=batch, columns_batch=True, ordering=NR)
    got = d.to_host((n, batch, 4)).transpose(1, 0, 2)
    assert np.array_equal(got, np.stack([_bitrev(r, logn) for r in rows]))
    d.free()
    with pytest.raises(K.IcicleError):
        K.ntt(x, False, ordering=9)
    K.release_domain()


@pytest.mark.parametrize("grp", ["g1", "g2"])
def test_msm_batch_and_precompute(gpu, O, grp):
    K = gpu
    rng = np.random.default_rng(21 if grp == "g1" else 22)
    n, batch = 700, 3
    G = O.ec_to_affine(grp, O.ec_generator(grp))
    bases = O.fixed_base_mul(grp, G, rand_fr(rng, n))
    bases[5] = 0
    sc = rand_fr(rng, batch * n)
    want = [O.ec_to_affine(grp, O.msm(grp, sc[b * n:(b + 1) * n], bases)) for b in range(batch)]
    res = K.msm(grp, sc, bases, batch_size=batch, shared_points=True)
    for b in range(batch):
        assert np.array_equal(K.ec(grp, "to_affine", res[b]), want[b])
    # one base set per batch element
    bases2 = np.concatenate([bases, bases[::-1], bases])
    res = K.msm(grp, sc, bases2, batch_size=batch, shared_points=False)
    assert np.array_equal(K.ec(grp, "to_affine", res[0]), want[0])
    assert np.array_equal(K.ec(grp, "to_affine", res[1]), O.ec_to_affine(grp, O.msm(grp, sc[n:2 * n], bases[::-1].copy())))
    # precomputed bases: [f·i + j] = 2^(j·shift)·P_i ; an MSM over them gives the same result
    f = 3
    pre = K.msm_precompute_bases(grp, bases, f, c=0)
    assert pre.shape[0] == f * n and np.array_equal(pre[0::f], bases)
    c = max(4, min(16, int(np.ceil(np.log2(n))) - 4))
    shift = c * (((254 // c + 1) + f - 1) // f)
    for i in (0, 5, 17, n - 1):
        p = O.ec_from_affine(grp, bases[i])
        for j in range(1, f):
            p = O.ec_mul_scalar(grp, p, 1 << shift)
            assert np.array_equal(pre[f * i + j], O.ec_to_affine(grp, p)), (i, j)
    res = K.msm(grp, sc[:n], pre, size=n, precompute_factor=f)
    assert np.array_equal(K.ec(grp, "to_affine", res), want[0])
    # Montgomery-form bases in and out
    bm = O.fq_convert_montgomery(bases.reshape(-1, 4), True).reshape(bases.shape)
    prem = K.msm_precompute_bases(grp, bm, f, points_mont=True)
    assert np.array_equal(O.fq_convert_montgomery(prem.reshape(-1, 4), False).reshape(pre.shape), pre)


@pytest.mark.parametrize("grp", ["g1", "g2"])
def test_msm_bitsize_and_precompute_factor_semantics(gpu, O, grp):
    """MSMConfig.bitsize (msm.h:32-34: scalars below 2^bitsize → fewer windows) and precompute_factor > 1 read through
    every precomputed multiple (window w uses multiple w / nbms, bucket set w mod nbms — icicle/src/msm.cpp:45-72,
    cuda_msm.cuh:186-203): same group element as the plain MSM, for several (c, f, bitsize)."""
    K = gpu
    rng = np.random.default_rng(31 if grp == "g1" else 32)
    n = 3000
    G = O.ec_to_affine(grp, O.ec_generator(grp))
    bases = O.fixed_base_mul(grp, G, rand_fr(rng, n))
    bases[7] = 0
    sc = rand_fr(rng, n)
    sc[0] = 0
    sc[1, :] = np.frombuffer((O.R_MOD - 1).to_bytes(32, "little"), dtype=np.uint64)
    want = O.ec_to_affine(grp, O.msm(grp, sc, bases))
    for c, f in ((0, 2), (0, 4), (10, 3), (13, 7), (5, 64)):
        pre = K.msm_precompute_bases(grp, bases, f, c=c)
        got = K.ec(grp, "to_affine", K.msm(grp, sc, pre, size=n, precompute_factor=f, c=c))
        assert np.array_equal(got, want), (c, f)
    # short scalars: 64-bit and 100-bit, with the maximum value present
    for bits in (1, 64, 100, 253):
        s2 = sc.copy()
        if bits <= 64:
            s2[:, 1:] = 0
            s2[:, 0] &= np.uint64((1 << bits) - 1)
            s2[2, 0] = np.uint64((1 << bits) - 1)
        elif bits == 100:
            s2[:, 2:] = 0
            s2[:, 1] &= np.uint64((1 << 36) - 1)
            s2[2, 0], s2[2, 1] = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64((1 << 36) - 1)
        else:
            s2[:, 3] &= np.uint64((1 << 61) - 1)
            s2[1] = 0
        w2 = O.ec_to_affine(grp, O.msm(grp, s2, bases))
        for c in (0, 9):
            got = K.ec(grp, "to_affine", K.msm(grp, s2, bases, bitsize=bits, c=c))
            assert np.array_equal(got, w2), (bits, c)
        if bits in (64, 100):
            f = 3
            pre = K.msm_precompute_bases(grp, bases, f, bitsize=bits)
            got = K.ec(grp, "to_affine", K.msm(grp, s2, pre, size=n, precompute_factor=f, bitsize=bits))
            assert np.array_equal(got, w2), (bits, "precompute")
    with pytest.raises(K.IcicleError):
        K.msm(grp, sc, bases, bitsize=300)


# ------------------------------------------------------------------------------------------------------------------------------
# The same entry points over the WHOLE field: every generator above stays below 2^253, so the values where limb arithmetic goes
# wrong (tests/fr_inputs.py, tests/field_inputs.py) never reached div, accumulate, the scalar∘vector ops, the reductions or the
# Fq conversions of points.  Expected values are Python integers.
# ------------------------------------------------------------------------------------------------------------------------------
import ctypes as C   # noqa: E402

from field_inputs import Q_MOD, edge_field, rand_field   # noqa: E402
from fr_inputs import R_MOD, edge_fr, ints_to_arr, rand_fr_full   # noqa: E402


def _edge_cross(rng, extra):
    """(a, b) as arrays and integer lists: the cross product of the Fr edge list with itself, then `extra` uniform pairs"""
    e = edge_fr()
    ra, rb = rand_fr_full(rng, extra), rand_fr_full(rng, extra)
    a = np.concatenate([ints_to_arr([x for x in e for _ in e]), ra])
    b = np.concatenate([ints_to_arr([y for _ in e for y in e]), rb])
    assert len(a) % 256
    return a, b


def test_vec_div_and_accumulate_over_the_whole_field(gpu, O):
    K, R = gpu, R_MOD
    a, b = _edge_cross(np.random.default_rng(41), 2000)
    ai, bi = O.arr_to_ints(a), O.arr_to_ints(b)
    assert sum(y == 0 for y in bi) >= 48 and any(x == 0 and y == 0 for x, y in zip(ai, bi))       # zero divisors, 0/0 among them
    want_div = O.ints_to_arr([x * (pow(y, -1, R) if y else 0) % R for x, y in zip(ai, bi)])
    want_acc = O.ints_to_arr([(x + y) % R for x, y in zip(ai, bi)])
    assert np.array_equal(K.vec_op2("div", a, b), want_div)
    da, db = K.DeviceVec.from_host(a), K.DeviceVec.from_host(b)
    K.vec_op2("div", da, db, out=da)                                                            # device resident, in place
    assert np.array_equal(da.to_host(a.shape), want_div)
    host = a.copy()
    K.accumulate_scalars(host, b)                                                               # host resident, in place
    assert np.array_equal(host, want_acc)
    da.copy_from_host(a)
    K.accumulate_scalars(da, db)
    assert np.array_equal(da.to_host(a.shape), want_acc)
    da.free()
    db.free()


@pytest.mark.parametrize("cols", [False, True])
def test_scalar_vector_ops_over_the_whole_field(gpu, O, cols):
    """one edge value per batch row as the scalar, the whole edge list and uniform values as its vector: the cross product"""
    K, R = gpu, R_MOD
    e = edge_fr()
    batch, size = len(e), len(e) + 37
    rows = [e + O.arr_to_ints(rand_fr_full(np.random.default_rng(50 + b), 37)) for b in range(batch)]
    flat = [rows[k % batch][k // batch] if cols else rows[k // size][k % size] for k in range(batch * size)]
    v, sc = ints_to_arr(flat), ints_to_arr(e)
    for name, f in (("add", lambda s, x: (s + x) % R), ("sub", lambda s, x: (s - x) % R), ("mul", lambda s, x: s * x % R)):
        want = O.ints_to_arr([f(e[(k % batch) if cols else (k // size)], x) for k, x in enumerate(flat)])
        assert np.array_equal(K.scalar_vec_op(name, sc, v, batch_size=batch, columns_batch=cols), want), name
        dv, ds = K.DeviceVec.from_host(v), K.DeviceVec.from_host(sc)
        K.scalar_vec_op(name, ds, dv, batch_size=batch, columns_batch=cols, out=dv)             # device resident, in place
        assert np.array_equal(dv.to_host(v.shape), want), name + " (device, in place)"
        dv.free()
        ds.free()


def _reduce_direct(K, name, v, size, batch, cols, on_device):
    """bn254_vector_{sum,product} called directly: input and RESULT both host resident or both device resident"""
    cfg = K.VecOpsConfig.default()
    cfg.is_a_on_device = cfg.is_result_on_device = on_device
    cfg.batch_size, cfg.columns_batch = batch, cols
    fn = getattr(K.lib(), "bn254_vector_" + name)
    if not on_device:
        out = np.zeros((batch, 4), dtype=np.uint64)
        K.check(fn(K.ptr_of(v), C.c_uint64(size), C.byref(cfg), K.ptr_of(out)), name)
        return out
    dv, dout = K.DeviceVec.from_host(v), K.DeviceVec(32 * batch)
    K.check(fn(K.ptr_of(dv), C.c_uint64(size), C.byref(cfg), K.ptr_of(dout)), name)
    out = dout.to_host((batch, 4))
    dv.free()
    dout.free()
    return out


@pytest.mark.parametrize("size", [1, 255, 256, 257, 4096, 4097, 4096 * 3 + 5])
def test_reductions_sizes_layouts_and_residency(gpu, O, size):
    """Σ and Π at one chunk, the chunk border and several chunks, batch 1 and 3 in both layouts, result on the host and on the
    device, over uniform values of [0, r) with r − 1 and 0 planted"""
    K, R = gpu, R_MOD
    for batch in (1, 3):
        rows = [O.arr_to_ints(rand_fr_full(np.random.default_rng(1000 * batch + size + b), size)) for b in range(batch)]
        for r in rows:
            r[0] = r[-1] = R - 1
        zrows = [list(r) for r in rows]
        zrows[-1][size // 2] = 0
        if size > 2:
            zrows[0][1] = 0                                                                      # Σ sees a zero in the first row as well
        want = {}
        for tag, rr in (("v", rows), ("z", zrows)):
            prods = []
            for r in rr:
                acc = 1
                for x in r:
                    acc = acc * x % R
                prods.append(acc)
            want[tag] = (O.ints_to_arr([sum(r) % R for r in rr]), O.ints_to_arr(prods))
        assert all(int(x) for x in O.arr_to_ints(want["v"][1]))                                   # Π of the zero-free rows is not trivially 0
        for cols in (False, True):
            for tag, rr in (("v", rows), ("z", zrows)):
                flat = [rr[k % batch][k // batch] if cols else rr[k // size][k % size] for k in range(batch * size)]
                v = ints_to_arr(flat)
                for on_device in (False, True):
                    where = (size, batch, cols, tag, on_device)
                    assert np.array_equal(_reduce_direct(K, "sum", v, size, batch, cols, on_device), want[tag][0]), ("sum",) + where
                    assert np.array_equal(_reduce_direct(K, "product", v, size, batch, cols, on_device), want[tag][1]), ("product",) + where


@pytest.mark.parametrize("name,words", [("bn254_affine_convert_montgomery", 2), ("bn254_g2_affine_convert_montgomery", 4),
                                        ("bn254_projective_convert_montgomery", 3), ("bn254_g2_projective_convert_montgomery", 6)])
def test_point_montgomery_conversions_are_fq_conversions_over_the_whole_field(gpu, O, name, words):
    """the point conversions are coordinate-wise Fq conversions: the Fq edge list (with the values of [r, q)) and 4096 uniform
    values of [0, q) as coordinates, both directions, host resident and device resident in place"""
    K = gpu
    vals = edge_field(Q_MOD) + rand_field(np.random.default_rng(61), 4096, Q_MOD)
    vals += edge_field(Q_MOD)[:-len(vals) % 12]                                                  # whole points for every layout
    assert len(vals) % words == 0 and any(R_MOD <= v < Q_MOD for v in vals) and Q_MOD - 1 in vals
    a = ints_to_arr(vals)
    fn = getattr(K.lib(), name)
    for to_mont, factor in ((True, 1 << 256), (False, pow(1 << 256, -1, Q_MOD))):
        want = ints_to_arr([v * factor % Q_MOD for v in vals])
        cfg = K.VecOpsConfig.default()
        out = np.zeros_like(a)
        K.check(fn(K.ptr_of(a), C.c_uint64(len(vals) // words), C.c_bool(to_mont), C.byref(cfg), K.ptr_of(out)), name)
        assert np.array_equal(out, want), (name, to_mont)
        d = K.DeviceVec.from_host(a)
        cfg.is_a_on_device = cfg.is_result_on_device = True
        K.check(fn(K.ptr_of(d), C.c_uint64(len(vals) // words), C.c_bool(to_mont), C.byref(cfg), K.ptr_of(d)), name)
        assert np.array_equal(d.to_host(a.shape), want), (name, to_mont, "device, in place")
        d.free()
