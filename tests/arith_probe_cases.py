"""Input lists, runners and comparisons shared by tests/test_arith_probe_host.py (CPU twin) and tests/test_gpu_arith_probe.py
(device kernels) for the probes of tests/arith_probe.hip.  A case names the probe(s) it runs, one tuple of input words per
lane, and a check of the raw output words against tests/arith_probe_model.py; only the runner differs between the two tests."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import arith_probe_model as M
from conftest import ROOT
from field_inputs import Q_MOD, R_MOD, edge_field, ints_to_words, rand_field, words_to_ints

CHAIN = 200          # x_madd steps per lane of the chain probes (arith_probe.hip: CHAIN)
CHAIN_LANES = 128

# probe → (input words, output words) per lane; W = words per coordinate (1 for G1, 2 for G2)
SHAPES = {}
for _f in ("fr", "fq"):
    for _op, _n in (("add", 2), ("sub", 2), ("neg", 1), ("dbl", 1), ("mul3", 1), ("mul", 2), ("sqr", 1), ("mul2sum", 4), ("to_mont", 1),
                    ("from_mont", 1), ("inv", 1), ("reduce_once", 1), ("is_canonical", 1)):
        SHAPES[f"{_f}_{_op}"] = (_n, 1)
for _op, _n in (("from_std", 1), ("from_mont256", 1), ("pack_canon_unpack", 1), ("mul", 2), ("sqr", 1), ("mul2", 4), ("mul4", 4), ("sub31", 2),
                ("sub53", 3), ("sqr_lazy", 2), ("inv", 1), ("inv_ds", 1), ("inv_ds_lazy", 2), ("zero_tests", 2)):
    SHAPES[f"f29_{_op}"] = (_n, 1)
for _op, _n, _m in (("from_std", 1, 1), ("from_mont256", 1, 1), ("pack_canon_unpack", 1, 1), ("mul", 2, 1), ("mul_lazy", 4, 1), ("sub2", 2, 1),
                    ("sub1300", 2, 2)):
    SHAPES[f"fr29_{_op}"] = (_n, _m)
for _f, _g, _w in (("fqops", "g1", 1), ("fq2", "g2", 2)):
    for _op, _n in (("add", 2), ("sub", 2), ("neg", 1), ("dbl", 1), ("mul", 2), ("sqr", 1), ("inv", 1), ("mul_sub_mul", 4)):
        SHAPES[f"{_f}_{_op}"] = (_n * _w, _w)
    for _op, _n, _m in (("x_madd", 6, 4), ("x_add", 8, 4), ("x_dbl", 4, 4), ("x_dbl_affine", 2, 4), ("x_proj_roundtrip", 3, 3), ("p_add", 7, 3),
                        ("p_dbl", 4, 3), ("p_to_affine", 3, 2)):
        SHAPES[f"{_g}_{_op}"] = (_n * _w, _m * _w)
    SHAPES[f"{_g}_p_eq"] = (6 * _w, 1)
    for _form in ("std", "mont256", "internal"):
        SHAPES[f"{_g}l_load_affine_{_form}"] = SHAPES[f"{_g}l_load_affine_{_form}_neg"] = (2 * _w, 2 * _w)
    for _op, _n, _m in (("x_madd", 6, 4), ("x_add", 8, 4), ("x_dbl", 4, 4), ("x_dbl_affine_exact", 2, 4), ("x_from_old", 4, 4), ("x_internal_roundtrip", 4, 8)):
        SHAPES[f"{_g}l_{_op}"] = (_n * _w, _m * _w)
    SHAPES[f"{_g}l_chain"] = (CHAIN * (2 * _w + 1), 8 * _w)

LAZY_PREFIXES = ("f29_", "g1l_", "g2l_")     # probes whose host twin also runs in the bound-checked (-DF29_CHECK) build
FQ2_PREFIXES = ("fq2_", "g2_")               # probes the device library holds twice (out-of-line and inlined Fq2Ops::mul / sqr)


# ------------------------------------------------------------------------------------------------ runners
def _call(fn, op, lanes):
    nin, nout = SHAPES[op]
    n = len(lanes)
    flat = [w for lane in lanes for w in lane]
    assert len(flat) == n * nin, (op, len(flat), n, nin)
    a = ints_to_words(flat)
    out = np.zeros((n * nout, 4), dtype=np.uint64)
    rc = fn(a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_int(n))
    assert rc == 0, f"{op}: the runner returned {rc}"
    w = words_to_ints(out)
    return [tuple(w[i * nout:(i + 1) * nout]) for i in range(n)]


@functools.lru_cache(maxsize=None)
def host_lib(checked: bool):
    """the host twin, compiled like tests/test_f29.py compiles f29_check.so"""
    out = os.path.join(ROOT, "build", "arith_probe_host_chk.so" if checked else "arith_probe_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-x", "c++", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "arith_probe.hip")]
    subprocess.run(cmd + (["-DF29_CHECK"] if checked else []), check=True)
    lib = C.CDLL(out)
    if checked:
        lib.probe_check_failure.restype = C.c_char_p
    return lib


def run_host(op, lanes, variant=""):
    out = _call(getattr(host_lib(False), f"probe_{op}_host"), op, lanes)
    if op.startswith(LAZY_PREFIXES):
        chk = host_lib(True)
        chk.probe_check_reset()
        again = _call(getattr(chk, f"probe_{op}_host"), op, lanes)
        why = chk.probe_check_failure()
        assert why is None, f"{op}: a bound stated in ff29.h / ec29.h does not hold on these inputs: {why.decode()}"
        assert again == out, f"{op}: the checked and the plain host build disagree"
    return out


@functools.lru_cache(maxsize=None)
def device_lib():
    path = os.path.join(ROOT, "icicle-snark_amd", "lib", "libisnark_arith_probe.so")
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: run `make` (hipcc --offload-arch=gfx950)")
    return C.CDLL(path)


def run_device(op, lanes, variant=""):
    return _call(getattr(device_lib(), f"probe_{op}{variant if op.startswith(FQ2_PREFIXES) else ''}"), op, lanes)


# ------------------------------------------------------------------------------------------------ comparisons
def _hx(t):
    return "(" + ", ".join(hex(v) for v in t) + ")"


def exact(op, lanes, got, want):
    assert len(got) == len(want) == len(lanes)
    for i, (g, w) in enumerate(zip(got, want)):
        if tuple(g) != tuple(w):
            raise AssertionError(f"{op}: lane {i} of {len(lanes)}: inputs {_hx(lanes[i])}\n  got  {_hx(g)}\n  want {_hx(w)}")


def group(op, F, read, lanes, got, want_points, width=None):
    """every output (its first `width` words) is a valid representation (invariants) of the expected group element"""
    for i, (g, P) in enumerate(zip(got, want_points)):
        Pg, why = read(F, g if width is None else g[:width])
        if why is None and Pg != P:
            why = f"wrong group element: got {Pg and _hx(F.flat(Pg[0]) + F.flat(Pg[1]))}, want {P and _hx(F.flat(P[0]) + F.flat(P[1]))}"
        if why is not None:
            raise AssertionError(f"{op}: lane {i} of {len(lanes)}: {why}\n  inputs {_hx(lanes[i][:16])}{' …' if len(lanes[i]) > 16 else ''}\n  output {_hx(g)}")


class Case:
    def __init__(self, ops, lanes, check):
        self.ops, self.lanes, self.check = ops, lanes, check          # check(outs: {op: [tuple of words per lane]})

    def run(self, runner, variant=""):
        self.check({op: runner(op, self.lanes, variant) for op in self.ops})


# ------------------------------------------------------------------------------------------------ field input lists
def _rng(seed):
    return np.random.default_rng(seed)


@functools.lru_cache(maxsize=None)
def unary(p, uniform=1024):
    return edge_field(p) + rand_field(_rng(101), uniform, p)


@functools.lru_cache(maxsize=None)
def pairs(p):
    """the whole cross product of the edge list with itself and 4096 uniform pairs; not a multiple of 64"""
    e = edge_field(p)
    u = rand_field(_rng(102), 8192, p)
    out = [(a, b) for a in e for b in e] + list(zip(u[:4096], u[4096:]))
    assert len(out) % 64
    return out


@functools.lru_cache(maxsize=None)
def quads(p):
    e = edge_field(p)
    n = len(e)
    out = []
    for s, t in ((1, 2), (7, 3), (n // 2, n - 1)):
        out += [(e[i], e[j], e[(i + s) % n], e[(j + t) % n]) for i in range(n) for j in range(n)]
    # the stated bound a·b + c·d < 2p² at its worst, then cancellations: a·b = c·d, a·b = −c·d, c = 0 (mul_sub_mul: neg(0))
    out += [(p - 1,) * 4, (p - 1, p - 1, p - 1, p - 2), (p - 1, p - 2, p - 2, p - 1), (p - 2,) * 4]
    for a in e:
        for b in (e[3], e[6], e[n // 3], a):
            out += [(a, b, b, a), (a, b, a, b), (a, b, (p - a) % p, b), (a, b, 0, b), (a, b, 0, 0), (0, b, a, 0)]
    u = rand_field(_rng(103), 4 * 4096, p)
    out += [tuple(u[4 * i:4 * i + 4]) for i in range(4096)]
    if len(out) % 64 == 0:
        out.append((1, 2, 3, 4))
    return out


@functools.lru_cache(maxsize=None)
def wide(p):
    """inputs of reduce_once, in [0, 2p): around p and 2p, p with one 32-bit limb one above / one below, and the field's own edges"""
    out = [p - 1, p, p + 1, 2 * p - 1, 2 * p - 2, 0, 1]
    for k in range(8):
        out += [p + (1 << (32 * k)), p - (1 << (32 * k))]
    out += edge_field(p) + [p + v for v in edge_field(p)] + [v + p * int(i & 1) for i, v in enumerate(rand_field(_rng(104), 1024, p))]
    assert all(0 <= v < 2 * p for v in out)
    return out


@functools.lru_cache(maxsize=None)
def any_words(p):
    """arbitrary 256-bit words for is_canonical and pack(canon(unpack))"""
    raw = _rng(105).integers(0, 256, size=(1024, 32), dtype=np.uint8)
    return wide(p) + [(1 << 256) - 1, (1 << 256) - 2, 2 * p, 2 * p + 1, 4 * p, 5 * p, 5 * p + 1, 1 << 255] + [int.from_bytes(r.tobytes(), "little") for r in raw]


def _field_case(pfx, op, f):
    name = f"{pfx}_{op}"
    one = lambda xs: [(x,) for x in xs]
    if op in ("add", "sub", "mul"):
        lanes = pairs(f.p)
    elif op == "mul2sum":
        lanes = quads(f.p)
    elif op == "reduce_once":
        lanes = one(wide(f.p))
    elif op == "is_canonical":
        lanes = one(any_words(f.p))
    elif op == "inv":
        lanes = one(unary(f.p, 512))
    else:
        lanes = one(unary(f.p))
    want = [(getattr(f, op)(*lane),) for lane in lanes]
    return Case([name], lanes, lambda outs: exact(name, lanes, outs[name], want))


# ------------------------------------------------------------------------------------------------ Fq2
@functools.lru_cache(maxsize=None)
def fq2_elements():
    e = edge_field(Q_MOD)
    n = len(e)
    u = rand_field(_rng(106), 2 * 2048, Q_MOD)
    out = [(v, v) for v in e] + [(e[i], e[n - 1 - i]) for i in range(n)] + [(0, v) for v in e] + [(v, 0) for v in e]
    return out + list(zip(u[:2048], u[2048:]))


def _fq2_pairs():
    E = fq2_elements()
    n = len(E)
    top = (Q_MOD - 1, Q_MOD - 1)
    out = [(top, top), (top, (Q_MOD - 1, Q_MOD - 2)), ((Q_MOD - 1, 0), top), ((0, Q_MOD - 1), (0, Q_MOD - 1))]
    out += [(E[k], E[(37 * k + 11) % n]) for k in range(n)] + [(E[k], E[n - 1 - k]) for k in range(n)] + [(E[k], E[k]) for k in range(4 * 83)]
    return out


def _fq2_quads():
    E = fq2_elements()
    n = len(E)
    top = (Q_MOD - 1, Q_MOD - 1)
    out = [(top,) * 4, (top, top, top, (Q_MOD - 1, Q_MOD - 2))]
    for s, t in ((1, 2), (7, 3), (n // 2, n - 1)):
        out += [(E[k], E[(5 * k + 1) % n], E[(k + s) % n], E[(5 * k + 1 + t) % n]) for k in range(n)]
    for k in range(0, n, 3):
        a, b = E[k], E[(11 * k + 5) % n]
        out += [(a, b, b, a), (a, b, a, b), (a, b, (0, 0), b), ((0, 0), b, a, (0, 0))]
    return out


def _fops_case(pfx, op):
    name = f"{pfx}_{op}"
    if pfx == "fqops":
        f, wrap = M.FQ, (lambda v: (v,))
        lanes = {"add": pairs, "sub": pairs, "mul": pairs, "mul_sub_mul": quads}.get(op, lambda p: [(x,) for x in unary(p, 512 if op == "inv" else 1024)])(Q_MOD)
        args = lanes
    else:
        f, wrap = M.FQ2, (lambda v: tuple(v))
        if op in ("add", "sub", "mul"):
            args = _fq2_pairs()
        elif op == "mul_sub_mul":
            args = _fq2_quads()
        elif op == "inv":
            e = edge_field(Q_MOD)
            args = [((0, 0),)] + [((v, 0),) for v in e] + [((0, v),) for v in e] + [(x,) for x in fq2_elements()[:4 * len(e)] + fq2_elements()[-256:]]
        else:
            args = [(x,) for x in fq2_elements()]
        lanes = [tuple(w for el in a for w in el) for a in args]
    want = [wrap(getattr(f, op)(*a)) for a in args]
    return Case([name], lanes, lambda outs: exact(name, lanes, outs[name], want))


# ------------------------------------------------------------------------------------------------ lazy fields
def _f29_case(op):
    name, p, R = f"f29_{op}", Q_MOD, M.R256
    one = lambda xs: [(x,) for x in xs]
    if op in ("mul", "sub31", "sqr_lazy", "zero_tests"):
        lanes = pairs(p)
    elif op in ("mul2", "mul4"):
        lanes = quads(p)
    elif op == "sub53":
        lanes = [q[:3] for q in quads(p)[::3]] + [(0, p - 1, p - 1), (p - 1, 0, 0), (0, 0, 0)]
    elif op == "inv":
        lanes = one(unary(p, 192))
    elif op == "inv_ds":
        lanes = one(unary(p, 2048))
    elif op == "inv_ds_lazy":
        lanes = pairs(p)[:83 * 83] + pairs(p)[-1024:]
    elif op == "pack_canon_unpack":
        lanes = one(any_words(p))
    else:
        lanes = one(unary(p))
    fn = {"from_std": lambda a: a * R, "from_mont256": lambda a: a, "pack_canon_unpack": lambda a: a, "mul": lambda a, b: a * b * R,
          "sqr": lambda a: a * a * R, "mul2": lambda a, b, c, d: (a * b + c * d) * R, "mul4": lambda a, b, c, d: (a * b + c * d + a * c + b * d) * R,
          "sub31": lambda a, b: (a - b) * R, "sub53": lambda a, b, c: (a - b - 2 * c) * R, "sqr_lazy": lambda a, b: (a - b) ** 2 * R,
          "inv": lambda a: M.inv0(a, p) * R, "inv_ds": lambda a: M.inv0(a, p) * R, "inv_ds_lazy": lambda a, b: M.inv0(a + b, p) * R,
          "zero_tests": lambda a, b: 3 | M.f29_maybe_zero_of_difference(a, b) << 2 | int(a == b) << 3}[op]
    want = [(fn(*lane) % p,) for lane in lanes]
    if op == "zero_tests":   # the cheap filter is a NECESSARY condition: it may never reject a true zero
        assert all(w[0] & 4 for lane, w in zip(lanes, want) if lane[0] == lane[1])
    return Case([name], lanes, lambda outs: exact(name, lanes, outs[name], want))


def _fr29_case(op):
    name, p = f"fr29_{op}", R_MOD
    one = lambda xs: [(x,) for x in xs]
    if op in ("mul", "sub2", "sub1300"):
        lanes = pairs(p)
    elif op == "mul_lazy":
        lanes = quads(p)
    elif op == "pack_canon_unpack":
        lanes = one(any_words(p))
    else:
        lanes = one(unary(p))
    fn = {"from_std": lambda a: (a,), "from_mont256": lambda a: (32 * a % p,), "pack_canon_unpack": lambda a: (a % p,), "mul": lambda a, b: (a * b % p,),
          "mul_lazy": lambda a, b, c, w: ((a + b - c) * w % p,), "sub2": lambda a, b: ((a - b) % p,), "sub1300": lambda a, b: ((a - b) % p,) * 2}[op]
    want = [fn(*lane) for lane in lanes]
    return Case([name], lanes, lambda outs: exact(name, lanes, outs[name], want))


# ------------------------------------------------------------------------------------------------ curves
BASE_SCALARS = list(range(1, 33)) + [int(v) % (R_MOD - 1) + 1 for v in rand_field(_rng(107), 32, R_MOD)]


@functools.lru_cache(maxsize=None)
def _points_of(O, grp, scalars):
    """k·G for every k, from the oracle, as affine points over Python integers (0 ↦ None)"""
    gen = O.ec_to_affine(grp, O.ec_generator(grp))
    std = O.fixed_base_mul(grp, gen, ints_to_words([k if k else 1 for k in scalars]))
    w = words_to_ints(std.reshape(-1, 4))
    F = M.FIELD[grp]
    per = 2 * F.words
    pts = [(F.unflat(w[i * per:i * per + F.words]), F.unflat(w[i * per + F.words:(i + 1) * per])) for i in range(len(scalars))]
    return [P if k else None for P, k in zip(pts, scalars)]


def base_points(O, grp):
    return _points_of(O, grp, tuple(BASE_SCALARS))


def _lams(F, n, seed):
    """n non-trivial scaling factors (neither 0 nor 1)"""
    u = rand_field(_rng(seed), 2 * n, Q_MOD - 2)
    return [F.unflat([u[2 * i] + 2, u[2 * i + 1]]) if F.words == 2 else u[2 * i] + 2 for i in range(n)]


@functools.lru_cache(maxsize=None)
def point_pairs(O, grp):
    """(P, Q): generic, Q = P, Q = −P, P the identity, Q the identity, both"""
    F, B = M.FIELD[grp], base_points(O, grp)
    out = [(B[i], B[(i + 1) % 64]) for i in range(64)] + [(B[i], B[(5 * i + 9) % 64]) for i in range(0, 64, 3)]
    out += [(B[i], B[i]) for i in range(0, 64, 3)] + [(B[i], M.ec_neg(F, B[i])) for i in range(1, 64, 3)]
    out += [(None, B[i]) for i in range(0, 64, 8)] + [(B[i], None) for i in range(3, 64, 8)] + [(None, None)] * 2
    assert len(out) % 64
    return out


def _curve_case(O, grp, op, key=None):
    """`key`: the probe whose outputs are checked, when it is not ec.h's own (the lazy twin of ec29.h on the same list)"""
    F, B = M.FIELD[grp], base_points(O, grp)
    name = key or f"{grp}_{op}"
    b3 = M.to_mont(F, F.mul(F.small(3), F.b))
    PQ = point_pairs(O, grp)
    l1, l2 = _lams(F, len(PQ), 108), _lams(F, len(PQ), 109)
    singles = B + [None]
    ls = _lams(F, len(singles), 110)
    rd = M.read_xyzz
    if op == "x_madd":
        lanes = [M.xyzz_of(F, P, a) + M.affine_of(F, Q) for (P, Q), a in zip(PQ, l1)] + [M.xyzz_of(F, P) + M.affine_of(F, Q) for P, Q in PQ]
        want = [M.ec_add(F, P, Q) for P, Q in PQ] * 2
    elif op == "x_add":
        lanes = [M.xyzz_of(F, P, a) + M.xyzz_of(F, Q, b) for (P, Q), a, b in zip(PQ, l1, l2)]
        want = [M.ec_add(F, P, Q) for P, Q in PQ]
    elif op == "x_dbl":
        lanes = [M.xyzz_of(F, P, a) for P, a in zip(singles, ls)] + [M.xyzz_of(F, P) for P in singles]
        want = [M.ec_add(F, P, P) for P in singles] * 2
    elif op in ("x_dbl_affine", "x_dbl_affine_exact"):
        pts = B + [M.ec_neg(F, P) for P in B[:7]]
        lanes = [M.affine_of(F, P) for P in pts]
        want = [M.ec_add(F, P, P) for P in pts]
    elif op == "x_proj_roundtrip":
        lanes = [M.proj_of(F, P, a) for P, a in zip(singles, ls)] + [M.proj_of(F, P) for P in singles]
        want, rd = singles * 2, M.read_proj
    elif op == "p_add":
        lanes = [M.proj_of(F, P, a) + M.proj_of(F, Q, b) + b3 for (P, Q), a, b in zip(PQ, l1, l2)]
        want, rd = [M.ec_add(F, P, Q) for P, Q in PQ], M.read_proj
    elif op == "p_dbl":
        lanes = [M.proj_of(F, P, a) + b3 for P, a in zip(singles, ls)]
        want, rd = [M.ec_add(F, P, P) for P in singles], M.read_proj
    elif op == "p_to_affine":
        lanes = [M.proj_of(F, P, a) for P, a in zip(singles, ls)] + [M.proj_of(F, P) for P in singles]
        want_words = [M.affine_of(F, P) for P in singles] * 2
        return Case([name], lanes, lambda outs: exact(name, lanes, outs[name], want_words))
    elif op == "p_eq":
        lanes = [M.proj_of(F, P, a) + M.proj_of(F, Q, b) for (P, Q), a, b in zip(PQ, l1, l2)]
        want_words = [(int(P == Q),) for P, Q in PQ]
        return Case([name], lanes, lambda outs: exact(name, lanes, outs[name], want_words))
    else:
        raise KeyError(op)

    def check(outs):
        group(name, F, rd, lanes, outs[name], want)
        if op == "x_proj_roundtrip":   # (X : Y : Z) ↦ (X·Z⁴ : Y·Z⁴ : Z⁵), the identity ↦ (0 : 1 : 0): the same formulas, bit for bit
            ex = []
            for P, a in list(zip(singles, ls)) + [(P, F.one) for P in singles]:
                z4 = F.mul(F.mul(a, a), F.mul(a, a))
                ex.append(M.proj_of(F, None) if P is None else M.to_mont(F, F.mul(F.mul(P[0], a), z4)) + M.to_mont(F, F.mul(F.mul(P[1], a), z4)) + M.to_mont(F, F.mul(z4, a)))
            exact(name, lanes, outs[name], ex)
    return Case([name], lanes, check)


def _curvel_case(O, grp, op):
    F, B = M.FIELD[grp], base_points(O, grp)
    name = f"{grp}l_{op}"
    if op.startswith("load_affine"):
        form = op.split("_")[2]
        enc = {"std": 1, "mont256": M.R256, "internal": M.R261}[form]
        pts = B + [M.ec_neg(F, P) for P in B[:7]]
        lanes = [tuple(v * enc % Q_MOD for v in F.flat(P[0]) + F.flat(P[1])) for P in pts]
        want = [M.affine_of(F, M.ec_neg(F, P) if op.endswith("_neg") else P) for P in pts]
        return Case([name], lanes, lambda outs: exact(name, lanes, outs[name], want))
    if op in ("x_from_old", "x_internal_roundtrip"):
        singles = B + [None]
        lanes = [M.xyzz_of(F, P, a) for P, a in zip(singles, _lams(F, len(singles), 111))] + [M.xyzz_of(F, P) for P in singles]
        if op == "x_from_old":
            want = lanes
        else:       # the internal encoding is the canonical Montgomery-261 word: 2^5 times the Montgomery-256 one
            want = [lane + tuple(v * 32 % Q_MOD for v in lane) for lane in lanes]
        return Case([name], lanes, lambda outs: exact(name, lanes, outs[name], want))
    if op == "chain":
        return _chain_case(O, grp)
    # the same lists as ec.h's operation of that name, the same group elements, and — same formulas — the same coordinates
    old_op = "x_dbl_affine" if op == "x_dbl_affine_exact" else op
    old_name = f"{grp}_{old_op}"
    old, lazy = _curve_case(O, grp, old_op), _curve_case(O, grp, old_op, key=name)
    lanes = old.lanes

    def check(outs):
        lazy.check(outs)                                              # group element and invariants of the lazy result
        old.check(outs)
        exact(f"{name} against {old_name}", lanes, outs[name], outs[old_name])
    return Case([name, old_name], lanes, check)


@functools.lru_cache(maxsize=None)
def _chain_case(O, grp):
    """128 buckets of 200 signed additions.  Lanes 0–63 walk over k·G with |k| ≤ 8 so that the accumulator keeps meeting the base it
    is given (P + P, P − P, restart after the identity); lanes 64–127 start with those patterns and go on with large multiples."""
    F, B, W = M.FIELD[grp], base_points(O, grp), M.FIELD[grp].words
    rng = _rng(112 if grp == "g1" else 113)
    lanes, totals, hits = [], [], {"dbl": 0, "cancel": 0, "restart": 0}
    for lane in range(CHAIN_LANES):
        if lane < 64:
            idx = rng.integers(0, 8, size=CHAIN)
        else:
            idx = rng.integers(0, 64, size=CHAIN)
            idx[:6] = [[4, 4, 9, 17, 2, 2], [4, 4, 6, 6, 11, 11], [0, 1, 2, 5, 11, 40], [3, 3, 3, 10, 5, 50]][lane % 4]
        sg = rng.integers(0, 2, size=CHAIN)
        if lane >= 64:
            sg[:6] = [[0, 0, 1, 0, 1, 1], [1, 0, 0, 1, 1, 1], [0, 0, 0, 0, 1, 0], [1, 1, 1, 0, 1, 0]][lane % 4]
        words, k = [], 0
        for i, s in zip(idx, sg):
            step = -BASE_SCALARS[i] if s else BASE_SCALARS[i]
            hits["restart"] += k == 0 and len(words) > 0
            hits["dbl"] += k == step
            hits["cancel"] += k == -step
            k += step                                                  # (as an integer: no sum of these multiples reaches r by accident)
            words += M.affine_of(F, B[i]) + (int(s),)
        lanes.append(tuple(words))
        totals.append(k % R_MOD)
    assert min(hits.values()) >= 16, hits
    want = _points_of(O, grp, tuple(totals))
    name = f"{grp}l_chain"

    def check(outs):
        got = outs[name]
        group(f"{name} (ec.h accumulator)", F, M.read_xyzz, lanes, got, want, width=4 * W)
        group(f"{name} (ec29.h accumulator)", F, M.read_xyzz, lanes, [g[4 * W:] for g in got], want)
        exact(f"{name}: ec29.h against ec.h", lanes, [g[4 * W:] for g in got], [g[:4 * W] for g in got])
    return Case([name], lanes, check)


# ------------------------------------------------------------------------------------------------ the list of cases
FIELD_OPS = ("add", "sub", "neg", "dbl", "mul3", "mul", "sqr", "mul2sum", "to_mont", "from_mont", "inv", "reduce_once", "is_canonical")
FOPS = ("add", "sub", "neg", "dbl", "mul", "sqr", "inv", "mul_sub_mul")
F29_OPS = ("from_std", "from_mont256", "pack_canon_unpack", "mul", "sqr", "mul2", "mul4", "sub31", "sub53", "sqr_lazy", "inv", "inv_ds", "inv_ds_lazy", "zero_tests")
FR29_OPS = ("from_std", "from_mont256", "pack_canon_unpack", "mul", "mul_lazy", "sub2", "sub1300")
CURVE_OPS = ("x_madd", "x_add", "x_dbl", "x_dbl_affine", "x_proj_roundtrip", "p_add", "p_dbl", "p_to_affine", "p_eq")
CURVEL_OPS = tuple(f"load_affine_{f}{n}" for f in ("std", "mont256", "internal") for n in ("", "_neg")) + \
    ("x_madd", "x_add", "x_dbl", "x_dbl_affine_exact", "x_from_old", "x_internal_roundtrip", "chain")

# id → (builder taking the oracle, device variant)
CASES = {}
for _op in FIELD_OPS:
    CASES[f"Fr-{_op}"] = (functools.partial(lambda O, op: _field_case("fr", op, M.FR), op=_op), "")
    CASES[f"Fq-{_op}"] = (functools.partial(lambda O, op: _field_case("fq", op, M.FQ), op=_op), "")
for _op in FOPS:
    CASES[f"FqOps-{_op}"] = (functools.partial(lambda O, op: _fops_case("fqops", op), op=_op), "")
    CASES[f"Fq2-{_op}"] = (functools.partial(lambda O, op: _fops_case("fq2", op), op=_op), "")
    CASES[f"Fq2-inline-{_op}"] = (functools.partial(lambda O, op: _fops_case("fq2", op), op=_op), "_inline")
for _op in F29_OPS:
    CASES[f"f29-{_op}"] = (functools.partial(lambda O, op: _f29_case(op), op=_op), "")
for _op in FR29_OPS:
    CASES[f"fr29-{_op}"] = (functools.partial(lambda O, op: _fr29_case(op), op=_op), "")
for _op in CURVE_OPS:
    CASES[f"G1-{_op}"] = (functools.partial(lambda O, op: _curve_case(O, "g1", op), op=_op), "")
    CASES[f"G2-{_op}"] = (functools.partial(lambda O, op: _curve_case(O, "g2", op), op=_op), "")
    CASES[f"G2-inline-{_op}"] = (functools.partial(lambda O, op: _curve_case(O, "g2", op), op=_op), "_inline")
for _op in CURVEL_OPS:
    CASES[f"G1L-{_op}"] = (functools.partial(lambda O, op: _curvel_case(O, "g1", op), op=_op), "")
    CASES[f"G2L-{_op}"] = (functools.partial(lambda O, op: _curvel_case(O, "g2", op), op=_op), "")
HOST_CASES = [k for k, (_, variant) in CASES.items() if not variant]    # the host has one instantiation of Fq2Ops
