"""Shared by tests/test_dist_qap.py (CPU) and tests/test_gpu_dist.py / tests/test_gpu_dist_shapes.py (GPU): the host-side
emulation of the two all-to-alls, the integer model of one whole distributed round, and the hand-made R1CS whose rows have
every shape the spmv's row loop can meet.  Test infrastructure, no test of its own."""
from __future__ import annotations

import random

import dist_qap_model as D

R_MOD = D.R_MOD


def exchange(K, bufs, rows, rb, cb):
    """bufs[r] = (send ptr, recv ptr) of rank r: chunk (q, p) of r's send buffer → offset (q, r) of p's receive buffer"""
    G = len(bufs)
    sends = [K.raw_to_host(s, rows * rb) for s, _ in bufs]
    for p in range(G):
        recv = bytearray(rows * rb)
        for q in range(rows):
            for r in range(G):
                recv[q * rb + r * cb:q * rb + (r + 1) * cb] = sends[r][q * rb + p * cb:q * rb + (p + 1) * cb]
        K.raw_to_device(bufs[p][1], bytes(recv))


def model_round(O, rows, logn, G):
    """One distributed round in plain integers from the spmv's rows [B | A | A∘B] (three lists of n = 2^logn):
    → (Y, Z, E) with Y[r][row] = what rank r sends in exchange 1 (m elements), Z[b][row][i1] = the chunk rank b sends to
    rank i1 in exchange 2 (m/G elements) and E[r] = A·B − C' at the coset points i ≡ r (mod G)."""
    n = 1 << logn
    m, mb = n // G, n // (G * G)
    wn, w2n = O.fr_omega(logn), O.fr_omega(logn + 1)
    inv = lambda v: O.arr_to_ints(O.fr_ntt(O.ints_to_arr(v), True))       # size-m inverse DFT including 1/m
    fwd = lambda v: O.arr_to_ints(O.fr_ntt(O.ints_to_arr(v), False))
    pw2n = D.power_table(w2n, 2 * n)
    Y = [D.stage1([x[r::G] for x in rows], r, G, n, wn, inv) for r in range(G)]
    Z = [D.stage2_tab([[Y[j1][row][b * mb:(b + 1) * mb] for j1 in range(G)] for row in range(3)], b, G, n, pw2n) for b in range(G)]
    E = [D.stage3([sum((Z[b][row][r] for b in range(G)), []) for row in range(3)], fwd) for r in range(G)]
    return Y, Z, E


# ---- the row-shape circuit ---------------------------------------------------------------------------------------------
LONG = (1, 2, 63, 64, 65, 300)                      # entries of the long side: around the 64 lanes of a wave, and far beyond
SPECIAL_COEFFS = (1, R_MOD - 1, R_MOD - 2, (1 << 253) + 1)
# one shape per run of eight consecutive rows, so that every residue class mod 8 (the widest distributed shard count) holds
# every shape: ("A", L) = A of L entries against B of one, ("B", L) the mirror image, the three kinds of empty rows and the
# records given twice and three times
SHAPES = [("A", L) for L in reversed(LONG)] + [("B", L) for L in LONG[:-1]] + [("A0", 0), ("B0", 0), ("00", 0), ("dup2", 0), ("dup3", 0), ("B", LONG[-1])]
BLOCK = 8 * len(SHAPES)


def row_shape_circuit(S, n_constraints=6000, n_public=2, n_inputs=400, seed=11):
    """(R1CS, witness, block starts) of domain 2^13.  Wires: 0 = the constant, 1 … n_public public, then the wire each
    constraint defines through C as the product of its A and B rows (the way synth.random_circuit does, so the witness
    satisfies the system), then n_inputs free wires — the last of them is wire n_vars − 1.  Three blocks of BLOCK rows (at
    row 0, in the middle, and ending on the last constraint row) run through SHAPES; row 0 is ("A", 300) and the last
    constraint row ("B", 300).  The rows between the blocks have 1 – 3 entries in A and 1 – 2 in B.  Entry e of row j
    carries coefficient r − 1, r − 2, 2^253 + 1, 1 or a 16-bit value by (j + e) mod 5; the long rows name wire 0 first and
    wire n_vars − 1 last."""
    nc = n_constraints
    assert nc % 8 == 0 and nc >= 3 * BLOCK
    rng = random.Random(seed)
    first_out = 1 + n_public
    first_in = first_out + nc
    n_vars = first_in + n_inputs
    r = S.R1CS(n_vars=n_vars, n_public=n_public, n_constraints=nc)
    w = [0] * n_vars
    w[0] = 1
    for i in list(range(1, first_out)) + list(range(first_in, n_vars)):
        w[i] = rng.randrange(2) if rng.random() < 0.3 else rng.randrange(1, R_MOD)
    starts = (0, (nc // 2) // 8 * 8, nc - BLOCK)
    shape_of = {}
    for s in starts:
        for t, shape in enumerate(SHAPES):
            for c in range(8):
                shape_of[s + 8 * t + c] = shape

    def coeff(j, e):
        k = (j + e) % 5
        return SPECIAL_COEFFS[k] if k < 4 else rng.randrange(2, 1 << 16)

    def wires(j, count):
        """`count` distinct wires whose values exist when row j is reached; wire 0 first and wire n_vars − 1 last in a long row"""
        known = first_out + j                               # wires 0 … known − 1, and all the inputs
        pick = lambda i: i if i < known else first_in + (i - known)
        if count >= 63:
            mid = rng.sample(range(1, known + n_inputs - 1), count - 2)
            return [0] + [pick(i) for i in mid] + [n_vars - 1]
        return [pick(i) for i in rng.sample(range(known + n_inputs), count)]

    for j in range(nc):
        kind, L = shape_of.get(j, ("fill", 0))
        if kind == "A":
            la, lb = wires(j, L), wires(j, 1)
        elif kind == "B":
            la, lb = wires(j, 1), wires(j, L)
        elif kind == "A0":
            la, lb = [], wires(j, 2)
        elif kind == "B0":
            la, lb = wires(j, 2), []
        elif kind == "00":
            la, lb = [], []
        elif kind == "dup2":                                # one (A, j, wire) record twice, between two others
            x, y, z = wires(j, 3)
            la, lb = [x, y, x, z], wires(j, 1)
        elif kind == "dup3":                                # one (B, j, wire) record three times
            x, y = wires(j, 2)
            la, lb = wires(j, 1), [x, x, y, x]
        else:
            la, lb = wires(j, rng.randrange(1, 4)), wires(j, rng.randrange(1, 3))
        sa = sb = 0
        for e, x in enumerate(la):
            v = coeff(j, e)
            r.A.append((j, x, v))
            sa += v * w[x]
        for e, x in enumerate(lb):
            v = coeff(j, len(la) + e)
            r.B.append((j, x, v))
            sb += v * w[x]
        r.C.append((j, first_out + j, 1))
        w[first_out + j] = (sa % R_MOD) * (sb % R_MOD) % R_MOD
    return r, w, starts
