"""groth16_zkey_verify_ptau in the exponent: the synthesiser knows every discrete logarithm, so each equation of
include/groth16_prover.h becomes one over Fr in Python integers — a section of points is the list of its scalars, a pairing
e(S, Q) = e(T, G₂) is s·q = t.  A test mutates the scalar lists exactly as it mutates the file and asks evaluate() for the kind, the
index and the mask the library must report for the same seed.  Nothing here calls the library.

  key     dict(a, b1, b2, c, ic, h): the scalars of sections 5, 6, 7, 8, 3, 9   (key_from(S.key_scalars(...)))
  header  dict(alpha1, beta1, beta2, gamma2, delta2): the scalars of the header's points
  ptau    (tau, alpha, beta)
"""
import hashlib

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
SIZES, KEY, HEADER, A, B1, B2, IC, C, H = range(1, 10)
NAMES = ["ok", "SIZES", "KEY", "HEADER", "A", "B1", "B2", "IC", "C", "H"]


def bit(kind):
    return 1 << (kind - HEADER)


def coefficient(seed: bytes, i: int) -> int:
    """the combined verifier's z_i: the low 128 bits of SHA-256(seed ‖ LE64(i)) as a little-endian integer, 0 replaced by 1"""
    return int.from_bytes(hashlib.sha256(seed + i.to_bytes(8, "little")).digest()[:16], "little") or 1


def key_from(ks):
    return dict(a=list(ks["a"]), b1=list(ks["b"]), b2=list(ks["b"]), c=list(ks["c"]), ic=list(ks["ic"]), h=list(ks["h"]))


def header_from(toxic):
    tau, alpha, beta, gamma, delta = toxic
    return dict(alpha1=alpha, beta1=beta, beta2=beta, gamma2=gamma, delta2=delta)


def rows(r, v, n):
    """a(v), b(v), c(v) over the domain: the circuit's rows, the public-binding rows in a, zeros above"""
    a, b, c = [0] * n, [0] * n, [0] * n
    for out, mat in ((a, r.A), (b, r.B), (c, r.C)):
        for (j, i, coef) in mat:
            out[j] = (out[j] + coef * v[i]) % R
    for s in range(r.n_public + 1):
        a[r.n_constraints + s] = v[s] % R
    return a, b, c


def dot(xs, ys):
    assert len(xs) == len(ys)
    return sum(x * y for x, y in zip(xs, ys)) % R


def evaluate(S, r, key, header, ptau, seed: bytes):
    """(kind, index, failed_mask) of a key whose sizes match the circuit's and whose points the key check accepts"""
    tau, alpha, beta = ptau
    m, npub = r.n_vars, r.n_public
    n = 1
    while n < r.n_constraints + npub + 1:
        n <<= 1
    logn = n.bit_length() - 1
    z = [coefficient(seed, s) for s in range(m)]
    y = [coefficient(seed, m + i) for i in range(n)]
    zpub = [z[s] if s <= npub else 0 for s in range(m)]
    zpriv = [0 if s <= npub else z[s] for s in range(m)]
    L = S.lagrange_at(n, logn, tau) if n > 1 else [1]
    L2 = S.lagrange_at(2 * n, logn + 1, tau)
    faults = []
    for index, (mine, theirs) in enumerate(((header["alpha1"], alpha), (header["beta1"], beta), (header["beta2"], beta))):
        if mine % R != theirs % R:
            faults.append((HEADER, index))
    a, b, _ = rows(r, z, n)
    if dot(z, key["a"]) != dot(a, L):
        faults.append((A, 0))
    if dot(z, key["b1"]) != dot(b, L):
        faults.append((B1, 0))
    if dot(z, key["b2"]) != dot(b, L):
        faults.append((B2, 0))

    def t_of(v):
        av, bv, cv = rows(r, v, n)
        return (beta * dot(av, L) + alpha * dot(bv, L) + dot(cv, L)) % R
    if header["gamma2"] * dot(z[:npub + 1], key["ic"]) % R != t_of(zpub):
        faults.append((IC, 0))
    if header["delta2"] * dot(z[npub + 1:], key["c"]) % R != t_of(zpriv):
        faults.append((C, 0))
    if header["delta2"] * dot(y, key["h"]) % R != dot(y, L2[1::2]):
        faults.append((H, 0))
    mask = 0
    for kind, _ in faults:
        mask |= bit(kind)
    return (faults[0][0], faults[0][1], mask) if faults else (0, 0, 0)
