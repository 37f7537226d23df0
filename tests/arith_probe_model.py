"""Expected values for tests/arith_probe.hip in Python integers: the Montgomery fields of ff.h (R = 2^256), Fq2, the lazy
radix-2^29 fields (R' = 2^261) and the affine group law over Fq and Fq2, written once for both."""
from field_inputs import Q_MOD, R_MOD

R256 = 1 << 256
R261 = 1 << 261


def inv0(x, p):
    """x⁻¹ mod p with the project's convention 0⁻¹ = 0"""
    return pow(x, -1, p) if x % p else 0


class Mont:
    """ff.h's Fp<P> on residues: every operation takes and returns integers in [0, p) (unless stated otherwise)"""

    def __init__(self, p):
        self.p, self.rinv, self.r2 = p, pow(R256, -1, p), R256 * R256 % p

    def add(self, a, b): return (a + b) % self.p
    def sub(self, a, b): return (a - b) % self.p
    def neg(self, a): return -a % self.p
    def dbl(self, a): return 2 * a % self.p
    def mul3(self, a): return 3 * a % self.p
    def mul(self, a, b): return a * b * self.rinv % self.p
    def sqr(self, a): return a * a * self.rinv % self.p
    def mul2sum(self, a, b, c, d): return (a * b + c * d) * self.rinv % self.p
    def mul_sub_mul(self, a, b, c, d): return (a * b - c * d) * self.rinv % self.p
    def to_mont(self, a): return a * R256 % self.p
    def from_mont(self, a): return a * self.rinv % self.p
    def inv(self, a): return inv0(a, self.p) * self.r2 % self.p                   # x·R ↦ x⁻¹·R
    def reduce_once(self, a): return a - self.p if a >= self.p else a             # a in [0, 2p)
    def is_canonical(self, a): return int(a < self.p)                             # a any 256-bit word


FR, FQ = Mont(R_MOD), Mont(Q_MOD)


class Mont2:
    """Fq2Ops of ec.h on pairs (c0, c1), u² = −1, Montgomery components"""
    p, f = Q_MOD, FQ

    def add(self, a, b): return (self.f.add(a[0], b[0]), self.f.add(a[1], b[1]))
    def sub(self, a, b): return (self.f.sub(a[0], b[0]), self.f.sub(a[1], b[1]))
    def neg(self, a): return (self.f.neg(a[0]), self.f.neg(a[1]))
    def dbl(self, a): return (self.f.dbl(a[0]), self.f.dbl(a[1]))
    def mul(self, a, b): return ((a[0] * b[0] - a[1] * b[1]) * self.f.rinv % self.p, (a[0] * b[1] + a[1] * b[0]) * self.f.rinv % self.p)
    def sqr(self, a): return self.mul(a, a)
    def mul_sub_mul(self, a, b, c, d): return self.sub(self.mul(a, b), self.mul(c, d))

    def inv(self, a):
        x0, x1 = self.f.from_mont(a[0]), self.f.from_mont(a[1])
        d = inv0(x0 * x0 + x1 * x1, self.p)
        return (self.f.to_mont(x0 * d % self.p), self.f.to_mont(-x1 * d % self.p))


FQ2 = Mont2()


# ------------------------------------------------------------------------------------------------ lazy radix-2^29 fields
NINV261 = -pow(Q_MOD, -1, R261) % R261
PINV29 = pow(Q_MOD, -1, 1 << 29)


def redc261(t):
    """the exact representative ff29.h's product scanning returns for a column sum t: (t + m·p) / 2^261, m = −t·p⁻¹ mod 2^261"""
    return (t + (t * NINV261 % R261) * Q_MOD) >> 261


def f29_from_std(a):
    """from_std's lazy result (an integer below 2p, congruent to a·2^261)"""
    return redc261(a * (R261 * R261 % Q_MOD))


def f29_maybe_zero_of_difference(a, b):
    """maybe_zero_mod_p(norm(sub<3,1>(from_std(a), from_std(b)))): the low 29-bit limb of the exact lazy value decides"""
    v = f29_from_std(a) + 3 * Q_MOD - f29_from_std(b)
    return int(((v & ((1 << 29) - 1)) * PINV29) & ((1 << 29) - 1) < 16)


# ------------------------------------------------------------------------------------------------ curves, affine, integers
class Base:
    """Fq for the group law: plain residues"""
    p = Q_MOD
    zero, one, words = 0, 1, 1
    b = 3
    def add(self, a, b): return (a + b) % self.p
    def sub(self, a, b): return (a - b) % self.p
    def mul(self, a, b): return a * b % self.p
    def inv(self, a): return pow(a, -1, self.p)
    def neg(self, a): return -a % self.p
    def small(self, k): return k % self.p
    def flat(self, a): return (a,)
    def unflat(self, w): return w[0]


class Ext(Base):
    """Fq2 for the group law: pairs of plain residues; the twist's b = 3 / (9 + u)"""
    zero, one, words = (0, 0), (1, 0), 2
    def add(self, a, b): return ((a[0] + b[0]) % self.p, (a[1] + b[1]) % self.p)
    def sub(self, a, b): return ((a[0] - b[0]) % self.p, (a[1] - b[1]) % self.p)
    def mul(self, a, b): return ((a[0] * b[0] - a[1] * b[1]) % self.p, (a[0] * b[1] + a[1] * b[0]) % self.p)
    def neg(self, a): return (-a[0] % self.p, -a[1] % self.p)
    def small(self, k): return (k % self.p, 0)
    def flat(self, a): return tuple(a)
    def unflat(self, w): return (w[0], w[1])

    def inv(self, a):
        d = pow(a[0] * a[0] + a[1] * a[1], -1, self.p)
        return (a[0] * d % self.p, -a[1] * d % self.p)


Ext.b = Ext().mul((3, 0), Ext().inv((9, 1)))
F1, F2 = Base(), Ext()
FIELD = {"g1": F1, "g2": F2}


def on_curve(F, P):
    """P = None is the identity"""
    if P is None:
        return True
    x, y = P
    return F.mul(y, y) == F.add(F.mul(F.mul(x, x), x), F.b)


def ec_neg(F, P):
    return None if P is None else (P[0], F.neg(P[1]))


def ec_add(F, P, Q):
    """the affine group law, every case"""
    if P is None:
        return Q
    if Q is None:
        return P
    if P[0] == Q[0]:
        if P[1] != Q[1] or P[1] == F.zero:
            return None
        lam = F.mul(F.mul(F.small(3), F.mul(P[0], P[0])), F.inv(F.add(P[1], P[1])))
    else:
        lam = F.mul(F.sub(Q[1], P[1]), F.inv(F.sub(Q[0], P[0])))
    x = F.sub(F.sub(F.mul(lam, lam), P[0]), Q[0])
    return (x, F.sub(F.mul(lam, F.sub(P[0], x)), P[1]))


def to_mont(F, a):
    return tuple(v * R256 % Q_MOD for v in F.flat(a))


def from_mont_words(F, w):
    return F.unflat([v * FQ.rinv % Q_MOD for v in w])


def xyzz_of(F, P, lam=None):
    """words of the XYZZ tuple (xλ², yλ³, λ², λ³), Montgomery form; identity: all zero"""
    if P is None:
        return (0,) * (4 * F.words)
    lam = F.one if lam is None else lam
    l2 = F.mul(lam, lam)
    l3 = F.mul(l2, lam)
    return to_mont(F, F.mul(P[0], l2)) + to_mont(F, F.mul(P[1], l3)) + to_mont(F, l2) + to_mont(F, l3)


def proj_of(F, P, lam=None):
    """words of the projective triple (xλ, yλ, λ), Montgomery form; identity (0, λ, 0)"""
    lam = F.one if lam is None else lam
    if P is None:
        return to_mont(F, F.zero) + to_mont(F, lam) + to_mont(F, F.zero)
    return to_mont(F, F.mul(P[0], lam)) + to_mont(F, F.mul(P[1], lam)) + to_mont(F, lam)


def affine_of(F, P):
    """words of an affine point, Montgomery form; identity (0, 0)"""
    if P is None:
        return (0,) * (2 * F.words)
    return to_mont(F, P[0]) + to_mont(F, P[1])


def read_xyzz(F, w):
    """raw XYZZ words (Montgomery) → (point or None, why-not-valid or None): checks ZZ³ = ZZZ² and the curve equation"""
    W = F.words
    x, y, zz, zzz = (from_mont_words(F, w[i * W:(i + 1) * W]) for i in range(4))
    if any(v >= Q_MOD for v in w):
        return None, "a coordinate is not canonical"
    if zz == F.zero:
        return None, None
    if F.mul(F.mul(zz, zz), zz) != F.mul(zzz, zzz):
        return None, "ZZ^3 != ZZZ^2"
    P = (F.mul(x, F.inv(zz)), F.mul(y, F.inv(zzz)))
    return P, None if on_curve(F, P) else "not on the curve"


def read_proj(F, w):
    W = F.words
    X, Y, Z = (from_mont_words(F, w[i * W:(i + 1) * W]) for i in range(3))
    if any(v >= Q_MOD for v in w):
        return None, "a coordinate is not canonical"
    if Z == F.zero:
        return None, None if X == F.zero and Y != F.zero else "Z = 0 but not (0 : y : 0)"
    zi = F.inv(Z)
    P = (F.mul(X, zi), F.mul(Y, zi))
    return P, None if on_curve(F, P) else "not on the curve"


def read_affine(F, w):
    W = F.words
    x, y = from_mont_words(F, w[:W]), from_mont_words(F, w[W:2 * W])
    if any(v >= Q_MOD for v in w):
        return None, "a coordinate is not canonical"
    if x == F.zero and y == F.zero:
        return None, None
    return (x, y), None if on_curve(F, (x, y)) else "not on the curve"
