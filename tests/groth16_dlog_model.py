"""Groth16 verification with chosen discrete logarithms — keys and proofs whose points are k·G for scalars picked here, and the
verdict every verifier must give them, from integer arithmetic mod r alone.  Test infrastructure (tests/test_pairing29.py,
tests/test_gpu_verify_batch.py).

With A = a·G₁, B = b·G₂, C = c·G₁, α₁ = α·G₁, β₂ = β·G₂, γ₂ = γ·G₂, δ₂ = δ·G₂ and ICⱼ = icⱼ·G₁, the verification equation
e(A, B) = e(α₁, β₂)·e(cpub, γ₂)·e(C, δ₂) holds exactly when

    a·b ≡ α·β + γ·(ic₀ + Σⱼ sⱼ·icⱼ₊₁) + δ·c   (mod r)

because e(G₁, G₂) has order r.  The identity has dlog 0, so every edge case of the verifier (identity points, cpub = O, the
doubling and cancelling branches of the public-input sum) is a choice of scalars with an exact answer.  Points come from the
CPU oracle's fixed-base multiplication (oracle/, its own C code), never from the library under test.
"""
from __future__ import annotations

import json
import random
from dataclasses import dataclass, field

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583

# public signals where scalar code goes wrong: the ends of the field, its halves, the top bit of a 254-bit scalar
EDGE_SIGNALS = [0, 1, R - 1, (R - 1) // 2, (R + 1) // 2, (1 << 253) - 1, 1 << 253]


@dataclass
class Key:
    alpha: int
    beta: int
    gamma: int
    delta: int
    ic: list                   # dlogs of IC₀ … IC_k; k ≥ n_public (entries past n_public + 1 are ignored by every verifier)
    n_public: int
    name: str = ""


@dataclass
class Proof:
    a: int
    b: int
    c: int
    b_outside: bool = False    # pi_b is a twist point outside the order-r subgroup (b is then not used)


@dataclass
class Item:
    key: Key
    proof: Proof
    signals: list              # public.json as integers (may be longer than n_public, may hold values ≥ r)
    label: str
    want: int = field(init=False)

    def __post_init__(self):
        self.want = model_verdict(self.key, self.proof, self.signals)

    @property
    def json_only(self):       # a case the parser decides (the checked header never sees it)
        return self.want == -2 and not self.proof.b_outside


def cpub_dlog(key: Key, signals) -> int:
    return (key.ic[0] + sum(s * key.ic[j + 1] for j, s in enumerate(signals[:key.n_public]))) % R


def model_verdict(key: Key, proof: Proof, signals) -> int:
    """1 accepted, 0 rejected, −2 for what the host verifier refuses as a format error: a signal ≥ r among the first
    n_public, too few signals, or a pi_b outside the order-r subgroup"""
    if len(signals) < key.n_public or any(not 0 <= s < R for s in signals[:key.n_public]) or proof.b_outside:
        return -2
    lhs = proof.a * proof.b
    rhs = key.alpha * key.beta + key.gamma * cpub_dlog(key, signals) + key.delta * proof.c
    return int((lhs - rhs) % R == 0)


def prove(key: Key, signals, a: int, b: int, e: int = 0, c: int | None = None) -> Proof:
    """c = (a·b − α·β − γ·cpub)/δ + e: valid for e = 0.  With δ = 0 the C term vanishes, so c stays as given (default 1) and
    a (b when b = 0) is solved for instead, e added to it."""
    t = (key.alpha * key.beta + key.gamma * cpub_dlog(key, signals)) % R
    if key.delta % R:
        return Proof(a % R, b % R, ((a * b - t) * pow(key.delta, -1, R) + e) % R)
    c = 1 if c is None else c % R
    if b % R:
        return Proof((t * pow(b, -1, R) + e) % R, b % R, c)
    return Proof(a % R, (t * pow(a, -1, R) + e) % R, c)


# ---- a twist point outside the order-r subgroup --------------------------------------------------------------------------
def _f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def _f2sqrt(a):
    n = (a[0] * a[0] + a[1] * a[1]) % Q
    sn = pow(n, (Q + 1) // 4, Q)
    if sn * sn % Q != n:
        return None
    for sgn in (1, -1):
        t = (a[0] + sgn * sn) * pow(2, -1, Q) % Q
        x0 = pow(t, (Q + 1) // 4, Q)
        if x0 * x0 % Q == t and x0:
            x1 = a[1] * pow(2 * x0, -1, Q) % Q
            if _f2mul((x0, x1), (x0, x1)) == (a[0] % Q, a[1] % Q):
                return (x0, x1)
    return None


def twist_point_outside_subgroup():
    """(x0, x1, y0, y1): on y² = x³ + 3/ξ but not killed by r — x = 1, 2, … until the right side is a square"""
    d = pow(82, -1, Q)
    bt = _f2mul((3, 0), (9 * d % Q, -d % Q))
    for x0 in range(1, 50):
        rhs = _f2mul(_f2mul((x0, 0), (x0, 0)), (x0, 0))
        y = _f2sqrt(((rhs[0] + bt[0]) % Q, (rhs[1] + bt[1]) % Q))
        if y:
            return (x0, 0, y[0], y[1])
    raise AssertionError("no twist point found")


# ---- points ------------------------------------------------------------------------------------------------------------------
class Points:
    """k·G₁ / k·G₂ as standard-form affine integers through the oracle (O = tests' `oracle` module), memoised; ask for many at
    once (`need`, then `resolve`), the fixed-base table is built once per call.  The identity is (0, 0)."""

    def __init__(self, O):
        self.O = O
        self.gen = {g: O.ec_to_affine(g, O.ec_generator(g)) for g in ("g1", "g2")}
        self.memo = {"g1": {}, "g2": {}}
        self.todo = {"g1": set(), "g2": set()}

    def need(self, group, ks):
        for k in ks:
            if k % R not in self.memo[group]:
                self.todo[group].add(k % R)

    def need_items(self, items):
        for k in {id(it.key): it.key for it in items}.values():
            self.need("g1", [k.alpha] + k.ic)
            self.need("g2", [k.beta, k.gamma, k.delta])
        self.need("g1", [x for it in items for x in (it.proof.a, it.proof.c)])
        self.need("g2", [it.proof.b for it in items if not it.proof.b_outside])

    def resolve(self):
        for g in ("g1", "g2"):
            ks = sorted(self.todo[g])
            self.todo[g].clear()
            if not ks:
                continue
            arr = self.O.fixed_base_mul(g, self.gen[g], self.O.ints_to_arr(ks))
            w = 2 if g == "g1" else 4
            flat = self.O.arr_to_ints(arr.reshape(-1, 4))
            for i, k in enumerate(ks):
                self.memo[g][k] = tuple(flat[w * i:w * i + w])

    def g1(self, k):
        return self.memo["g1"][k % R]

    def g2(self, k):
        return self.memo["g2"][k % R]


def _g1_json(p):
    return [str(p[0]), str(p[1]), "1"] if any(p) else ["0", "0", "0"]


def _g2_json(p):
    if not any(p):
        return [["0", "0"], ["0", "0"], ["0", "0"]]
    return [[str(p[0]), str(p[1])], [str(p[2]), str(p[3])], ["1", "0"]]


def vk_json(pts: Points, key: Key) -> str:
    """verification_key.json text (the shape of synth.vk_to_json)"""
    return json.dumps({
        "protocol": "groth16", "curve": "bn128", "nPublic": key.n_public,
        "vk_alpha_1": _g1_json(pts.g1(key.alpha)), "vk_beta_2": _g2_json(pts.g2(key.beta)),
        "vk_gamma_2": _g2_json(pts.g2(key.gamma)), "vk_delta_2": _g2_json(pts.g2(key.delta)),
        "IC": [_g1_json(pts.g1(k)) for k in key.ic],
    })


def proof_json(pts: Points, proof: Proof) -> str:
    b = twist_point_outside_subgroup() if proof.b_outside else pts.g2(proof.b)
    return json.dumps({"pi_a": _g1_json(pts.g1(proof.a)), "pi_b": _g2_json(b), "pi_c": _g1_json(pts.g1(proof.c)),
                       "protocol": "groth16", "curve": "bn128"})


def public_json(signals) -> str:
    return json.dumps([str(s) for s in signals])


# ---- the case table --------------------------------------------------------------------------------------------------------
def _rand(rnd):
    return rnd.randrange(1, R)


def random_key(rnd, n_public, name="", **fixed):
    k = Key(_rand(rnd), _rand(rnd), _rand(rnd), _rand(rnd), [_rand(rnd) for _ in range(n_public + 1)], n_public, name)
    for f, v in fixed.items():
        setattr(k, f, v)
    return k


def proof_variants(key: Key, signals, rnd):
    """the proofs of one (key, signals) pair: (label, proof, signals)"""
    n = key.n_public
    a, b = _rand(rnd), _rand(rnd)
    valid = prove(key, signals, a, b)
    out = [("valid", valid, signals), ("e=1", prove(key, signals, a, b, e=1), signals)]
    if key.delta:
        out.append(("A=O", prove(key, signals, 0, b), signals))
        out.append(("B=O", prove(key, signals, a, 0), signals))
        t = (key.alpha * key.beta + key.gamma * cpub_dlog(key, signals)) % R
        out.append(("C=O", Proof(a, t * pow(a, -1, R) % R, 0), signals))
    else:
        out.append(("A=O", Proof(0, b, 1), signals))       # the model decides: valid only when α·β + γ·cpub ≡ 0
        out.append(("C=O", prove(key, signals, a, b, c=0), signals))
    out.append(("-A", Proof(-valid.a % R, valid.b, valid.c), signals))
    if n:
        j = rnd.randrange(n)
        out.append((f"s{j}+1", valid, signals[:j] + [(signals[j] + 1) % R] + signals[j + 1:]))
        out.append((f"s{j}-1", valid, signals[:j] + [(signals[j] - 1) % R] + signals[j + 1:]))
    if n >= 2:
        i, j = rnd.sample(range(n), 2)
        sw = list(signals)
        sw[i], sw[j] = sw[j], sw[i]
        out.append((f"swap{i},{j}", valid, sw))
        j = rnd.randrange(1, n)
        out.append((f"s{j}+r", valid, signals[:j] + [signals[j] + R] + signals[j + 1:]))
    out.append(("B outside", Proof(valid.a, valid.b, valid.c, b_outside=True), signals))
    return out


def case_table(seed=0x5ea1):
    """[(key, [Item, …]), …]: every key of the table with its proofs (see tests/test_pairing29.py for what each reaches)"""
    rnd = random.Random(seed)
    r = lambda: _rand(rnd)
    e = EDGE_SIGNALS
    keys = []  # (key, [signal vectors])
    keys.append((random_key(rnd, 0, "n=0"), [[]]))
    keys.append((random_key(rnd, 2, "n=2"), [[e[0], e[1]], [e[2], e[3]]]))
    keys.append((random_key(rnd, 3, "n=3"), [[e[4], e[5], e[6]], [e[2]] * 3]))
    keys.append((random_key(rnd, 8, "n=8"), [e + [r()], [e[5]] * 8]))
    keys.append((random_key(rnd, 40, "n=40"), [[r() for _ in range(40)]]))
    k = random_key(rnd, 2, "ic2=ic1")           # Straus: the second addition of the top set bit meets acc = P and doubles
    k.ic[2] = k.ic[1]
    s = r()
    keys.append((k, [[s, s], [R - 1, R - 1]]))
    k = random_key(rnd, 2, "ic2=-ic1")          # Straus: acc = P, then −P at every set bit: cancels to O
    k.ic[2] = -k.ic[1] % R
    keys.append((k, [[s, s], [e[6], e[6]]]))
    k = random_key(rnd, 3, "ic2=O")             # an identity IC entry (ic_zero)
    k.ic[2] = 0
    keys.append((k, [[r(), r(), r()], [e[5]] * 3]))
    k = random_key(rnd, 2, "ic0=O")             # an identity IC₀
    k.ic[0] = 0
    keys.append((k, [[r(), r()]]))
    s = [r(), r()]
    k = random_key(rnd, 2, "ic0=sum")           # the final IC₀ addition meets acc = IC₀ and doubles
    k.ic[0] = (s[0] * k.ic[1] + s[1] * k.ic[2]) % R
    keys.append((k, [s, [r(), r()]]))
    k = random_key(rnd, 2, "ic0=-sum")          # cpub = O: its pairing is left out
    k.ic[0] = -(s[0] * k.ic[1] + s[1] * k.ic[2]) % R
    keys.append((k, [s]))
    keys.append((random_key(rnd, 2, "gamma=0", gamma=0), [[r(), r()]]))
    keys.append((random_key(rnd, 2, "delta=0", delta=0), [[r(), r()]]))
    keys.append((random_key(rnd, 2, "alpha=0", alpha=0), [[r(), r()]]))
    keys.append((random_key(rnd, 2, "beta=0", beta=0), [[r(), r()]]))
    k = random_key(rnd, 2, "IC longer")         # IC entries past n_public + 1 are never read
    k.ic += [r(), 0, r()]
    keys.append((k, [[r(), r()]]))
    table = []
    for key, svecs in keys:
        items = []
        for v, sv in enumerate(svecs):
            for label, proof, sig in proof_variants(key, sv, rnd):
                items.append(Item(key, proof, sig, f"{key.name} signals#{v} {label}"))
        # public.json longer than n_public: the extra entries (one of them ≥ r) are ignored
        v = items[0]
        items.append(Item(key, v.proof, v.signals + [r(), R + 7], f"{key.name} valid, public longer"))
        table.append((key, items))
    return table
