"""The constructed keys and circuits of the groth16_zkey_verify_ptau tests, as scalars: every case is (circuit for the handle, key
scalars, header scalars) with the first kind it must be reported under.  tests/test_zkey_verify_model.py runs them through the
discrete-log model alone; tests/test_gpu_zkey_verify.py builds the files from the same scalars and asks the library."""
import copy

import zkey_verify_dlog_model as M

R = M.R


def base_circuit(S):
    """test_gpu_witness_check's circuit (163 wires, 153 constraints, npub 2, domain 256), built without a GPU"""
    r, w = S.random_circuit(150, 2, 10, seed=11)
    long_a = [(151, i, 1000 + 7 * k) for k, i in enumerate(range(20, 60))]
    r.A += long_a
    r.B.append((151, 0, 1))
    r.C.append((151, 0, sum(v * w[i] for _, i, v in long_a) % R))
    r.A += [(152, 5, 2), (152, 5, 3)]
    r.B.append((152, 0, 1))
    r.C.append((152, 0, 5 * w[5] % R))
    r.n_constraints = 153
    return r


def other_toxic(S, tau=False, alpha_beta=False, gamma_delta=False):
    """the default toxic waste with some of it replaced by another seed's"""
    a, b = S.toxic_waste(), S.toxic_waste(0xD1FF)
    pick = [tau, alpha_beta, alpha_beta, gamma_delta, gamma_delta]
    return tuple(y if p else x for x, y, p in zip(a, b, pick))


def header_of(toxic):
    tau, alpha, beta, gamma, delta = toxic
    return dict(alpha1=alpha, beta1=beta, beta2=beta, gamma2=gamma, delta1=delta, delta2=delta)


def swapped(xs, lo=0):
    """xs with its first two DISTINCT elements at or above lo exchanged, and their positions"""
    i = lo
    j = next(k for k in range(i + 1, len(xs)) if xs[k] != xs[i])
    out = list(xs)
    out[i], out[j] = out[j], out[i]
    return out, (i, j)


def with_c_plus_one(r, public):
    """the circuit with one coefficient of C raised by 1: on wire 0 (a public column) or on the first private wire C names"""
    out = copy.deepcopy(r)
    k = next(k for k, (j, i, v) in enumerate(out.C) if (i <= r.n_public) == public)
    j, i, v = out.C[k]
    out.C[k] = (j, i, (v + 1) % R)
    return out


def plain_domain_h(S, r, toxic):
    """section 9 built on the domain itself instead of its odd coset: L_i(τ)·(τⁿ − 1)/(−2δ)"""
    tau, delta = toxic[0], toxic[4]
    n = S.key_scalars(r, toxic)["n"]
    zt = (pow(tau, n, R) - 1) * pow((-2 * delta) % R, -1, R) % R
    return [x * zt % R for x in S.lagrange_at(n, n.bit_length() - 1, tau)]


def cases(S, r=None):
    """[(name, circuit of the handle, key, header, first kind, exact mask or None)] over the default ptau (S.toxic_waste()'s τ, α, β)"""
    r = r or base_circuit(S)
    toxic = S.toxic_waste()
    base = M.key_from(S.key_scalars(r, toxic))
    hdr = header_of(toxic)
    out = [("untouched", r, base, hdr, 0, 0)]
    gd = other_toxic(S, gamma_delta=True)
    out.append(("other gamma and delta", r, M.key_from(S.key_scalars(r, gd)), header_of(gd), 0, 0))
    for name, kind in (("a", M.A), ("b1", M.B1), ("b2", M.B2), ("c", M.C), ("h", M.H), ("ic", M.IC)):
        key = dict(base)
        key[name], (i, j) = swapped(base[name])
        assert base[name][i] != base[name][j]
        out.append((f"two points of {name} swapped", r, key, hdr, kind, M.bit(kind)))
    out.append(("C coefficient of a private wire", with_c_plus_one(r, False), base, hdr, M.C, M.bit(M.C)))
    out.append(("C coefficient of a public wire", with_c_plus_one(r, True), base, hdr, M.IC, M.bit(M.IC)))
    same_size, _ = S.random_circuit(150, 2, 10, seed=12)
    same_size.n_constraints = 153
    out.append(("another circuit of the same sizes", same_size, base, hdr, M.A, None))
    tt = other_toxic(S, tau=True)
    out.append(("another tau, header alpha and beta the ptau's", r, M.key_from(S.key_scalars(r, tt)), header_of(tt), M.A, None))
    ta = other_toxic(S, tau=True, alpha_beta=True)
    out.append(("another tau, alpha and beta", r, M.key_from(S.key_scalars(r, ta)), header_of(ta), M.HEADER, None))
    out.append(("built with another delta than the header's", r, M.key_from(S.key_scalars(r, toxic[:4] + (gd[4],))), hdr, M.C, M.bit(M.C) | M.bit(M.H)))
    key = dict(base)
    key["h"] = plain_domain_h(S, r, toxic)
    out.append(("H on the plain domain", r, key, hdr, M.H, M.bit(M.H)))
    return out
