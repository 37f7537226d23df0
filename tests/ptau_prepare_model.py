"""What groth16_ptau_prepare must write (include/groth16_prover.h), restated with Python integers in the exponent: an unprepared
powers-of-tau file for any (power, τ, α, β), a direct O(n²) inverse transform mod r, and the prepared file's bytes.  Test
infrastructure (tests/test_ptau_prepare_model.py, tests/test_gpu_ptau_prepare.py).  Points come from a caller-supplied
fixed_base_mul(group, scalars) → standard-form affine (the oracle's or the library's generator multiplication), as the
synthesiser's do; nothing here divides by τ − ωʲ, so τ may lie inside a domain."""
import struct

import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
ROU_28 = 0x2A3C09F0A58A7E8500E0A7EB8EF62ABC402D111E41112ED49BD61B6E725B19F0
SOURCE = {12: 2, 13: 3, 14: 4, 15: 5}
ELEM = {2: 64, 3: 128, 4: 64, 5: 64, 12: 64, 13: 128, 14: 64, 15: 64}


def omega(logn):
    w = ROU_28
    for _ in range(28 - logn):
        w = w * w % R
    return w


def inverse_transform(xs, p):
    """out[j] = (1/2^p)·Σ_{i<2^p} ω_p^{−ij}·xs[i]; xs shorter than 2^p is extended with zeros"""
    n = 1 << p
    assert len(xs) <= n
    xs = [x % R for x in xs] + [0] * (n - len(xs))
    wi = pow(omega(p), -1, R)
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * wi % R
    ninv = pow(n, -1, R)
    return [sum(x * pw[i * j & (n - 1)] for i, x in enumerate(xs) if x) % R * ninv % R for j in range(n)]


def source_scalars(power, tau, alpha, beta):
    """discrete logarithms of sections 2, 3, 4, 5"""
    N = 1 << power
    pw = [1] * (2 * N - 1)
    for i in range(1, 2 * N - 1):
        pw[i] = pw[i - 1] * tau % R
    return {2: pw, 3: pw[:N], 4: [alpha * x % R for x in pw[:N]], 5: [beta * x % R for x in pw[:N]]}


def prepared_scalars(power, tau, alpha, beta):
    """discrete logarithms of sections 12 … 15: block p of section s is the inverse transform of the first 2^p elements of its
    source; section 12's block power + 1 has only 2^(power+1) − 1 of them — the last input is zero"""
    src = source_scalars(power, tau, alpha, beta)
    out = {}
    for sid, s in SOURCE.items():
        out[sid] = []
        for p in range(power + (2 if sid == 12 else 1)):
            out[sid] += inverse_transform(src[s][:1 << p], p)
    return out


def _points(group, scalars, fbm, to_mont):
    """file bytes of scalar·G per scalar: affine, Montgomery form, the identity all zero"""
    size = 64 if group == "g1" else 128
    live = [i for i, k in enumerate(scalars) if k % R]
    out = np.zeros((len(scalars), size // 8), dtype=np.uint64)
    if live:
        arr = np.frombuffer(b"".join((scalars[i] % R).to_bytes(32, "little") for i in live), dtype=np.uint64).reshape(-1, 4).copy()
        pts = np.ascontiguousarray(to_mont(np.ascontiguousarray(fbm(group, arr))))
        out[live] = pts.reshape(len(live), -1)
    return out.tobytes()


def _section(sid, payload):
    return struct.pack("<IQ", sid, len(payload)) + payload


def _header(power):
    return struct.pack("<I", 32) + Q.to_bytes(32, "little") + struct.pack("<II", power, power)


def write_unprepared(power, tau, alpha, beta, fbm, to_mont):
    """sections 1 … 7 of the layout DESIGN §7d states, nothing else"""
    src = source_scalars(power, tau, alpha, beta)
    secs = [(1, _header(power))] + [(s, _points("g2" if s == 3 else "g1", src[s], fbm, to_mont)) for s in (2, 3, 4, 5)]
    secs += [(6, _points("g2", [beta], fbm, to_mont)), (7, struct.pack("<I", 0))]
    return b"ptau" + struct.pack("<II", 1, len(secs)) + b"".join(_section(s, p) for s, p in secs)


def expected_prepared(unprepared, power, tau, alpha, beta, fbm, to_mont):
    """the input with sections 12 … 15 appended and the section count adjusted"""
    sc = prepared_scalars(power, tau, alpha, beta)
    n = struct.unpack_from("<I", unprepared, 8)[0]
    tail = b"".join(_section(s, _points("g2" if s == 13 else "g1", sc[s], fbm, to_mont)) for s in (12, 13, 14, 15))
    return unprepared[:8] + struct.pack("<I", n + 4) + unprepared[12:] + tail


def sections(image):
    """{id: (payload offset, length)} and the ids in file order"""
    pos, out, order = 12, {}, []
    for _ in range(struct.unpack_from("<I", image, 8)[0]):
        sid, ln = struct.unpack_from("<IQ", image, pos)
        out[sid] = (pos + 12, ln)
        order.append(sid)
        pos += 12 + ln
    assert pos == len(image)
    return out, order


def payload(image, sid):
    off, ln = sections(image)[0][sid]
    return image[off:off + ln]


def without(image, drop):
    secs, order = sections(image)
    keep = [s for s in order if s not in drop]
    return image[:8] + struct.pack("<I", len(keep)) + b"".join(_section(s, image[secs[s][0]:secs[s][0] + secs[s][1]]) for s in keep)


def with_payload(image, sid, new):
    secs, order = sections(image)
    return image[:12] + b"".join(_section(s, new if s == sid else image[secs[s][0]:secs[s][0] + secs[s][1]]) for s in order)


def prepared_size(power, unprepared_len):
    N = 1 << power
    return unprepared_len + 4 * 12 + (4 * N - 1) * 64 + (2 * N - 1) * (128 + 64 + 64)
