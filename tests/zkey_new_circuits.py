"""The circuits of the groth16_zkey_new tests (tests/test_zkey_new_size.py on the CPU, tests/test_gpu_zkey_new.py on the GPU), all
CONSTRUCTED, and the reading of a key's container that both need."""
import struct

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
FULL = 0x2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f80919 % R
# zero, ±1, ±2, a short one, a word boundary crossed, both sides of the sign rule's boundary, full width (tests/test_zkey_new29.py)
CLASSES = [0, 1, 2, R - 1, R - 2, (1 << 16) - 1, 1 << 127, (R - 1) // 2, (R + 1) // 2, FULL]


def sections(image):
    """{id: (offset of the payload, length)} of an iden3 binary container, and the ids in file order"""
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


def records(image):
    """section 4 as a list of (matrix, row, wire, stored value)"""
    p = payload(image, 4)
    n = struct.unpack_from("<I", p, 0)[0]
    assert len(p) == 4 + 44 * n
    return [struct.unpack_from("<III", p, 4 + 44 * i) + (int.from_bytes(p[16 + 44 * i:48 + 44 * i], "little"),) for i in range(n)]


def stated_records(r):
    """section 4 in the stated order: constraint by constraint, A's terms then B's in the order the .r1cs lists them (write_r1cs
    keeps the order of r's lists within a row), then the public-binding records; the value as the file stores it, v·R² mod r"""
    r2 = pow(2, 512, R)
    rows = [([], []) for _ in range(r.n_constraints)]
    for k, mat in enumerate((r.A, r.B)):
        for (j, i, v) in mat:
            rows[j][k].append((k, j, i, v % R * r2 % R))
    out = [rec for a, b in rows for rec in a + b]
    return out + [(0, r.n_constraints + s, s, r2) for s in range(r.n_public + 1)]


def mixed(S):
    """test_gpu_witness_check.Circuit's R1CS — random_circuit(150, 2, 10, seed=11) plus an all-empty constraint, a 40-term A and a
    wire named twice: 163 wires, 153 constraints — and by hand: wire 163, whose only A terms are (153, 1), (153, 1); wire 164, whose
    only terms in A, B and C cancel in pairs (v, r − v); wire 165, in no matrix; and constraints 155, 156, 157, whose A, B and C
    carry every coefficient class, zero included.  Returns (R1CS, a witness that satisfies it)."""
    r, w = S.random_circuit(150, 2, 10, seed=11)
    long_a = [(151, i, 1000 + 7 * k) for k, i in enumerate(range(20, 60))]
    r.A += long_a
    r.B.append((151, 0, 1))
    r.C.append((151, 0, sum(v * w[i] for _, i, v in long_a) % R))
    r.A += [(152, 5, 2), (152, 5, 3)]
    r.B.append((152, 0, 1))
    r.C.append((152, 0, 5 * w[5] % R))
    assert (r.n_vars, len(w)) == (163, 163)
    w = list(w) + [9, 77, 5]
    r.A += [(153, 163, 1), (153, 163, 1)]
    r.B.append((153, 0, 1))
    r.C.append((153, 0, 18))
    for mat, v in ((r.A, 0x1234567), (r.B, FULL), (r.C, 3)):
        mat += [(154, 164, v), (154, 164, R - v)]
    wires = list(range(20, 20 + len(CLASSES)))
    value = sum(c * w[i] for c, i in zip(CLASSES, wires)) % R
    r.A += [(155, i, c) for c, i in zip(CLASSES, wires)]
    r.B.append((155, 0, 1))
    r.C.append((155, 0, value))
    r.A.append((156, 0, 1))
    r.B += [(156, i, c) for c, i in zip(CLASSES, wires)]
    r.C.append((156, 0, value))
    r.A.append((157, 0, 1))
    r.B.append((157, 0, 1))
    r.C += [(157, i, c) for c, i in zip(CLASSES, wires)] + [(157, 0, (1 - value) % R)]
    r.n_vars, r.n_constraints = 166, 158
    return r, w


def fan(S, n=300):
    """wire 0 and the private wire 2 in A, B and C of every constraint under varying coefficients: columns of n terms"""
    r = S.R1CS(n_vars=3 + n, n_public=1, n_constraints=n)
    for j in range(n):
        c = CLASSES[j % len(CLASSES)]
        r.A += [(j, 0, 1 + j), (j, 2, c if j % 3 else 1)]
        r.B += [(j, 2, (R - 1 - j) if j % 2 else 7 * j + 1), (j, 0, c if j % 4 == 1 else 1)]
        r.C += [(j, 0, (j * j + 1) % R), (j, 3 + j, 1), (j, 2, CLASSES[(j + 3) % len(CLASSES)] if j % 5 else R - 1 - j)]
    return r


def tiny(S):
    """no private wire: section 8 is empty"""
    return S.R1CS(n_vars=3, n_public=2, n_constraints=2, A=[(0, 1, 1), (1, 2, 3)], B=[(0, 2, 1), (1, 0, 1)], C=[(0, 0, 5), (1, 1, 2)])


def circuits(S):
    return {"mixed": mixed(S)[0], "fan": fan(S), "chain6": S.squaring_chain(6)[0], "chain7": S.squaring_chain(7)[0], "tiny": tiny(S)}


def check_r1cs(r, w):
    rows = [[0, 0, 0] for _ in range(r.n_constraints)]
    for k, mat in enumerate((r.A, r.B, r.C)):
        for (j, i, v) in mat:
            rows[j][k] = (rows[j][k] + v * w[i]) % R
    return all(a * b % R == c for a, b, c in rows)
