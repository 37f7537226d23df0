"""The packed proving key ("zkez", version 1; include/groth16_prover.h) in Python integers: the coefficient's value
v = file·R⁻² mod r through tests/wtns_pack_model.py's codec, the points through tests/point_pack_model.py, the body of section 4,
the container's writer and the decoder of a body with its faults.  Nothing here calls the library: every expected byte of
tests/test_zkey_pack29.py, tests/test_zkey_pack_host.py and tests/test_gpu_zkey_pack.py comes from this text."""
import struct

import point_pack_model as PK
import wtns_pack_model as WM

R_MOD = WM.R_MOD
MONT = 1 << 256
R2 = MONT * MONT % R_MOD
R2_INV = pow(R2, -1, R_MOD)
BLOCK = WM.BLOCK
RECORD = 44
POINT_BYTES = {3: 64, 5: 64, 6: 64, 7: 128, 8: 64, 9: 64}                    # a packed element has half of it
CODE, NONCANONICAL, RANGE, DIRECTORY = WM.CODE, WM.NONCANONICAL, WM.RANGE, WM.DIRECTORY
KIND_TEXT = WM.KIND_TEXT


def to_file(v: int) -> int:
    """the 256-bit integer section 4 stores for the standard-form coefficient v"""
    return v * R2 % R_MOD


def from_file(f: int) -> int:
    assert 0 <= f < R_MOD
    return f * R2_INV % R_MOD


def encode_file(f: int):
    """→ (code, payload) of a file value below r"""
    return WM.encode(from_file(f))


def decode_file(c: int, payload: bytes):
    """→ (file value, 0) or (None, kind)"""
    v, kind = WM.decode(c, payload)
    return (None, kind) if kind else (to_file(v), 0)


# ---- records and the body of section 4
def records_of(values, triples=None) -> bytes:
    """n records {m, c, s, v·R²} of standard-form values; the triples default to (k % 2, k, k + 1)"""
    out = bytearray()
    for k, v in enumerate(values):
        m, c, s = triples[k] if triples is not None else (k % 2, k, k + 1)
        out += struct.pack("<III", m, c, s) + to_file(v).to_bytes(32, "little")
    return bytes(out)


def record_values(records: bytes):
    """the standard-form values of n records"""
    return [from_file(int.from_bytes(records[i + 12:i + 44], "little")) for i in range(0, len(records), RECORD)]


def coefs_parts(records: bytes, replace=None):
    """→ (triples, codes, directory entries, payload) of n records; replace: {element: (code, payload)} put in its place"""
    assert len(records) % RECORD == 0
    triples, codes, payload, directory = bytearray(), bytearray(), bytearray(), []
    for k in range(len(records) // RECORD):
        rec = records[k * RECORD:(k + 1) * RECORD]
        if k % BLOCK == 0:
            directory.append(len(payload))
        c, p = (replace or {}).get(k) or encode_file(int.from_bytes(rec[12:], "little"))
        triples += rec[:12]
        codes.append(c)
        payload += p
    directory.append(len(payload))
    return bytes(triples), bytes(codes), directory, bytes(payload)


def body(declared: int, triples: bytes, codes: bytes, directory, payload: bytes, n=None, payload_bytes=None) -> bytes:
    n = len(codes) if n is None else n
    payload_bytes = len(payload) if payload_bytes is None else payload_bytes
    return struct.pack("<IIQ", declared, n, payload_bytes) + triples + codes + b"".join(struct.pack("<Q", d) for d in directory) + payload


def coefs_body(records: bytes, declared=None, replace=None) -> bytes:
    """the packed body of n records as groth16_zkey_coefs_pack writes it (declared_count = n unless given)"""
    n = len(records) // RECORD
    return body(n if declared is None else declared, *coefs_parts(records, replace))


def body_parts(b: bytes):
    """→ (declared, n, payload_bytes, triples, codes, directory entries, payload) of a body whose size is the sum of its parts"""
    declared, n, pb = struct.unpack_from("<IIQ", b, 0)
    nb = (n + BLOCK - 1) // BLOCK
    o = 16
    triples, o = b[o:o + 12 * n], o + 12 * n
    codes, o = b[o:o + n], o + n
    directory, o = [struct.unpack_from("<Q", b, o + 8 * i)[0] for i in range(nb + 1)], o + 8 * (nb + 1)
    assert len(b) == o + pb
    return declared, n, pb, triples, codes, directory, b[o:]


def unpack_body(b: bytes):
    """a body a reader accepts → (records with zero records at the faulty elements, faults): faults is the list of (element, kind) in
    element order — a block whose lengths do not sum to its span reports DIRECTORY at its first element and nothing else"""
    _, n, _, triples, codes, directory, payload = body_parts(b)
    out, faults = bytearray(), []
    for blk in range((n + BLOCK - 1) // BLOCK):
        cs = codes[blk * BLOCK:min(n, (blk + 1) * BLOCK)]
        lens = [WM.code_len(c) or 0 for c in cs]
        if sum(lens) != directory[blk + 1] - directory[blk]:
            faults.append((blk * BLOCK, DIRECTORY))
            out += bytes(RECORD * len(cs))
            continue
        pos = directory[blk]
        for k, c in enumerate(cs):
            e = blk * BLOCK + k
            f, kind = decode_file(c, payload[pos:pos + lens[k]]) if WM.code_len(c) is not None else (None, CODE)
            if kind:
                faults.append((e, kind))
                out += bytes(RECORD)
            else:
                out += triples[12 * e:12 * e + 12] + f.to_bytes(32, "little")
            pos += lens[k]
    return bytes(out), faults


# ---- the container
def sections(image: bytes):
    """[(id, payload)] of a snarkjs binary container, in file order"""
    n = struct.unpack_from("<I", image, 8)[0]
    pos, out = 12, []
    for _ in range(n):
        sid, ln = struct.unpack_from("<IQ", image, pos)
        out.append((sid, bytes(image[pos + 12:pos + 12 + ln])))
        pos += 12 + ln
    return out


def container(secs, magic=b"zkez", version=1) -> bytes:
    return magic + struct.pack("<II", version, len(secs)) + b"".join(struct.pack("<IQ", sid, len(p)) + p for sid, p in secs)


def pack_section(sid: int, p: bytes) -> bytes:
    if sid in POINT_BYTES:
        return PK.pack_points(p, POINT_BYTES[sid] == 128)
    if sid == 4:
        return coefs_body(p[4:], declared=struct.unpack_from("<I", p, 0)[0])
    return p


def pack_file(zkey: bytes) -> bytes:
    """the packed key of a sound .zkey: magic zkez, version 1, the sections in the key's order, the point sections and section 4
    packed, every other section byte for byte"""
    return container([(sid, pack_section(sid, p)) for sid, p in sections(zkey)])


def with_section(image: bytes, sid: int, payload: bytes) -> bytes:
    return container([(i, payload if i == sid else p) for i, p in sections(image)], magic=image[:4], version=struct.unpack_from("<I", image, 4)[0])


def payload(image: bytes, sid: int) -> bytes:
    return dict(sections(image))[sid]


def packed_bound(zkey: bytes) -> int:
    """every value at 32 payload bytes"""
    total = 12
    for sid, p in sections(zkey):
        n = (len(p) - 4) // RECORD
        total += 12 + (len(p) // 2 if sid in POINT_BYTES else 16 + 45 * n + 8 * ((n + BLOCK - 1) // BLOCK + 1) if sid == 4 else len(p))
    return total
