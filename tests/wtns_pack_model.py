"""The packed witness ("wtnz", version 1) in Python integers: the value's encoder and decoder, the container's writer and reader and
the whole-file decoder with its faults.  Nothing here calls the library: every expected byte of tests/test_wtns_pack_host.py and
tests/test_gpu_wtns_pack.py comes from this text.

    v = 0: code 0x00 | v = 1: code 0x40 | m = r − v, bytes(m) < bytes(v): code 0x80 | bytes(m), payload m | else code bytes(v), payload v
"""
import struct

R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BLOCK = 256
MAX_SPAN = BLOCK * 32
CODE, NONCANONICAL, RANGE, DIRECTORY = 1, 2, 3, 4
KIND_TEXT = {CODE: "an undefined code byte", NONCANONICAL: "the value's form is not canonical", RANGE: "32 bytes that are not below r",
             DIRECTORY: "the block's lengths do not sum to its directory span"}


def nbytes(x: int) -> int:
    return (x.bit_length() + 7) // 8


def encode(v: int):
    """→ (code, payload) of 0 <= v < r"""
    assert 0 <= v < R_MOD
    if v == 0:
        return 0x00, b""
    if v == 1:
        return 0x40, b""
    m = R_MOD - v
    if nbytes(m) < nbytes(v):
        return 0x80 | nbytes(m), m.to_bytes(nbytes(m), "little")
    return nbytes(v), v.to_bytes(nbytes(v), "little")


def code_len(c: int):
    """payload bytes of a code byte; None: undefined"""
    if c in (0x00, 0x40):
        return 0
    if 0x01 <= c <= 0x20:
        return c
    if 0x81 <= c <= 0x9f:
        return c & 0x7f
    return None


def decode(c: int, payload: bytes):
    """→ (value, 0) or (None, kind); payload has code_len(c) bytes"""
    ln = code_len(c)
    if ln is None:
        return None, CODE
    assert len(payload) == ln
    if c == 0x00:
        return 0, 0
    if c == 0x40:
        return 1, 0
    if payload[-1] == 0:
        return None, NONCANONICAL
    x = int.from_bytes(payload, "little")
    if c & 0x80:
        return R_MOD - x, 0
    if x == 1:
        return None, NONCANONICAL
    if ln == 32:
        if x >= R_MOD:
            return None, RANGE
        if nbytes(R_MOD - x) < 32:
            return None, NONCANONICAL
    return x, 0


# ---- containers
def sections(kind: bytes, secs, version: int = 1) -> bytes:
    out = kind + struct.pack("<II", version, len(secs))
    for sid, data in secs:
        out += struct.pack("<IQ", sid, len(data)) + data
    return out


def read_sections(image: bytes):
    """{id: payload} of an iden3 container (every id once)"""
    nsec = struct.unpack_from("<I", image, 8)[0]
    pos, out = 12, {}
    for _ in range(nsec):
        sid, ln = struct.unpack_from("<IQ", image, pos)
        out[sid] = image[pos + 12:pos + 12 + ln]
        pos += 12 + ln
    return out


def wtns_header(n: int, q: int = R_MOD) -> bytes:
    return struct.pack("<I", 32) + q.to_bytes(32, "little") + struct.pack("<I", n)


def write_wtns(values, q: int = R_MOD) -> bytes:
    """a .wtns of sections 1 and 2, version 2; values may be >= r (32 bytes each)"""
    return sections(b"wtns", [(1, wtns_header(len(values), q)), (2, b"".join(int(v).to_bytes(32, "little") for v in values))], version=2)


def wtns_values(image: bytes):
    body = read_sections(image)[2]
    return [int.from_bytes(body[i:i + 32], "little") for i in range(0, len(body), 32)]


def pack_parts(values):
    """→ (codes, directory entries, payload) of the values"""
    codes, payload, directory = bytearray(), bytearray(), []
    for i, v in enumerate(values):
        if i % BLOCK == 0:
            directory.append(len(payload))
        c, p = encode(v)
        codes.append(c)
        payload += p
    directory.append(len(payload))
    return bytes(codes), directory, bytes(payload)


def container(n: int, codes: bytes, directory, payload: bytes, q: int = R_MOD, order=(1, 2, 3, 4)) -> bytes:
    body = {1: wtns_header(n, q), 2: codes, 3: b"".join(struct.pack("<Q", d) for d in directory), 4: payload}
    return sections(b"wtnz", [(s, body[s]) for s in order])


def pack(values) -> bytes:
    """the packed witness of the values, as groth16_wtns_pack writes it (sections 1, 2, 3, 4)"""
    codes, directory, payload = pack_parts(values)
    return container(len(values), codes, directory, payload)


def packed_size(values) -> int:
    return 12 + 4 * 12 + 40 + len(values) + 8 * ((len(values) + BLOCK - 1) // BLOCK + 1) + sum(len(encode(v)[1]) for v in values)


def unpack(image: bytes):
    """a packed witness whose container a reader accepts → (values, faults): faults is the list of (element, kind) in element
    order — a block whose lengths do not sum to its span reports DIRECTORY at its first element and nothing else; a faulty
    element's value is None"""
    secs = read_sections(image)
    n = struct.unpack_from("<I", secs[1], 36)[0]
    codes, payload = secs[2], secs[4]
    directory = [struct.unpack_from("<Q", secs[3], 8 * i)[0] for i in range(len(secs[3]) // 8)]
    values, faults = [], []
    for b in range((n + BLOCK - 1) // BLOCK):
        blk = codes[b * BLOCK:min(n, (b + 1) * BLOCK)]
        lens = [code_len(c) or 0 for c in blk]
        if sum(lens) != directory[b + 1] - directory[b]:
            faults.append((b * BLOCK, DIRECTORY))
            values += [None] * len(blk)
            continue
        pos = directory[b]
        for k, c in enumerate(blk):
            v, kind = decode(c, payload[pos:pos + lens[k]]) if code_len(c) is not None else (None, CODE)
            if kind:
                faults.append((b * BLOCK + k, kind))
            values.append(v)
            pos += lens[k]
    return values, faults


def edge_values():
    """the values at which a rule of the encoding changes"""
    r = R_MOD
    return [0, 1, 2, 255, 256, (1 << 248) - 1, 1 << 248, (r - 1) // 2, (r + 1) // 2, r - (1 << 248) - 1, r - (1 << 248), r - (1 << 248) + 1, r - 256, r - 255,
            r - 2, r - 1]
