"""The host half of groth16_zkey_pack / groth16_zkey_unpack / groth16_cache_load_packed: the two size functions and the packed
container's reader (zkez_layout, zkez_coefs_layout) against tests/zkey_pack_model.py.  The packed key is the model's — the golden
key packed by Python integers — and every refusal here is decided before any device call: none of these tests initialises a GPU,
and on a machine without one they would see −5 instead of the −2 / −3 they assert."""
import ctypes as C
import struct

import pytest

import zkey_corpus as ZC
import zkey_pack_model as ZM

POINT_WORD = {3: 32, 5: 32, 6: 32, 7: 64, 8: 32, 9: 32}


@pytest.fixture(scope="module")
def zkey():
    return ZC.golden_zkey()


@pytest.fixture(scope="module")
def zkez(zkey):
    return ZM.pack_file(zkey)


def test_the_models_packed_key_is_what_the_format_says(zkey, zkez):
    """conditions on the model's own output, before anything is compared with it"""
    assert zkez[:12] == b"zkez" + struct.pack("<I", 1) + zkey[8:12]
    a, b = ZM.sections(zkey), ZM.sections(zkez)
    assert [s for s, _ in a] == [s for s, _ in b]
    for (sid, p), (_, q) in zip(a, b):
        if sid in ZM.POINT_BYTES:
            assert 2 * len(q) == len(p)
        elif sid == 4:
            declared, n, pb, triples, codes, directory, payload = ZM.body_parts(q)
            assert (declared, n) == (struct.unpack_from("<I", p, 0)[0], (len(p) - 4) // 44) and directory[0] == 0 and directory[-1] == pb == len(payload)
            assert triples == b"".join(p[4 + 44 * k:16 + 44 * k] for k in range(n))
            assert ZM.unpack_body(q) == (p[4:], [])
            # a key's coefficients are small: ±1 and little else
            assert set(codes) <= {0x40, 0x81, 0x01, 0x02, 0x03} and len(q) < len(p) // 2
        else:
            assert p == q
    points = sum(len(p) for sid, p in a if sid in ZM.POINT_BYTES)
    assert len(zkez) == len(zkey) - points // 2 - len(ZM.payload(zkey, 4)) + len(ZM.payload(zkez, 4))


def test_the_size_functions(K, zkey, zkez):
    assert K.zkey_unpacked_size(zkez) == len(zkey)
    assert K.zkey_packed_bound(zkey) == ZM.packed_bound(zkey) >= len(zkez)
    # bytes behind the last section are no part of either container
    assert K.zkey_unpacked_size(zkez + b"tail") == len(zkey) and K.zkey_packed_bound(zkey + b"tail") == ZM.packed_bound(zkey)
    # an unknown section and a longer section 10 are carried over
    more = ZM.container(ZM.sections(zkey) + [(77, b"x" * 1001)], magic=b"zkey")
    assert K.zkey_unpacked_size(ZM.pack_file(more)) == len(more) and K.zkey_packed_bound(more) == ZM.packed_bound(more)
    with pytest.raises(K.ProverError, match=r"\(-2\): Invalid File format \(expected 'zkez'\)"):
        K.zkey_unpacked_size(zkey)
    with pytest.raises(K.ProverError, match=r"\(-2\): Invalid File format \(expected 'zkey'\)"):
        K.zkey_packed_bound(zkez)


def _last_error(K):
    K.lib().groth16_last_error.restype = C.c_char_p
    return K.lib().groth16_last_error().decode()


def _every_reader(K, image):
    """(code, text) of each entry that reads a packed key, the GPU ones with a device string that would open device 0"""
    lib, out = K.lib(), []
    size = C.c_uint64()
    out.append((lib.groth16_zkey_unpacked_size(image, C.c_size_t(len(image)), C.byref(size)), _last_error(K)))
    rep, buf = K.ZkeyPackReport(), C.create_string_buffer(1 << 20)
    out.append((lib.groth16_zkey_unpack(image, C.c_size_t(len(image)), buf, C.c_size_t(len(buf)), b"HIP", C.byref(rep)), _last_error(K)))
    cm = K.CacheManager()
    try:
        out.append((lib.groth16_cache_load_packed(cm._h, b"k", image, C.c_size_t(len(image)), 0, 0, 1), _last_error(K)))
        assert not cm.contains("k")
    finally:
        cm.close()
    return out


def _refused(K, image, text, code=-2):
    for rc, msg in _every_reader(K, image):
        assert rc == code and text in msg, (rc, msg)


def test_each_form_is_refused_by_the_others_readers(K, zkey, zkez):
    _refused(K, zkey, "Invalid File format (expected 'zkez')")
    _refused(K, b"ptaz" + zkez[4:], "Invalid File format (expected 'zkez')")
    _refused(K, zkez[:4] + struct.pack("<I", 2) + zkez[8:], "Version not supported")
    cm = K.CacheManager()
    try:
        with pytest.raises(K.ProverError, match=r"\(-2\): Invalid File format \(expected 'zkey'\)"):
            cm.load("k", zkez)
        assert not cm.contains("k")
    finally:
        cm.close()
    rep = K.ZkeyPackReport()
    assert K.lib().groth16_zkey_pack(zkez, C.c_size_t(len(zkez)), None, C.c_size_t(0), b"HIP", C.byref(rep)) == -2
    assert "Invalid File format (expected 'zkey')" in _last_error(K)
    for call in (K.zkey_check, K.zkey_export_vk):
        with pytest.raises(K.ProverError, match=r"Invalid File format \(expected 'zkey'\)"):
            call(zkez)


def test_packing_reads_the_key_through_the_key_checks_reader(K, zkey):
    """need_ic: a key without section 3, which the prover loads, is refused with the reader's message"""
    rep = K.ZkeyPackReport()
    for bad, text in ((ZM.container(ZC.without(ZM.sections(zkey), 3), magic=b"zkey"), "Missing section 3"),
                      (ZM.container(ZC.resized(ZM.sections(zkey), 5, -64), magic=b"zkey"), "zkey: point section size mismatch"),
                      (ZM.container(ZC.resized(ZM.sections(zkey), 4, -1), magic=b"zkey"), "zkey: coefficient section size")):
        assert K.lib().groth16_zkey_pack(bad, C.c_size_t(len(bad)), None, C.c_size_t(0), b"HIP", C.byref(rep)) == -2 and text in _last_error(K)
        with pytest.raises(K.ProverError, match=text):
            K.zkey_packed_bound(bad)


def test_every_point_section_one_word_short_and_one_word_long(K, zkey, zkez):
    nv, npub, dom = struct.unpack_from("<III", ZM.payload(zkey, 2), 72)
    for sid, word in POINT_WORD.items():
        p = ZM.payload(zkez, sid)
        for bad in (p[:-word], p + bytes(word)):
            _refused(K, ZM.with_section(zkez, sid, bad), "zkez: section %d holds %d bytes, a packed key of %d wires, %d public signals and domain %d has %d" % (sid, len(bad), nv, npub, dom, len(p)))


def test_section_4_against_the_sum_of_its_parts(K, zkez):
    b = ZM.payload(zkez, 4)
    declared, n, pb, triples, codes, directory, payload = ZM.body_parts(b)
    text = "zkez: section 4 holds %d bytes, %d coefficients with a payload of %d bytes have %d"
    _refused(K, ZM.with_section(zkez, 4, b[:-1]), text % (len(b) - 1, n, pb, len(b)))
    _refused(K, ZM.with_section(zkez, 4, b + b"\0"), text % (len(b) + 1, n, pb, len(b)))
    # n_coef disagreeing with the size, one way and the other
    for m in (n - 1, n + 1):
        want = 16 + 13 * m + 8 * ((m + 255) // 256 + 1) + pb
        _refused(K, ZM.with_section(zkez, 4, b[:4] + struct.pack("<I", m) + b[8:]), text % (len(b), m, pb, want))
    # a payload size no section can hold
    _refused(K, ZM.with_section(zkez, 4, b[:8] + struct.pack("<Q", (1 << 64) - 13 * n - 16) + b[16:]), "zkez: section 4 holds %d bytes, %d coefficients with a payload of %d bytes have 0" % (len(b), n, (1 << 64) - 13 * n - 16))
    _refused(K, ZM.with_section(zkez, 4, b[:15]), "zkez: section 4 holds 15 bytes, its three counts alone have 16")
    # the declared count is carried, not read
    for rc, _ in _every_reader(K, ZM.with_section(zkez, 4, struct.pack("<I", 0xdeadbeef) + b[4:]))[:1]:
        assert rc == 0


def test_the_directory(K, zkez):
    """a body of 300 coefficients (two blocks) in the golden key's place: the directory is judged before the coefficient count is
    held against anything else"""
    records = ZM.records_of([(1 << 64) + k for k in range(300)])
    triples, codes, directory, payload = ZM.coefs_parts(records)
    assert directory == [0, 256 * 9, 300 * 9]

    def image(d, pay=payload):
        return ZM.with_section(zkez, 4, ZM.body(300, triples, codes, d, pay))

    assert _every_reader(K, image(directory))[0][0] == 0
    _refused(K, image([1, 256 * 9, 300 * 9]), "zkez: directory entry 0 is 1, not 0")
    _refused(K, image([0, 2800, 2700]), "zkez: directory entry 2 is below entry 1")
    _refused(K, image([0, 256 * 9, 300 * 9 - 1]), "zkez: the directory ends at 2699, the payload holds 2700 bytes")
    _refused(K, image([0, 256 * 9, 300 * 9 + 1]), "zkez: the directory ends at 2701, the payload holds 2700 bytes")
    big = bytes(9000)
    _refused(K, image([0, 8193, 9000], big), "zkez: block 0 spans 8193 bytes, 8192 is the most")
    _refused(K, image([0, 100, 9000], big), "zkez: block 1 spans 8900 bytes, 8192 is the most")
    assert _every_reader(K, image([0, 8192, 9000], big))[0][0] == 0          # (host-valid: the kernel's sum test is what refuses it)


def test_doubled_missing_and_truncated(K, zkez):
    secs = ZM.sections(zkez)
    for sid in (1, 2, 3, 4, 7, 9):
        _refused(K, ZM.container(ZC.doubled(secs, sid)), "Section Duplicated %d" % sid)
        _refused(K, ZM.container(ZC.without(secs, sid)), "Missing section %d" % sid)
    _refused(K, zkez[:-3], "exceeds the file")
    _refused(K, zkez[:20], "truncated section table")
    # the header's rules are the .zkey's
    h = bytearray(ZM.payload(zkez, 2))
    h[4] ^= 1
    _refused(K, ZM.with_section(zkez, 2, bytes(h)), "zkey: not a BN254 key")
    _refused(K, ZM.with_section(zkez, 1, struct.pack("<I", 2)), "Protocol not supported")


def test_arguments(K, zkez):
    with pytest.raises(K.ProverError, match=r"\(-3\).*does not name one HIP device"):
        K.zkey_unpack(zkez, device="HIP:0-1")
    cm = K.CacheManager()
    try:
        with pytest.raises(K.ProverError, match=r"\(-3\): shard 1 of 2: groth16_cache_load_packed takes single-device keys"):
            cm.load_packed("k", zkez, shard_rank=1, shard_count=2)
    finally:
        cm.close()
    # the raw codec's reader is section 4's
    with pytest.raises(K.ProverError, match=r"\(-2\): zkez: section 4 holds 23 bytes"):
        K.coefs_unpack(ZM.coefs_body(b"")[:-1])
