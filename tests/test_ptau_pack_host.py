"""The host half of groth16_ptau_pack / groth16_ptau_unpack: the two size functions and the packed container's reader
(ptau_packed_layout) against tests/point_pack_model.py.  The files are the model's — tests/ptau_prepare_model.py's images over the
oracle's generator multiplication, packed by Python integers — and every refusal here is decided before any device call: none of
these tests initialises a GPU, and on a machine without one they would see −5 instead of the −2 / −3 they assert.  Parameters, never
measurements."""
import struct

import pytest

import point_pack_model as PK
import ptau_prepare_model as PM

TOXIC = (0x1234567, 0x89abcde, 0xf012345)


class World:
    def __init__(self, K, O):
        self.K = K
        G = {g: O.ec_to_affine(g, O.ec_generator(g)) for g in ("g1", "g2")}
        fbm = lambda g, sc: O.fixed_base_mul(g, G[g], sc)
        to_mont = lambda a: O.fq_convert_montgomery(a, True)
        self.raw = {p: PM.write_unprepared(p, *TOXIC, fbm, to_mont) for p in (0, 1, 3)}
        self.prepared = {p: PM.expected_prepared(self.raw[p], p, *TOXIC, fbm, to_mont) for p in (0, 1, 3)}
        self.packed = {p: PK.pack_file(self.raw[p]) for p in (0, 1, 3)}
        self.packed_prepared = {p: PK.pack_file(self.prepared[p]) for p in (0, 1, 3)}


@pytest.fixture(scope="module")
def world(K, O):
    return World(K, O)


def test_the_models_packed_file_is_what_the_format_says(world):
    """conditions on the model's own output, before anything is compared with it"""
    for p in (0, 1, 3):
        N = 1 << p
        for image, packed, prepared in ((world.raw[p], world.packed[p], False), (world.prepared[p], world.packed_prepared[p], True)):
            assert packed[:12] == b"ptaz" + image[4:12] and len(packed) == PK.packed_size(p, prepared) and len(image) == PK.unpacked_size(p, prepared)
            secs, order = PM.sections(packed)
            assert order == PM.sections(image)[1]
            want = {2: (2 * N - 1) * 32, 3: N * 64, 4: N * 32, 5: N * 32, 6: 64}
            if prepared:
                want.update({12: (4 * N - 1) * 32, 13: (2 * N - 1) * 64, 14: (2 * N - 1) * 32, 15: (2 * N - 1) * 32})
            assert {s: ln for s, (_, ln) in secs.items() if s in want} == want
            assert PM.payload(packed, 1) == PM.payload(image, 1) and PM.payload(packed, 7) == PM.payload(image, 7)
            # section 2 element 0 is the generator: x as the file holds it, a clear sign bit or a set one, never the flag
            first = PM.payload(packed, 2)[:32]
            assert first[:31] == PM.payload(image, 2)[:31] and first[31] & 0x3f == PM.payload(image, 2)[31] and not first[31] & 0x40


@pytest.mark.parametrize("power", [0, 1, 3, 7, 27])
@pytest.mark.parametrize("prepared", [False, True])
def test_the_size_functions(K, power, prepared):
    N = 1 << power
    points = (2 * N - 1) * 64 + N * 128 + 2 * N * 64 + 128 + ((4 * N - 1) * 64 + (2 * N - 1) * 256 if prepared else 0)
    nsec = 11 if prepared else 7
    for extra in (0, 740 + 5, 12 + 1000):                                    # a fresh file; a record in section 7; an unknown section
        ptau = 12 + 12 * nsec + 44 + 4 + points + extra
        packed = ptau - points // 2
        assert ptau == PK.unpacked_size(power, prepared, 44 + 4 + extra) and packed == PK.packed_size(power, prepared, 44 + 4 + extra)
        assert K.ptau_packed_size(power, prepared, ptau) == packed
        assert K.ptau_unpacked_size(power, prepared, packed) == ptau


def test_the_size_functions_on_the_models_files(world):
    K = world.K
    for p in (0, 1, 3):
        assert K.ptau_packed_size(p, False, len(world.raw[p])) == len(world.packed[p])
        assert K.ptau_packed_size(p, True, len(world.prepared[p])) == len(world.packed_prepared[p])
        assert K.ptau_unpacked_size(p, False, len(world.packed[p])) == len(world.raw[p])
        assert K.ptau_unpacked_size(p, True, len(world.packed_prepared[p])) == len(world.prepared[p])


def test_the_size_functions_refuse(K):
    for f in (K.ptau_packed_size, K.ptau_unpacked_size):
        with pytest.raises(K.ProverError, match=r"\(-3\).*above 27"):
            f(28, False, 1 << 40)
        with pytest.raises(K.ProverError, match=r"\(-3\).*at least"):
            f(3, True, 100)
    least = 12 + 12 * 7 + 44 + 64 + 128 + 2 * 64 + 128                       # power 0, without section 7's payload
    assert K.ptau_packed_size(0, False, least) == least - (32 + 64 + 2 * 32 + 64)
    with pytest.raises(K.ProverError, match=r"\(-3\)"):
        K.ptau_packed_size(0, False, least - 1)


def _refused(K, call, image, text, code=-2):
    with pytest.raises(K.ProverError, match=r"\(%d\)" % code) as e:
        call(image)
    assert text in str(e.value), str(e.value)


def _section(sid, payload):
    return struct.pack("<IQ", sid, len(payload)) + payload


def test_the_packed_reader_refuses(world):
    K = world.K
    raw, packed, pp = world.raw[1], world.packed[1], world.packed_prepared[1]
    # a wrong magic, in either direction; each form handed to the other's reader
    _refused(K, K.ptau_unpack, b"zkey" + packed[4:], "Invalid File format (expected 'ptaz')")
    _refused(K, K.ptau_pack, b"zkey" + raw[4:], "Invalid File format (expected 'ptau')")
    _refused(K, K.ptau_unpack, raw, "Invalid File format (expected 'ptaz')")
    _refused(K, K.ptau_unpack, world.prepared[1], "Invalid File format (expected 'ptaz')")
    _refused(K, K.ptau_pack, packed, "Invalid File format (expected 'ptau')")
    _refused(K, K.ptau_pack, pp, "Invalid File format (expected 'ptau')")
    _refused(K, K.ptau_unpack, b"ptaz" + struct.pack("<I", 2) + packed[8:], "Version not supported")
    # a section one element short and one element long
    for image, sid, elem in ((packed, 2, 32), (packed, 3, 64), (packed, 5, 32), (packed, 6, 64), (pp, 12, 32), (pp, 13, 64), (pp, 15, 32)):
        p = PM.payload(image, sid)
        want = PK.packed_section_bytes(1, sid)
        assert len(p) == want
        for bad in (p[:-elem], p + bytes(elem)):
            _refused(K, K.ptau_unpack, PM.with_payload(image, sid, bad), "ptau: section %d holds %d bytes, a packed file of power 1 has %d" % (sid, len(bad), want))
    # a duplicated section
    dup = packed[:8] + struct.pack("<I", 8) + packed[12:] + _section(4, PM.payload(packed, 4))
    _refused(K, K.ptau_unpack, dup, "Section Duplicated 4")
    _refused(K, K.ptau_unpack, PM.without(packed, {5}), "Missing section 5")
    # three of sections 12 to 15
    _refused(K, K.ptau_unpack, PM.without(pp, {14}), "3 of the sections 12 to 15 are present")
    # a truncated file
    _refused(K, K.ptau_unpack, packed[:-3], "section 7 exceeds the file")
    _refused(K, K.ptau_unpack, packed[:20], "truncated section table")
    _refused(K, K.ptau_unpack, packed[:7], "Invalid File format")
    # a header that is not BN254's, a power no packed file can have
    h = bytearray(PM.payload(packed, 1))
    h[4] ^= 1
    _refused(K, K.ptau_unpack, PM.with_payload(packed, 1, bytes(h)), "the prime is not the BN254 base field's")
    _refused(K, K.ptau_unpack, PM.with_payload(packed, 1, PM.payload(packed, 1)[:36] + struct.pack("<II", 28, 28)), "above 27", code=-3)
    # a device string that names no device is an argument error before the file is looked at
    with pytest.raises(K.ProverError, match=r"\(-3\).*does not name one HIP device"):
        K.ptau_unpack(packed, device="HIP:0-1")


def test_the_existing_host_readers_refuse_the_packed_form(world):
    """as they refuse any foreign magic today"""
    K = world.K
    for image in (world.packed[1], world.packed_prepared[1]):
        for call in (K.ptau_info, K.ptau_prepared_size, K.ptau_contributions):
            _refused(K, call, image, "Invalid File format (expected 'ptau')")
