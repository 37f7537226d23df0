"""The .r1cs reader through groth16_r1cs_info: container, header and the host walk over section 2's count words that bounds every
record.  Host only — these tests run where there is no GPU, which shows that the function opens none.  Every malformed file is
CONSTRUCTED: a named edit of a sound file, and must come back as a format error (-2) whose text names the cause."""
import struct

import pytest

Q_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583


def _sections(z):
    """[(id, offset of the payload, length)] of an iden3 binary container"""
    n = struct.unpack_from("<I", z, 8)[0]
    pos, out = 12, []
    for _ in range(n):
        sid, ln = struct.unpack_from("<IQ", z, pos)
        out.append((sid, pos + 12, ln))
        pos += 12 + ln
    return out


def _where(z, sid):
    return next((off, ln) for s, off, ln in _sections(z) if s == sid)


@pytest.fixture(scope="module")
def circuits(S):
    return [S.random_circuit(150, 2, 10, seed=11)[0], S.squaring_chain(70)[0]]


def _counts(r):
    return (r.n_vars, r.n_public, r.n_constraints, len(r.A) + len(r.B) + len(r.C))


def _info(K, image):
    i = K.r1cs_info(image)
    assert i.device_bytes == 0 and i.upload_ms == 0 and i.device_ms == 0
    return (i.n_wires, i.n_public, i.n_constraints, i.n_terms)


@pytest.mark.parametrize("order", [(1, 2, 3), (2, 3, 1), (3, 2, 1)])
def test_round_trip_in_every_section_order(K, S, circuits, order):
    for r in circuits:
        for n_pub_out in range(r.n_public + 1):
            assert _info(K, S.write_r1cs(r, n_pub_out=n_pub_out, section_order=order)) == _counts(r)
        # an unknown section (5: a custom-gate section) is ignored wherever it stands
        assert _info(K, S.write_r1cs(r, section_order=order, extra_sections=[(5, b"\x07" * 40)])) == _counts(r)


def test_n_pub_out_values(K, S, circuits):
    r = circuits[0]
    assert r.n_public == 2
    for n_pub_out in (0, 1, 2):
        image = S.write_r1cs(r, n_pub_out=n_pub_out)
        off, _ = _where(image, 1)
        assert struct.unpack_from("<II", image, off + 40) == (n_pub_out, 2 - n_pub_out)
        assert _info(K, image) == _counts(r)


def test_vectorised_writer_is_the_list_writer(S):
    for n in (1, 2, 3, 70):
        assert S.write_r1cs_squaring_chain(n) == S.write_r1cs(S.squaring_chain(n)[0])


def test_empty_circuit_is_legal(K, S):
    r = S.R1CS(n_vars=4, n_public=1, n_constraints=0)
    assert _info(K, S.write_r1cs(r)) == (4, 1, 0, 0)


def test_empty_rows_are_legal(K, S):
    r = S.R1CS(n_vars=4, n_public=1, n_constraints=3, A=[(1, 2, 5)], B=[], C=[(2, 3, 1), (2, 3, 1)])
    assert _info(K, S.write_r1cs(r)) == (4, 1, 3, 3)


def _malformed(S, r):
    good = S.write_r1cs(r)
    h_off, _ = _where(good, 1)
    c_off, c_len = _where(good, 2)
    cases = {}
    cases["wrong magic"] = (b"r1cx" + good[4:], "Invalid File format")
    cases["version 2"] = (good[:4] + struct.pack("<I", 2) + good[8:], "Version not supported")
    e = bytearray(good)
    struct.pack_into("<I", e, h_off, 64)
    cases["n8 = 64"] = (bytes(e), "unsupported field size 64")
    e = bytearray(good)
    e[h_off + 4:h_off + 36] = Q_MOD.to_bytes(32, "little")
    cases["the prime replaced by q"] = (bytes(e), "prime")
    cases["section 2 missing"] = (S.write_r1cs(r, section_order=(1, 3)), "Missing section 2")
    cases["section 1 twice"] = (S.write_r1cs(r, section_order=(1, 2, 3, 1)), "Section Duplicated 1")
    # (sections in the order 1, 3, 2: section 2 is the file's tail, so cutting the file cuts a record)
    tail = S.write_r1cs(r, section_order=(1, 3, 2))
    t_off, t_len = _where(tail, 2)
    assert t_off + t_len == len(tail)
    cases["file truncated inside a record"] = (tail[:len(tail) - 17], "section 2 exceeds the file")
    e = bytearray(good)
    cnt = struct.unpack_from("<I", e, c_off)[0]
    assert cnt >= 1
    struct.pack_into("<I", e, c_off, cnt + c_len)                       # the walk would leave the section at once
    cases["a count word raised: overrun"] = (bytes(e), "constraint 0, matrix A: a count of %d overruns section 2" % (cnt + c_len))
    # the LAST row's count word (every row of these circuits' C has one term): the walk is in step until there.  An edit of an
    # earlier count word can leave a file that still parses — the walk would read a count out of a value's bytes.
    last = c_off + c_len - 36 - 4
    assert struct.unpack_from("<I", good, last)[0] == 1
    e = bytearray(good)
    struct.pack_into("<I", e, last, 2)
    cases["a count word raised by one: overrun at the end"] = (bytes(e), "constraint %d, matrix C: a count of 2 overruns section 2" % (r.n_constraints - 1))
    e = bytearray(good)
    struct.pack_into("<I", e, last, 0)
    cases["a count word lowered: the walk ends early"] = (bytes(e), "section 2 has 36 bytes left behind its %d constraints" % r.n_constraints)
    e = bytearray(good)
    pos = next(12 + sum(12 + ln for _, _, ln in _sections(good)[:k]) for k, (s, _, _) in enumerate(_sections(good)) if s == 2)
    struct.pack_into("<Q", e, pos + 4, len(good))
    cases["section size claiming more than the file holds"] = (bytes(e), "section 2 exceeds the file")
    e = bytearray(good)
    struct.pack_into("<I", e, h_off + 60, 0x10000000)
    cases["a constraint count the section cannot hold"] = (bytes(e), "do not fit section 2")
    return cases


def test_constructed_malformed_files_are_format_errors(K, S, circuits):
    for r in circuits:
        for name, (image, text) in _malformed(S, r).items():
            with pytest.raises(K.ProverError) as err:
                K.r1cs_info(image)
            assert "(-2)" in str(err.value) and text in str(err.value), (name, str(err.value))


def test_null_and_short_images(K):
    for image in (b"", b"r1cs", b"r1cs" + struct.pack("<II", 1, 1)):
        with pytest.raises(K.ProverError, match=r"\(-2\)"):
            K.r1cs_info(image)
