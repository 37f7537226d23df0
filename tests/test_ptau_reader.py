"""groth16_ptau_info — the host half of groth16_zkey_verify_ptau: container, header and block bounds of a prepared .ptau.  Host
only: no test here initialises a GPU.  No file written by snarkjs exists offline; synth.write_ptau and the reader follow the one
layout include/groth16_prover.h states.  Also here: the synthesiser's additions leave every existing writer byte-identical."""
import hashlib
import struct

import pytest


@pytest.fixture(scope="module")
def fbm(O):
    gen = {g: O.ec_to_affine(g, O.ec_generator(g)) for g in ("g1", "g2")}
    return lambda g, sc: O.fixed_base_mul(g, gen[g], sc)


@pytest.fixture(scope="module")
def ptau(S, O, fbm):
    return S.write_ptau(4, fbm, points_to_mont=lambda a: O.fq_convert_montgomery(a, True))


def _sections(image):
    pos, out = 12, []
    for _ in range(struct.unpack_from("<I", image, 8)[0]):
        sid, ln = struct.unpack_from("<IQ", image, pos)
        out.append((sid, pos + 12, ln))
        pos += 12 + ln
    return out


def _without(image, drop):
    keep = [(sid, image[off:off + ln]) for sid, off, ln in _sections(image) if sid not in drop]
    return image[:8] + struct.pack("<I", len(keep)) + b"".join(struct.pack("<IQ", sid, len(p)) + p for sid, p in keep)


def _resized(image, sid_cut, new_len):
    secs = [(sid, image[off:off + ln][:new_len] if sid == sid_cut else image[off:off + ln]) for sid, off, ln in _sections(image)]
    return image[:12] + b"".join(struct.pack("<IQ", sid, len(p)) + p for sid, p in secs)


def test_info_of_a_written_ptau(K, ptau):
    info = K.ptau_info(ptau)
    assert (info.power, info.ceremony_power) == (4, 4)
    n = 16
    want = {1: 44, 2: (2 * n - 1) * 64, 3: n * 128, 4: n * 64, 5: n * 64, 6: 128, 7: 4,
            12: (4 * n - 1) * 64, 13: (2 * n - 1) * 128, 14: (2 * n - 1) * 64, 15: (2 * n - 1) * 64}
    assert {sid: b for sid, b in enumerate(info.section_bytes) if b} == want
    for k in range(5):
        assert K.ptau_info(ptau, domain_power=k).power == 4


def test_info_of_a_mapped_file(K, ptau, tmp_path):
    p = tmp_path / "pot.ptau"
    p.write_bytes(ptau)
    assert list(K.ptau_info(p).section_bytes) == list(K.ptau_info(ptau).section_bytes)


def test_point_sections_are_the_powers_and_lagrange_values(K, S, O, ptau, fbm):
    """the writer against the layout: section 4 element 0 is [α]₁, section 12's block for power 2 is [L_j(τ)]₁ of the size-4 domain"""
    tau, alpha, beta = S.toxic_waste()[:3]
    off = {sid: o for sid, o, _ in _sections(ptau)}
    mont = lambda g, xs: O.fq_convert_montgomery(fbm(g, S.ints_to_arr(xs)), True).tobytes()
    assert ptau[off[4]:off[4] + 128] == mont("g1", [alpha, alpha * tau % S.R_MOD])
    assert ptau[off[5]:off[5] + 64] == mont("g1", [beta]) and ptau[off[6]:off[6] + 128] == mont("g2", [beta])
    L = S.lagrange_at(4, 2, tau)
    assert ptau[off[12] + 3 * 64:off[12] + 7 * 64] == mont("g1", L)
    assert ptau[off[13] + 3 * 128:off[13] + 7 * 128] == mont("g2", L)
    assert ptau[off[14] + 3 * 64:off[14] + 7 * 64] == mont("g1", [alpha * x % S.R_MOD for x in L])
    assert ptau[off[15] + 3 * 64:off[15] + 7 * 64] == mont("g1", [beta * x % S.R_MOD for x in L])
    L32 = S.lagrange_at(32, 5, tau)
    assert ptau[off[12] + 31 * 64:off[12] + 63 * 64] == mont("g1", L32)      # section 12 goes on to power + 1


def test_each_malformed_file_has_its_own_message(K, ptau):
    def refused(image, code, text, **kw):
        with pytest.raises(K.ProverError, match=rf"\({code}\)") as e:
            K.ptau_info(image, **kw)
        assert text in str(e.value), str(e.value)

    refused(ptau[:len(ptau) - 100], -2, "exceeds the file")
    refused(ptau[:20], -2, "truncated section table")
    refused(b"zkey" + ptau[4:], -2, "expected 'ptau'")
    refused(ptau[:4] + struct.pack("<I", 2) + ptau[8:], -2, "Version not supported")
    hdr = next(o for sid, o, _ in _sections(ptau) if sid == 1)
    changed = bytearray(ptau)
    changed[hdr + 4] ^= 2                                          # q
    refused(bytes(changed), -2, "not the BN254 base field's")
    refused(_without(ptau, {4}), -2, "Missing section 4")
    refused(_without(ptau, {13}), -2, "Missing section 13")
    refused(_without(ptau, {12, 13, 14, 15}), -2, "has not been prepared for phase 2")
    # a block out of its section: only the blocks a verify would read are demanded
    short12 = _resized(ptau, 12, (2 * 16 - 1) * 64)              # section 12 without its block for power + 1
    assert K.ptau_info(short12).power == 4 and K.ptau_info(short12, domain_power=3).power == 4
    refused(short12, -2, "section 12 holds 1984 bytes, its block for power 5 ends at byte 4032", domain_power=4)
    refused(_resized(ptau, 14, 15 * 64), -2, "section 14 holds 960 bytes, its block for power 4", domain_power=4)
    refused(ptau, -3, "power 4 is below the key's domain 2^5", domain_power=5)


def test_existing_writers_are_byte_identical(S, O, fbm):
    """setup, write_r1cs and write_wtns write what they wrote before key_scalars / toxic= / write_ptau were added: the digests
    were taken from the previous revision of the synthesiser"""
    r, w = S.random_circuit(40, 2, 5, seed=3)
    zkey, _ = S.setup(r, fbm, points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
    assert hashlib.sha256(zkey).hexdigest() == "d04d702091177fbafb6f9e12102b23134501cbf05552abe397bc5f87743cb4a0"
    zkey2, _ = S.setup(S.squaring_chain(20)[0], fbm)
    assert hashlib.sha256(zkey2).hexdigest() == "7bd11d9bd70e9680e0242889510d5cb31f6dfeecf45f5a3f90c711da1bfafaed"
    assert hashlib.sha256(S.write_r1cs(r)).hexdigest() == "5b596429dbfe70856ccbf65636ce296b7fbcef183302fe06a68010e617b45413"
    assert hashlib.sha256(S.write_wtns(w)).hexdigest() == "5866a7af45695b06e3ee75d7092c4f292564bda3d855463fab6131ed68facbea"
    # toxic= with the default toxic waste is the default
    assert S.setup(r, fbm, points_to_mont=lambda a: O.fq_convert_montgomery(a, True), toxic=S.toxic_waste())[0] == zkey
