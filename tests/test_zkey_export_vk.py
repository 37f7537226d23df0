"""groth16_zkey_export_vk: the verification key of a .zkey as snarkjs' verification_key.json text, against the golden key's
fixture, the library's own verifier and the synthesiser's vk.  Host only — these tests run where there is no GPU, which shows
that the function opens none."""
import base64
import json
import struct

import pytest

from conftest import load_golden, unhex


def _sections(z):
    """[(id, offset of the payload, length)] of a snarkjs binary container"""
    n = struct.unpack_from("<I", z, 8)[0]
    pos, out = 12, []
    for _ in range(n):
        sid, ln = struct.unpack_from("<IQ", z, pos)
        out.append((sid, pos + 12, ln))
        pos += 12 + ln
    return out


@pytest.fixture(scope="module")
def golden():
    g = load_golden("groth16.json")
    return g, base64.b64decode(g["zkey"])


def test_golden_key_exports_the_fixture_vk(K, S, golden):
    g, zkey = golden
    v = g["vk"]
    vk = dict(vk_alpha_1=unhex(v["vk_alpha_1"], 2, 4), vk_beta_2=unhex(v["vk_beta_2"], 4, 4), vk_gamma_2=unhex(v["vk_gamma_2"], 4, 4),
              vk_delta_2=unhex(v["vk_delta_2"], 4, 4), IC=[unhex(p, 2, 4) for p in v["IC"]], n_public=len(v["IC"]) - 1)
    want = json.loads(S.vk_to_json(vk))
    got = json.loads(K.zkey_export_vk(zkey))
    assert sorted(got) == sorted(want)
    for field in want:
        assert got[field] == want[field], field
    assert got["protocol"] == "groth16" and got["curve"] == "bn128" and got["nPublic"] == 1


def test_golden_proofs_verify_with_the_exported_vk(K, golden):
    g, zkey = golden
    text = K.zkey_export_vk(zkey)
    for c in g["cases"]:
        assert K.groth16_verify_json(json.dumps(c["proof"]), json.dumps(c["public"]), text) is True
        bad = [str(int(c["public"][0]) + 1)] + c["public"][1:]
        assert K.groth16_verify_json(json.dumps(c["proof"]), json.dumps(bad), text) is False


@pytest.mark.parametrize("n_public", [0, 3])
def test_synthesised_key_exports_the_synthesisers_vk(K, S, O, n_public):
    G = {g: O.ec_to_affine(g, O.ec_generator(g)) for g in ("g1", "g2")}
    r1, _ = S.random_circuit(12, n_public, 4)
    zkey, vk = S.setup(r1, lambda g, sc: O.fixed_base_mul(g, G[g], sc), points_to_mont=lambda a: O.fq_convert_montgomery(a, True))
    got = json.loads(K.zkey_export_vk(zkey))
    assert got == json.loads(S.vk_to_json(vk))
    assert got["nPublic"] == n_public and len(got["IC"]) == n_public + 1


def test_export_reports_malformed_keys_and_small_buffers(K, golden):
    import ctypes as C
    _, zkey = golden
    f = K.lib().groth16_zkey_export_vk
    f.restype = C.c_int64
    call = lambda z, out, cap: f(C.c_char_p(bytes(z)), C.c_size_t(len(z)), out, C.c_size_t(cap))
    text = K.zkey_export_vk(zkey)
    need = len(text.encode()) + 1
    # a buffer too small: the needed length comes back and the buffer is left alone
    assert call(zkey, None, 0) == need
    small = C.create_string_buffer(b"\x55" * 16, 16)
    assert call(zkey, small, 16) == need and small.raw == b"\x55" * 16
    exact = C.create_string_buffer(need)
    assert call(zkey, exact, need) == need and exact.value.decode() == text
    # a truncated file: the container reader's format error
    assert call(zkey[:len(zkey) // 2], None, 0) == -2
    with pytest.raises(K.ProverError, match="exceeds the file|truncated"):
        K.zkey_export_vk(zkey[:len(zkey) // 2])
    assert call(zkey[:8], None, 0) == -2
    # a file without section 3: rebuilt from the other sections
    secs = _sections(zkey)
    kept = [(sid, off, ln) for sid, off, ln in secs if sid != 3]
    assert len(kept) == len(secs) - 1
    no_ic = zkey[:8] + struct.pack("<I", len(kept)) + b"".join(struct.pack("<IQ", sid, ln) + zkey[off:off + ln] for sid, off, ln in kept)
    assert call(no_ic, None, 0) == -2
    with pytest.raises(K.ProverError, match="Missing section 3"):
        K.zkey_export_vk(no_ic)
