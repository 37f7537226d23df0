"""groth16_zkey_new_size — the size of the key groth16_zkey_new writes and its section-4 record count, from the .r1cs alone —
against the synthesiser: len(setup(...)) and the record count of setup()'s own section 4, for the circuits of the GPU tests.  Host
only: runs where there is no GPU, which shows that the function opens none."""
import struct

import pytest

import zkey_new_circuits as ZC
from test_r1cs_reader import _malformed


@pytest.fixture(scope="module")
def keys(S, O):
    G = {g: O.ec_to_affine(g, O.ec_generator(g)) for g in ("g1", "g2")}
    fbm = lambda g, sc: O.fixed_base_mul(g, G[g], sc)
    to_mont = lambda a: O.fq_convert_montgomery(a, True)
    return {name: (r, S.setup(r, fbm, points_to_mont=to_mont)[0]) for name, r in ZC.circuits(S).items()}


def test_the_circuits_have_the_shapes_the_cases_need(S, keys):
    """conditions on the inputs, checked against the synthesiser — not measurements"""
    shape = lambda r: (r.n_vars, r.n_public, r.n_constraints, S.key_scalars(r)["n"])
    assert shape(keys["mixed"][0]) == (166, 2, 158, 256)
    assert shape(keys["fan"][0]) == (303, 1, 300, 512)
    assert shape(keys["chain6"][0]) == (8, 1, 6, 8) and 6 + 1 + 1 == 8          # the binding rows are the domain's last rows
    assert shape(keys["chain7"][0]) == (9, 1, 7, 16)
    assert shape(keys["tiny"][0]) == (3, 2, 2, 8)
    r, w = ZC.mixed(S)
    assert ZC.check_r1cs(r, w)
    count = lambda mat, wire: [t[2] for t in mat if t[1] == wire]
    assert count(r.A, 163) == [1, 1] and not count(r.B, 163) and not count(r.C, 163)
    for mat in (r.A, r.B, r.C):
        a, b = count(mat, 164)
        assert (a + b) % ZC.R == 0 and a and b
        assert not count(mat, 165)
        assert {t[2] for t in mat} >= set(ZC.CLASSES)                              # every coefficient class, zero included
    assert sum(1 for t in r.A if t[0] == 151) == 40 and [t[1] for t in r.A if t[0] == 152] == [5, 5]
    assert not [t for m in (r.A, r.B, r.C) for t in m if t[0] == 150]             # the empty row
    f = keys["fan"][0]
    for mat in (f.A, f.B, f.C):
        assert len(count(mat, 0)) == 300 and len(count(mat, 2)) == 300 and len(set(count(mat, 2))) > 2


@pytest.mark.parametrize("name", ["mixed", "fan", "chain6", "chain7", "tiny"])
def test_size_and_record_count_are_the_synthesisers(K, S, keys, name):
    r, zkey = keys[name]
    secs, order = ZC.sections(zkey)
    assert order == list(range(1, 11))                                            # synth's layout is the stated one
    assert ZC.payload(zkey, 10) == struct.pack("<I", 0) and ZC.payload(zkey, 1) == struct.pack("<I", 1)
    n_records = len(ZC.records(zkey))
    assert n_records == len(r.A) + len(r.B) + r.n_public + 1
    assert sorted(ZC.records(zkey)) == sorted(ZC.stated_records(r))
    assert secs[8][1] == 64 * (r.n_vars - r.n_public - 1) and (name != "tiny" or secs[8][1] == 0)
    for order_ in ((1, 2, 3), (3, 2, 1)):
        assert K.zkey_new_size(S.write_r1cs(r, section_order=order_)) == (len(zkey), n_records)


def test_an_empty_circuit(K, S):
    r = S.R1CS(n_vars=4, n_public=1, n_constraints=0)
    size, n = K.zkey_new_size(S.write_r1cs(r))
    assert n == 2 and size == 12 + 10 * 12 + 4 + 660 + 64 * 2 + (4 + 44 * 2) + 64 * 4 * 2 + 128 * 4 + 64 * 2 + 64 * 2 + 4


def test_malformed_r1cs_gives_the_readers_codes(K, S):
    for r in (S.random_circuit(150, 2, 10, seed=11)[0], S.squaring_chain(70)[0]):
        for name, (image, text) in _malformed(S, r).items():
            with pytest.raises(K.ProverError) as err:
                K.zkey_new_size(image)
            assert "(-2)" in str(err.value) and text in str(err.value), (name, str(err.value))
    for image in (b"", b"r1cs", b"r1cs" + struct.pack("<II", 1, 1)):
        with pytest.raises(K.ProverError, match=r"\(-2\)"):
            K.zkey_new_size(image)
