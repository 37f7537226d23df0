"""The host half of the packed witness: groth16_wtns_packed_size / _pack / _unpack_host, the container reader (wtnz_layout) and the
host decoder against tests/wtns_pack_model.py's Python integers, byte for byte in both directions.  Every case is CONSTRUCTED, and
every refusal here is decided before any device call: none of these tests initialises a GPU.  tests/wtns_pack_check.cpp, a
stand-alone program of the same host code whose HOST side alone is built under AddressSanitizer and UBSan, runs over a byte-mutation
corpus."""
import os
import random
import struct
import subprocess

import pytest

import wtns_pack_model as M
from conftest import ROOT

R = M.R_MOD
EDGES = M.edge_values()


def mixed(n, seed=1):
    """n values: three quarters bits, the rest edges, small values, negated small values and full-width ones"""
    rng = random.Random(seed)
    pool = EDGES + [rng.randrange(R) for _ in range(8)] + [rng.randrange(1 << 64) for _ in range(4)] + [R - rng.randrange(1, 1 << 40) for _ in range(4)]
    return [rng.randrange(2) if rng.random() < 0.75 else rng.choice(pool) for _ in range(n)]


def test_the_models_encoding_is_what_the_format_says():
    """conditions on the model's own output, before anything is compared with it"""
    assert M.encode(0) == (0x00, b"") and M.encode(1) == (0x40, b"") and M.encode(2) == (0x01, b"\x02")
    assert M.encode(255) == (0x01, b"\xff") and M.encode(256) == (0x02, b"\x00\x01")
    assert M.encode(R - 1) == (0x81, b"\x01") and M.encode(R - 2) == (0x81, b"\x02") and M.encode(R - 255) == (0x81, b"\xff") and M.encode(R - 256) == (0x82, b"\x00\x01")
    assert M.encode((1 << 248) - 1) == (0x1f, b"\xff" * 31) and M.encode(1 << 248) == (0x20, b"\x00" * 31 + b"\x01")
    assert M.encode(R - (1 << 248) + 1) == (0x9f, b"\xff" * 31)                       # the longest negated form
    assert M.encode(R - (1 << 248))[0] == 0x20 and M.encode(R - (1 << 248) - 1)[0] == 0x20 and M.encode((R - 1) // 2)[0] == 0x20 and M.encode((R + 1) // 2)[0] == 0x20
    for v in EDGES + mixed(200):
        c, p = M.encode(v)
        assert len(p) == M.code_len(c) and M.decode(c, p) == (v, 0)
    # what the rules buy: a bit wire 1 byte, a full-width value 33, three quarters bits about 9 bytes a value
    n = 1 << 12
    rng = random.Random(5)
    quarter = [rng.randrange(2) if i % 4 else rng.randrange(1 << 248, R - (1 << 248)) for i in range(n)]
    assert M.packed_size([1] * n) - M.packed_size([]) == n + 8 * (n // 256)
    assert M.packed_size([R // 3] * n) - M.packed_size([]) == 33 * n + 8 * (n // 256)
    assert 9.0 <= (M.packed_size(quarter) - M.packed_size([])) / n <= 9.1


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_pack_and_unpack_byte_for_byte(K, n):
    values = (EDGES * (n // len(EDGES) + 1))[:n] if n <= 257 else mixed(n)
    wtns, want = M.write_wtns(values), M.pack(values)
    assert K.wtns_packed_size(wtns) == len(want) == M.packed_size(values)
    packed, rep = K.wtns_pack(wtns)
    assert packed == want and (rep.n_witness, rep.in_bytes, rep.out_bytes) == (n, len(wtns), len(want))
    back, rep = K.wtns_unpack(want)
    assert back == wtns and (rep.n_witness, rep.in_bytes, rep.out_bytes) == (n, len(want), len(wtns))
    assert M.unpack(want) == (values, [])


def test_every_edge_value_alone_and_the_sections_in_any_order(K):
    for v in EDGES:
        assert K.wtns_pack(M.write_wtns([v]))[0] == M.pack([v])
    values = mixed(300, seed=3)
    codes, directory, payload = M.pack_parts(values)
    for order in ((4, 3, 2, 1), (2, 4, 1, 3)):
        assert K.wtns_unpack(M.container(300, codes, directory, payload, order=order))[0] == M.write_wtns(values)


def test_file_entries(K, tmp_path):
    values = mixed(700, seed=4)
    w, z, back = tmp_path / "w.wtns", tmp_path / "w.wtnz", tmp_path / "back.wtns"
    w.write_bytes(M.write_wtns(values))
    assert K.wtns_pack(str(w), out=str(z))[0] is None and z.read_bytes() == M.pack(values)
    assert K.wtns_unpack(str(z), out=str(back))[0] is None and back.read_bytes() == w.read_bytes()
    with pytest.raises(K.ProverError, match="the output path is the input's"):
        K.wtns_pack(str(w), out=str(w))
    # a failed call leaves nothing
    bad = tmp_path / "bad.wtnz"
    bad.write_bytes(M.container(1, b"\x41", [0, 0], b""))
    with pytest.raises(K.WitnessFault):
        K.wtns_unpack(str(bad), out=str(tmp_path / "never.wtns"))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["back.wtns", "bad.wtnz", "w.wtns", "w.wtnz"]


def test_a_hard_link_of_the_input_is_refused_and_no_refusal_leaves_a_temporary(K, tmp_path):
    """the shared _file entry: the same file under two names, and the temporary of a call that fails behind its sink"""
    w, link, bad = tmp_path / "w.wtns", tmp_path / "link.wtns", tmp_path / "bad.wtnz"
    w.write_bytes(M.write_wtns(mixed(300, seed=6)))
    os.link(w, link)
    before = w.read_bytes()
    with pytest.raises(K.ProverError, match="the output path is the input's"):
        K.wtns_pack(str(w), out=str(link))
    assert w.read_bytes() == before and link.read_bytes() == before
    assert not list(tmp_path.glob("*.tmp.*"))
    bad.write_bytes(M.container(1, b"\x41", [0, 0], b""))  # an undefined code: the fault is found after the output was sized
    with pytest.raises(K.WitnessFault):
        K.wtns_unpack(str(bad), out=str(tmp_path / "never.wtns"))
    assert not list(tmp_path.glob("*.tmp.*"))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["bad.wtnz", "link.wtns", "w.wtns"]


def with_faults(values, faults):
    """the packed parts of `values` with element e's (code, payload) replaced: faults = {e: (code, payload)}"""
    codes, payload, directory = bytearray(), bytearray(), []
    for i, v in enumerate(values):
        if i % M.BLOCK == 0:
            directory.append(len(payload))
        c, p = faults.get(i, None) or M.encode(v)
        codes.append(c)
        payload += p
    directory.append(len(payload))
    return M.container(len(values), bytes(codes), directory, bytes(payload))


FAULTS = {
    "CODE": [(0x21, b""), (0xa0, b"")],
    "CODE-2": [(0x41, b""), (0x80, b"")],
    "NONCANONICAL-top-byte": [(0x02, b"\x05\x00"), (0x83, b"\x01\x02\x00")],
    "NONCANONICAL-one": [(0x01, b"\x01"), (0x01, b"\x01")],
    "NONCANONICAL-negation-shorter": [(0x20, (R - 1).to_bytes(32, "little")), (0x20, (R - (1 << 248) + 1).to_bytes(32, "little"))],
    "RANGE": [(0x20, R.to_bytes(32, "little")), (0x20, b"\xff" * 32)],
}


@pytest.mark.parametrize("name", sorted(FAULTS))
def test_each_fault_kind_twice_names_the_lower_and_counts_both(K, name):
    kind = getattr(M, name.split("-")[0])
    values = mixed(600, seed=7)
    lo, hi = 259, 517                                                        # two blocks, neither a block's first element
    image = with_faults(values, {lo: FAULTS[name][0], hi: FAULTS[name][1]})
    assert M.unpack(image)[1] == [(lo, kind), (hi, kind)]
    with pytest.raises(K.WitnessFault, match=f"wtnz: element {lo}: {M.KIND_TEXT[kind]}") as e:
        K.wtns_unpack(image)
    rep = e.value.report
    assert (rep.fault_kind, rep.fault_index, rep.fault_count) == (kind, lo, 2) and K.WTNZ_KINDS[kind] == name.split("-")[0]


def test_directory_fault_is_named_at_the_blocks_first_element(K):
    values = mixed(800, seed=8)
    codes, directory, payload = M.pack_parts(values)
    assert len(directory) == 5 and directory[1] > 0 and directory[2] > directory[1]
    moved = list(directory)
    moved[2] -= 1                                                            # still monotone, still ends at section 4's size: host-valid
    image = M.container(800, codes, moved, payload)
    assert M.unpack(image)[1] == [(256, M.DIRECTORY), (512, M.DIRECTORY)]
    with pytest.raises(K.WitnessFault, match="wtnz: element 256: the block's lengths do not sum to its directory span") as e:
        K.wtns_unpack(image)
    assert (e.value.report.fault_kind, e.value.report.fault_index, e.value.report.fault_count) == (M.DIRECTORY, 256, 2)
    # an undefined code counts 0 bytes: the block's sum still holds and the fault is the code's
    image = with_faults(values, {300: (0x7f, b"")})
    with pytest.raises(K.WitnessFault, match="wtnz: element 300: an undefined code byte"):
        K.wtns_unpack(image)


def test_container_refusals(K):
    values = mixed(300, seed=9)
    codes, directory, payload = M.pack_parts(values)
    good = M.container(300, codes, directory, payload)
    assert K.wtns_unpack(good)[0] == M.write_wtns(values)

    def refused(image, text):
        with pytest.raises(K.ProverError, match=text) as e:
            K.wtns_unpack(image)
        assert "(-2)" in str(e.value) and not isinstance(e.value, K.WitnessFault)

    refused(b"wtnx" + good[4:], r"Invalid File format \(expected 'wtnz'\)")
    refused(good[:8], "Invalid File format")
    refused(good[:12 + 12 + 40 + 5], "truncated section table")
    refused(good[:4] + struct.pack("<I", 2) + good[8:], "Version not supported")
    refused(M.sections(b"wtnz", [(1, M.wtns_header(300)), (2, codes), (3, b"")]), "Missing section 4")
    refused(M.sections(b"wtnz", [(1, M.wtns_header(300)), (2, codes), (2, codes), (3, b""), (4, payload)]), "Section Duplicated 2")
    refused(M.sections(b"wtnz", [(1, M.wtns_header(300)[:-1]), (2, codes), (3, b""), (4, payload)]), "wtnz: unsupported field size")
    refused(M.container(300, codes[:-1], directory, payload), "wtnz: section 2 holds 299 bytes, 300 values have 300 codes")
    refused(M.container(300, codes, directory + [directory[-1]], payload), "wtnz: section 3 holds 32 bytes, the directory of 300 values has 24")
    refused(M.container(300, codes, [1] + directory[1:], payload), "wtnz: directory entry 0 is 1, not 0")
    refused(M.container(300, codes, [0, directory[2] + 1, directory[2]], payload), "wtnz: directory entry 2 is below entry 1")
    refused(M.container(300, codes, directory[:-1] + [directory[-1] + 1], payload), f"wtnz: the directory ends at {directory[-1] + 1}, section 4 holds {directory[-1]} bytes")
    refused(M.container(300, codes, directory, payload + b"\0"), f"wtnz: the directory ends at {directory[-1]}, section 4 holds {directory[-1] + 1} bytes")
    refused(M.container(300, codes, [0, 8193, 8193], b"\0" * 8193), "wtnz: block 0 spans 8193 bytes, 8192 is the most")
    refused(M.container(300, codes, directory, payload, q=R + 2), "wtnz: the prime is not the BN254 scalar field's")
    # a full block of 8192 bytes is the most there is, and valid
    full = [R // 3] * 256
    assert K.wtns_unpack(M.pack(full))[0] == M.write_wtns(full) and M.pack_parts(full)[1] == [0, 8192]


def test_wtns_readers_refuse_wtnz_and_the_reverse(K):
    values = mixed(40, seed=10)
    wtns, wtnz = M.write_wtns(values), M.pack(values)
    with pytest.raises(K.ProverError, match=r"Invalid File format \(expected 'wtns'\)"):
        K.wtns_pack(wtnz)
    with pytest.raises(K.ProverError, match=r"Invalid File format \(expected 'wtns'\)"):
        K.wtns_packed_size(wtnz)
    with pytest.raises(K.ProverError, match=r"Invalid File format \(expected 'wtnz'\)"):
        K.wtns_unpack(wtns)
    # (every .wtns reader of the library is parse_wtns, which wtns_pack has just gone through; the prove and the witness check
    # refusing a packed witness, and their packed entries refusing a .wtns, are tests/test_gpu_wtns_pack.py's: they need a key)


def test_pack_refuses_a_value_not_below_r(K):
    values = mixed(600, seed=11)
    values[300], values[555] = R, (1 << 256) - 1
    with pytest.raises(K.WitnessFault, match="wtns: element 300 is not below r") as e:
        K.wtns_pack(M.write_wtns(values))
    assert (e.value.report.fault_kind, e.value.report.fault_index, e.value.report.fault_count) == (M.RANGE, 300, 2)
    with pytest.raises(K.ProverError, match="wtns: element 300 is not below r"):
        K.wtns_packed_size(M.write_wtns(values))
    with pytest.raises(K.ProverError, match="wtns: the prime is not the BN254 scalar field's"):
        K.wtns_pack(M.write_wtns([1, 2], q=R + 2))
    # the buffer entry tests its room before anything is written
    import ctypes as C
    wtns, rep, buf = M.write_wtns([5, 6]), K.WtnsPackReport(), C.create_string_buffer(b"\xaa" * 64, 64)
    assert K.lib().groth16_wtns_pack(wtns, C.c_size_t(len(wtns)), buf, C.c_size_t(64), C.byref(rep)) == -3 and rep.out_bytes == len(M.pack([5, 6])) and buf.raw == b"\xaa" * 64


def test_the_sanitized_host_program_over_a_mutation_corpus(tmp_path):
    """tests/wtns_pack_check.cpp: the host reader and decoder, stand-alone, under AddressSanitizer and UBSan.  It mutates small valid
    containers byte by byte; whatever the reader lets through must decode inside its buffers.  The program prints what it ran."""
    exe = os.path.join(ROOT, "build", "wtns_pack_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    csrc = os.path.join(ROOT, "icicle-snark_amd", "csrc")
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "--offload-host-only", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + csrc, "-x", "hip", os.path.join(ROOT, "tests", "wtns_pack_check.cpp"), os.path.join(csrc, "prover", "containers.cpp"), "-o", exe], check=True)
    seeds = []
    for k, values in enumerate(([], [0], EDGES, mixed(257, seed=12), [R // 3] * 256 + [1])):
        p = tmp_path / f"seed{k}.wtnz"
        p.write_bytes(M.pack(values))
        seeds.append(str(p))
    run = subprocess.run([exe] + seeds, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "accepted" in run.stdout and "refused" in run.stdout
