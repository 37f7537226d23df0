"""The inputs behind tests/golden/zkey_load_messages.json: the small key of tests/golden/groth16.json with one section missing or
duplicated, a header field or a section length off, and keys with two such faults, which pin the fault that is reported first.
Test infrastructure (tests/test_zkey_load_messages.py replays it).

    python tests/zkey_corpus.py --record      writes the fixture from the library of the tree this file lies in

The fixture pins (return value, groth16_last_error() text) of groth16_cache_load for every case of build(), and of
groth16_zkey_export_vk for the cases of build_ic() — faults of section 3, which only the key check and the vk export read.  Every
case fails the container and header checks, which run before a device is touched: the record needs no GPU.  Names, codes and texts
only are stored; a key is stored by its SHA-256, so a drift of this builder shows as a hash mismatch."""
import base64
import ctypes as C
import hashlib
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "zkey_load_messages.json")
LOADER_SECTIONS = (1, 2, 4, 5, 6, 7, 8, 9)
POINT_BYTES = {3: 64, 5: 64, 6: 64, 7: 128, 8: 64, 9: 64}
# section 2: n8q u32, q[32], n8r u32, r[32], n_vars u32, n_public u32, domain u32, then the six points
OFF_N8Q, OFF_Q, OFF_N8R, OFF_R, OFF_N_VARS, OFF_N_PUBLIC, OFF_DOMAIN = 0, 4, 36, 40, 72, 76, 80


def golden_zkey():
    with open(os.path.join(HERE, "golden", "groth16.json")) as f:
        return base64.b64decode(json.load(f)["zkey"])


def sections(z):
    """[(id, payload)] of a snarkjs binary container, in file order"""
    n = struct.unpack_from("<I", z, 8)[0]
    pos, out = 12, []
    for _ in range(n):
        sid, ln = struct.unpack_from("<IQ", z, pos)
        out.append((sid, bytes(z[pos + 12:pos + 12 + ln])))
        pos += 12 + ln
    return out


def container(secs, head=b"zkey\x01\x00\x00\x00"):
    return head + struct.pack("<I", len(secs)) + b"".join(struct.pack("<IQ", sid, len(p)) + p for sid, p in secs)


def without(secs, sid):
    return [s for s in secs if s[0] != sid]


def doubled(secs, sid):
    return secs + [s for s in secs if s[0] == sid]


def resized(secs, sid, delta):
    """the payload of section `sid` `delta` bytes longer (zeros) or shorter"""
    return [(i, p + b"\0" * delta if delta > 0 else p[:len(p) + delta]) if i == sid else (i, p) for i, p in secs]


def header(secs, off, data):
    return [(i, p[:off] + data + p[off + len(data):]) if i == 2 else (i, p) for i, p in secs]


def u32(v):
    return struct.pack("<I", v)


def build(zkey=None):
    """[(name, key bytes)]: every case is rejected by the loader's container and header checks"""
    secs = sections(zkey if zkey is not None else golden_zkey())
    hdr = dict(secs)[2]
    n_vars = struct.unpack_from("<I", hdr, OFF_N_VARS)[0]
    out = []

    def case(name, s):
        out.append((name, container(s)))

    for sid in LOADER_SECTIONS:
        case(f"section {sid} missing", without(secs, sid))
    for sid in LOADER_SECTIONS:
        case(f"section {sid} duplicated", doubled(secs, sid))
    case("protocol 2", [(i, u32(2)) if i == 1 else (i, p) for i, p in secs])
    case("header one byte short", resized(secs, 2, -1))
    case("n8q 31", header(secs, OFF_N8Q, u32(31)))
    case("n8r 31", header(secs, OFF_N8R, u32(31)))
    case("wrong q", header(secs, OFF_Q, bytes([hdr[OFF_Q] ^ 1])))
    case("wrong r", header(secs, OFF_R, bytes([hdr[OFF_R] ^ 1])))
    case("domain 0", header(secs, OFF_DOMAIN, u32(0)))
    case("domain 6", header(secs, OFF_DOMAIN, u32(6)))
    case("n_public = n_vars", header(secs, OFF_N_PUBLIC, u32(n_vars)))
    case("coefficient section of 3 bytes", [(i, p[:3]) if i == 4 else (i, p) for i, p in secs])
    case("coefficient section one byte short", resized(secs, 4, -1))
    case("coefficient section one byte long", resized(secs, 4, +1))
    for sid in (5, 6, 7, 8, 9):
        case(f"section {sid} one point short", resized(secs, sid, -POINT_BYTES[sid]))
        case(f"section {sid} one point long", resized(secs, sid, +POINT_BYTES[sid]))
    # two faults: the one reported first
    case("section 5 missing and n8q 31", header(without(secs, 5), OFF_N8Q, u32(31)))
    case("section 9 duplicated and domain 6", header(doubled(secs, 9), OFF_DOMAIN, u32(6)))
    case("wrong q and section 7 one point short", header(resized(secs, 7, -128), OFF_Q, bytes([hdr[OFF_Q] ^ 1])))
    assert len({n for n, _ in out}) == len(out)
    return out


def build_ic(zkey=None):
    """[(name, key bytes)]: faults of section 3, which the loader does not read — groth16_zkey_export_vk reports them"""
    secs = sections(zkey if zkey is not None else golden_zkey())
    return [("section 3 missing", container(without(secs, 3))), ("section 3 duplicated", container(doubled(secs, 3))),
            ("section 3 one point short", container(resized(secs, 3, -64)))]


def accepted_variants(zkey=None):
    """[(name, key bytes)]: keys the parser must keep accepting (and the prover must keep proving with)"""
    secs = sections(zkey if zkey is not None else golden_zkey())
    coef = dict(secs)[4]
    declared = struct.unpack_from("<I", coef, 0)[0]
    return [("section 3 removed", container(without(secs, 3))),
            ("unknown sections 12 and 40 appended", container(secs + [(12, b"\x07" * 5), (40, b"\x09" * 3)])),
            ("declared coefficient count wrong", container([(i, u32(declared + 3) + p[4:]) if i == 4 else (i, p) for i, p in secs]))]


def sha(z):
    return hashlib.sha256(z).hexdigest()


def last_error(lib):
    lib.groth16_last_error.restype = C.c_char_p
    return (lib.groth16_last_error() or b"").decode()


def _manager(lib):
    lib.groth16_cache_manager_new.restype = C.c_void_p
    return C.c_void_p(lib.groth16_cache_manager_new())


def run_load(lib, z):
    """[return value, message] of groth16_cache_load on a manager of its own"""
    cm = _manager(lib)
    try:
        rc = lib.groth16_cache_load(cm, b"corpus", C.c_char_p(z), C.c_size_t(len(z)), 0, 0, 1)
        return [rc, last_error(lib) if rc else ""]
    finally:
        lib.groth16_cache_manager_free(cm)


def run_load_file(lib, path):
    cm = _manager(lib)
    try:
        rc = lib.groth16_cache_load_file(cm, b"corpus", os.fsencode(path), 0, 0, 1)
        return [rc, last_error(lib) if rc else ""]
    finally:
        lib.groth16_cache_manager_free(cm)


def run_prove(lib, zkey_path, wtns_path, out_dir, device=b"HIP"):
    """groth16_prove from files: a key that is not cached takes the cold route"""
    cm = _manager(lib)
    try:
        rc = lib.groth16_prove(os.fsencode(wtns_path), os.fsencode(zkey_path), os.fsencode(os.path.join(out_dir, "proof.json")),
                               os.fsencode(os.path.join(out_dir, "public.json")), device, cm)
        return [rc, last_error(lib) if rc else ""]
    finally:
        lib.groth16_cache_manager_free(cm)


def run_export_vk(lib, z):
    f = lib.groth16_zkey_export_vk
    f.restype = C.c_int64
    rc = int(f(C.c_char_p(z), C.c_size_t(len(z)), None, C.c_size_t(0)))
    return [rc, last_error(lib)] if rc < 0 else [0, ""]


def record():
    import importlib
    sys.path.insert(0, os.path.dirname(HERE))
    K = importlib.import_module("icicle-snark_amd")
    load = {name: dict(zip(("rc", "message"), run_load(K.lib(), z)), sha256=sha(z)) for name, z in build()}
    export = {name: dict(zip(("rc", "message"), run_export_vk(K.lib(), z)), sha256=sha(z)) for name, z in build_ic()}
    doc = {"about": "(return value, groth16_last_error() text) per case of tests/zkey_corpus.py, recorded from the library as it was while "
                    "build_cache (cache.cpp) still carried its own copy of the container and header checks beside zkey_layout "
                    "(containers.cpp).  `load`: groth16_cache_load on the cases of build(); `export_vk`: groth16_zkey_export_vk on the cases "
                    "of build_ic().",
           "load": load, "export_vk": export}
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, indent=1, ensure_ascii=True)
        f.write("\n")
    print(f"{len(load)} + {len(export)} cases -> {FIXTURE}")


if __name__ == "__main__":
    if "--record" in sys.argv:
        record()
