"""The mixed-key verifier's host part without a GPU: tests/verify_mixed_check.cpp — a stand-alone program over the product's
grouping, per-key sums and segment layout (csrc/prover/verify_host.h) and pairing29.h, compiled with -DF29_CHECK — evaluates the
mixed equation and each key's own equation for inputs written here from the discrete-log model (tests/groth16_dlog_model.py); the
expected verdicts are the model's integer arithmetic.  The same program once more under AddressSanitizer and UBSan (a plain
executable, nothing preloaded).  And groth16_vkset_new's refusals, which are decided before any device is touched."""
import ctypes as C
import hashlib
import json
import os
import random
import struct
import subprocess

import pytest

from conftest import ROOT
import groth16_dlog_model as M

R = M.R
SEEDS = [hashlib.sha256(b"mixed host %d" % k).digest() for k in range(3)]


def _build(name, extra):
    out = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-O1", "-std=c++17", "-DF29_CHECK", *extra, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "icicle-snark_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "verify_mixed_check.cpp")],
                   check=True)
    return out


@pytest.fixture(scope="module")
def exe():
    return _build("verify_mixed_check", [])


@pytest.fixture(scope="module")
def dlog(O):
    table = M.case_table()
    pts = M.Points(O)
    pts.need_items([it for _, items in table for it in items])
    pts.resolve()
    return table, pts


def _le(ints):
    return b"".join(int(x).to_bytes(32, "little") for x in ints)


def _input(pts, keys, batch, seed):
    """the program's input: `batch` = [(key index, coefficient index, Item)]"""
    out = struct.pack("<II", len(keys), len(batch)) + seed
    for key in keys:
        n = key.n_public
        out += struct.pack("<I", n) + _le(pts.g1(key.alpha)) + _le(pts.g2(key.beta)) + _le(pts.g2(key.gamma)) + _le(pts.g2(key.delta))
        out += _le([v for k in key.ic[:n + 1] for v in pts.g1(k)])
    for k, index, it in batch:
        b = M.twist_point_outside_subgroup() if it.proof.b_outside else pts.g2(it.proof.b)
        out += struct.pack("<iQ", k, index) + _le(pts.g1(it.proof.a)) + _le(b) + _le(pts.g1(it.proof.c))
        out += _le(it.signals[:keys[k].n_public])
    return out


def _run(exe, tmp_path, pts, keys, batch, seed, env=None):
    path = tmp_path / "mixed.bin"
    path.write_bytes(_input(pts, keys, batch, seed))
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, (run.returncode, run.stdout[-300:], run.stderr[-2000:])
    lines = run.stdout.split("\n")
    assert lines[0].startswith("global ") and lines[len(keys) + 1] == "bounds ok", run.stdout[-300:]
    return int(lines[0].split()[1]), [int(ln.split()[2]) for ln in lines[1:len(keys) + 1]], run.stderr


def _model(keys, batch):
    """(the whole batch, each key): 1 iff every item there has the model's verdict 1 — a pi_b outside the subgroup (−2) fails it"""
    per_key = [int(all(it.want == 1 for k, _, it in batch if k == j)) for j in range(len(keys))]
    return int(all(it.want == 1 for _, _, it in batch)), per_key


def _shuffled(rnd, picks):
    """[(key index, Item)] → a batch in random order; an item's coefficient index is its place in the batch"""
    picks = list(picks)
    rnd.shuffle(picks)
    return [(k, i, it) for i, (k, it) in enumerate(picks)]


def test_every_valid_item_of_the_table_in_one_batch(exe, dlog, tmp_path):
    table, pts = dlog
    keys = [key for key, _ in table]
    batch = _shuffled(random.Random(1), [(k, it) for k, (_, items) in enumerate(table) for it in items if it.want == 1])
    assert {"gamma=0", "delta=0", "alpha=0", "beta=0", "n=0", "n=40"} <= {keys[k].name for k, _, _ in batch}
    got = _run(exe, tmp_path, pts, keys, batch, SEEDS[0])
    assert got[:2] == (1, [1] * len(keys))


def test_keys_with_invalid_items_fail_alone(exe, dlog, tmp_path):
    """every third key brings all its items (rejected ones, a pi_b outside the subgroup), the others their valid items only: the
    batch fails, and so does exactly each key that the model says holds an item that is not accepted"""
    table, pts = dlog
    keys = [key for key, _ in table]
    picks = []
    for k, (_, items) in enumerate(table):
        picks += [(k, it) for it in items if not it.json_only and (k % 3 == 1 or it.want == 1)]
    batch = _shuffled(random.Random(2), picks)
    want = _model(keys, batch)
    assert want[0] == 0 and set(want[1]) == {0, 1} and want[1] == [int(k % 3 != 1) for k in range(len(keys))]
    assert _run(exe, tmp_path, pts, keys, batch, SEEDS[1])[:2] == want


def test_errors_that_cancel_across_two_keys(exe, O, tmp_path):
    """item 1 under key 1 with error e₁, item 2 under key 2 with e₂ = −δ₁·e₁·δ₂⁻¹: the unweighted product of the two equations is 1
    (asserted in integers), the weighted one and both keys' own equations are not; a third key's valid item is untouched"""
    rnd = random.Random(3)
    keys = [M.random_key(rnd, 2, "k1"), M.random_key(rnd, 3, "k2"), M.random_key(rnd, 1, "k3")]
    sig = [[rnd.randrange(R) for _ in range(k.n_public)] for k in keys]
    e1 = rnd.randrange(1, R)
    e2 = -keys[0].delta * e1 * pow(keys[1].delta, -1, R) % R
    items = [M.Item(keys[0], M.prove(keys[0], sig[0], rnd.randrange(1, R), rnd.randrange(1, R), e=e1), sig[0], "e1"),
             M.Item(keys[1], M.prove(keys[1], sig[1], rnd.randrange(1, R), rnd.randrange(1, R), e=e2), sig[1], "e2"),
             M.Item(keys[2], M.prove(keys[2], sig[2], rnd.randrange(1, R), rnd.randrange(1, R)), sig[2], "valid")]
    assert [it.want for it in items] == [0, 0, 1]
    assert sum(it.proof.a * it.proof.b - it.key.alpha * it.key.beta - it.key.gamma * M.cpub_dlog(it.key, it.signals) - it.key.delta * it.proof.c
               for it in items) % R == 0
    pts = M.Points(O)
    pts.need_items(items)
    pts.resolve()
    for seed in SEEDS:
        assert _run(exe, tmp_path, pts, keys, [(k, k, it) for k, it in enumerate(items)], seed)[:2] == (0, [0, 0, 1])


def _small_case(O):
    rnd = random.Random(4)
    keys = [M.random_key(rnd, 0, "n=0"), M.random_key(rnd, 2, "idle"), M.random_key(rnd, 3, "n=3"), M.random_key(rnd, 2, "gamma=0", gamma=0)]
    picks = []
    for k in (0, 2, 3):
        for t in range(3):
            sig = [rnd.randrange(R) for _ in range(keys[k].n_public)]
            picks.append((k, M.Item(keys[k], M.prove(keys[k], sig, rnd.randrange(1, R), rnd.randrange(1, R)), sig, f"valid {k}.{t}")))
    valid = picks[3][1]
    outside = M.Item(keys[2], M.Proof(valid.proof.a, valid.proof.b, valid.proof.c, b_outside=True), valid.signals, "B outside")
    pts = M.Points(O)
    pts.need_items([it for _, it in picks])
    pts.need("g1", [keys[1].alpha] + keys[1].ic)    # the key without items
    pts.need("g2", [keys[1].beta, keys[1].gamma, keys[1].delta])
    pts.resolve()
    return keys, picks, outside, pts


def test_a_key_without_items_and_a_flagged_pi_b(exe, O, tmp_path):
    keys, picks, outside, pts = _small_case(O)
    batch = [(k, 5 * i + 2, it) for i, (k, it) in enumerate(picks)]         # coefficient indices with gaps
    assert _run(exe, tmp_path, pts, keys, batch, SEEDS[2])[:2] == (1, [1, 1, 1, 1])
    batch.insert(4, (2, 1000, outside))
    assert _run(exe, tmp_path, pts, keys, batch, SEEDS[2])[:2] == (0, [1, 1, 0, 1])
    assert _run(exe, tmp_path, pts, keys, [], SEEDS[2])[:2] == (1, [1, 1, 1, 1])   # no item at all


def test_the_same_program_under_asan_and_ubsan(O, tmp_path):
    san = _build("verify_mixed_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan"])
    keys, picks, outside, pts = _small_case(O)
    batch = [(k, i, it) for i, (k, it) in enumerate(picks)] + [(2, 77, outside)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    glob, per_key, err = _run(san, tmp_path, pts, keys, batch, SEEDS[0], env=env)
    assert (glob, per_key) == (0, [1, 1, 0, 1])
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]


# ---- groth16_vkset_new: what it refuses before any device is touched -------------------------------------------------------------
def _err(K):
    return K.lib().groth16_verify_last_error().decode()


def test_vkset_new_refuses_a_malformed_key_without_a_device(K, dlog):
    table, pts = dlog
    good = [M.vk_json(pts, table[k][0]).encode() for k in (1, 2)]
    bad = [good[0][:-2], json.dumps(dict(json.loads(good[1]), nPublic="x")).encode()]
    lib = K.lib()
    h = C.c_void_p(1)
    arr = (C.c_char_p * 4)(good[0], good[1], bad[0], bad[1])
    assert lib.groth16_vkset_new(arr, 4, b"HIP", C.byref(h)) == -2
    assert _err(K).startswith("key 2: ") and "malformed JSON" in _err(K) and h.value is None
    arr = (C.c_char_p * 4)(bad[1], good[1], bad[0], good[0])
    assert lib.groth16_vkset_new(arr, 4, b"HIP", C.byref(h)) == -2
    assert _err(K).startswith("key 0: ") and "nPublic" in _err(K)
    with pytest.raises(K.ProverError, match="key 1: "):
        K.VkSet([good[0].decode(), bad[0].decode()])
    # a point of the key outside its group: the host subgroup test of parse_vk
    x0, x1, y0, y1 = M.twist_point_outside_subgroup()
    vk = json.loads(good[0])
    vk["vk_gamma_2"] = [[str(x0), str(x1)], [str(y0), str(y1)], ["1", "0"]]
    with pytest.raises(K.ProverError, match="key 0: "):
        K.VkSet([json.dumps(vk)])


def test_vkset_null_arguments(K, dlog):
    table, pts = dlog
    good = M.vk_json(pts, table[1][0]).encode()
    lib = K.lib()
    h = C.c_void_p()
    arr = (C.c_char_p * 2)(good, None)
    assert lib.groth16_vkset_new(None, 1, b"HIP", C.byref(h)) == -3
    assert lib.groth16_vkset_new(arr, 2, b"HIP", C.byref(h)) == -3          # a null entry
    assert lib.groth16_vkset_new(arr, 1, None, C.byref(h)) == -3
    assert lib.groth16_vkset_new(arr, 1, b"HIP", None) == -3
    assert "null argument" in _err(K)
    assert lib.groth16_vkset_info(None, -1, None) == -3
    assert lib.groth16_verify_batch_mixed(None, None, None, None, 1, None, None, None) == -3
    lib.groth16_vkset_free(None)
    bad = (C.c_char_p * 1)(good[:-2])
    assert lib.groth16_vkset_new(bad, 1, b"HIP:0-1", C.byref(h)) != 0 and "one device" in _err(K)
