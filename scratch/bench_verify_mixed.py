"""Sweep of K.VkSet.verify (groth16_verify_batch_mixed) against the only thing a user could do before it: one
groth16_verify_batch_combined call per key, in the same process on the same inputs, variants interleaved.

    python scratch/bench_verify_mixed.py [--n 4096] [--keys 1,8,64,512] [--runs 5] [--out profiles/verify_mixed_sweep.txt]
    python scratch/bench_verify_mixed.py --trace-keys 64     (one warm-up and one timed call, all valid and one bad tenant: for a kernel trace)

Keys and proofs come from the discrete-log model (tests/groth16_dlog_model.py): 512 random keys with two public signals, eight
distinct valid proofs each, tiled to n/K items per key and shuffled into one batch.  Per K: wall time from the JSON texts to the
verdicts through the Python binding, the call's own parse and after-parse times, and the loop's wall time.  Then the segmented
sum alone on resident operands of the mixed call's shape (3·K segments) for three cuts, the pairing product over 3·K resident
pairs (an upper bound of the tail's Miller launch: it adds the product passes and one final exponentiation), groth16_vkset_new
per key, and one bad tenant at K = 64 against the per-item stage for every key."""
import argparse
import ctypes as C
import importlib
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--keys", default="1,8,64,512")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-keys", type=int, default=0)
    a = ap.parse_args()
    K = importlib.import_module("icicle-snark_amd")
    import groth16_dlog_model as M
    import oracle as O
    K.set_device("HIP", 0)
    ks = [int(x) for x in a.keys.split(",")] if not a.trace_keys else [a.trace_keys]
    kmax, per = max(ks + [64]), 8
    rnd = random.Random(2024)
    keys = [M.random_key(rnd, 2, f"k{k}") for k in range(kmax)]
    items = [[M.Item(key, M.prove(key, sig, M._rand(rnd), M._rand(rnd)), sig, "valid") for sig in ([M._rand(rnd), M._rand(rnd)] for _ in range(per))]
             for key in keys]
    bad = M.Item(keys[3], M.prove(keys[3], items[3][0].signals, M._rand(rnd), M._rand(rnd), e=1), items[3][0].signals, "e=1")
    pts = M.Points(O)
    pts.need_items([it for row in items for it in row] + [bad])
    pts.resolve()
    vkjs = [M.vk_json(pts, key) for key in keys]
    texts = [[(M.proof_json(pts, it.proof), M.public_json(it.signals)) for it in row] for row in items]
    bad_text = (M.proof_json(pts, bad.proof), M.public_json(bad.signals))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def batch(counts, seed):
        b = [(k, texts[k][i % per]) for k, c in enumerate(counts) for i in range(c)]
        random.Random(seed).shuffle(b)
        return [pq[0] for _, pq in b], [pq[1] for _, pq in b], [k for k, _ in b]

    def loop(call, proofs, publics, key_of, nk):
        t0 = time.perf_counter()
        out = [None] * len(proofs)
        for k in range(nk):
            at = [i for i, t in enumerate(key_of) if t == k]
            if at:
                got = call([proofs[i] for i in at], [publics[i] for i in at], vkjs[k])
                for i, v in zip(at, got[0] if isinstance(got, tuple) else got):
                    out[i] = v
        return (time.perf_counter() - t0) * 1e3, out

    def mixed(vs, proofs, publics, key_of):
        t0 = time.perf_counter()
        got, rep = vs.verify(proofs, publics, key_of)
        return (time.perf_counter() - t0) * 1e3, rep.parse_ms, rep.device_ms, got, rep

    med = statistics.median
    spread = lambda xs: max(xs) - min(xs)

    def compare(label, counts, seed, tamper=None):
        nk = len(counts)
        proofs, publics, key_of = batch(counts, seed)
        want = [1] * len(proofs)
        if tamper is not None:
            proofs.insert(tamper, bad_text[0]), publics.insert(tamper, bad_text[1]), key_of.insert(tamper, 3), want.insert(tamper, 0)
        with K.VkSet(vkjs[:nk]) as vs:
            m = mixed(vs, proofs, publics, key_of)               # warm-up, and the verdicts
            assert m[3] == want and m[4].path == int(tamper is None), (label, m[4].path)
            assert loop(K.groth16_verify_batch_combined, proofs, publics, key_of, nk)[1] == want
            rows_m, rows_l, rows_i = [], [], []
            if a.trace_keys:
                mixed(vs, proofs, publics, key_of)
                return
            for _ in range(a.runs):
                rows_m.append(mixed(vs, proofs, publics, key_of)[:3])
                rows_l.append(loop(K.groth16_verify_batch_combined, proofs, publics, key_of, nk)[0])
                if tamper is not None:
                    rows_i.append(loop(K.groth16_verify_batch, proofs, publics, key_of, nk)[0])
        w = [r[0] for r in rows_m]
        s = (f"  {label:>14} {nk:>4} {med(w):9.2f} {spread(w):7.2f} {med(r[1] for r in rows_m):9.2f} {med(r[2] for r in rows_m):9.2f} "
             f"{med(rows_l):10.2f} {spread(rows_l):8.2f} {med(rows_l) / med(w):7.2f}")
        if rows_i:
            s += f"   per-item stage for every key (loop of groth16_verify_batch): {med(rows_i):9.2f}"
        emit(s)

    n = a.n
    if a.trace_keys:
        compare("trace", [n // a.trace_keys] * a.trace_keys, 1)
        compare("trace bad", [n // a.trace_keys] * a.trace_keys, 1, tamper=n // 2)
        return
    emit(f"# K.VkSet.verify (mixed) and a loop of groth16_verify_batch_combined over the keys, interleaved in one process; n = {n} valid")
    emit(f"# proofs, two public signals; medians of {a.runs} runs after one warm-up of each; ms; spread = max − min of the runs; x = loop / mixed")
    emit(f"# {'batch':>14} {'K':>4} {'mix_wall':>9} {'spread':>7} {'mix_parse':>9} {'mix_after':>9} {'loop_wall':>10} {'spread':>8} {'x':>7}")
    for nk in ks:
        compare("even", [n // nk] * nk, nk)
    if 64 in ks:
        compare("half in key 0", [n // 2] + [(n // 2) // 63] * 63, 7)
        emit("# one bad tenant: K = 64, one invalid proof in key 3; the loop pays one failed combined attempt and that key's fallback")
        compare("one bad tenant", [n // 64] * 64, 64, tamper=n // 2)

    # ---- the segmented sum alone, on resident operands shaped as the mixed call's
    lib = K.lib()

    def resident(fn):
        fn()
        K.check(lib.icicle_device_synchronize(), "sync")
        ts = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            fn()
            K.check(lib.icicle_device_synchronize(), "sync")
            ts.append((time.perf_counter() - t0) * 1e3)
        return med(ts), spread(ts)

    emit("# icicle_snark_msm_segmented alone: resident operands, 3·K segments (K of n/K 128-bit entries, K of 3 and K of 1 254-bit entries);")
    emit("# wall time of the call and a device synchronisation, ms (median, spread)")
    emit(f"# {'K':>4} {'cut 256':>16} {'cut 1024':>16} {'cut 4096':>16}")
    nrng = np.random.default_rng(5)
    for nk in ks:
        lens = [n // nk] * nk + [3] * nk + [1] * nk
        total = sum(lens)
        sc = nrng.integers(0, 1 << 62, size=(total, 4), dtype=np.uint64)
        sc[:n, 2:] = 0
        pts_d = K.DeviceVec.from_host(K.generator_mul("g1", nrng.integers(1, 1 << 62, size=(total, 4), dtype=np.uint64)))
        sc_d, out_d = K.DeviceVec.from_host(sc), K.DeviceVec(3 * nk * 64)
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        bits = np.array([128] * nk + [254] * 2 * nk, dtype=np.uint8)
        row = f"  {nk:>4}"
        for cut in (256, 1024, 4096):
            t = resident(lambda: K.check(lib.icicle_snark_msm_segmented(K.ptr_of(pts_d), K.ptr_of(sc_d), K.ptr_of(offsets), C.c_uint32(3 * nk), K.ptr_of(bits),
                                                                     C.c_uint32(cut), None, K.ptr_of(out_d)), "msm_segmented"))
            row += f" {t[0]:9.3f} {t[1]:6.3f}"
        emit(row)
        for d in (pts_d, sc_d, out_d):
            d.free()
    emit("# icicle_snark_pairing_product over 3·K resident pairs (the tail's Miller launch, plus the product passes and one final exponentiation), ms")
    for nk in ks:
        P = K.DeviceVec.from_host(K.generator_mul("g1", nrng.integers(1, 1 << 62, size=(3 * nk, 4), dtype=np.uint64)))
        Q = K.DeviceVec.from_host(K.generator_mul("g2", nrng.integers(1, 1 << 62, size=(3 * nk, 4), dtype=np.uint64)))
        out = K.DeviceVec(12 * 32)
        t = resident(lambda: K.check(lib.icicle_snark_pairing_product(K.ptr_of(P), K.ptr_of(Q), C.c_uint64(3 * nk), None, K.ptr_of(out)), "pairing_product"))
        emit(f"  {nk:>4} {t[0]:9.3f} {t[1]:6.3f}")
        for d in (P, Q, out):
            d.free()
    emit("# groth16_vkset_new: wall time per key (parse, host subgroup tests, upload), ms")
    for nk in ks:
        ts = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            K.VkSet(vkjs[:nk]).free()
            ts.append((time.perf_counter() - t0) * 1e3 / nk)
        emit(f"  {nk:>4} {med(ts):9.3f} {spread(ts):6.3f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
