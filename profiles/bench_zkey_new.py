"""groth16_zkey_new on benchmark/1600k and a synthesised power-21 .ptau, and the sweep of its heavy-column threshold over a
circuit of the same size with the constant wire in every row.

    python profiles/bench_zkey_new.py --make DIR                 synthesise c.r1cs, fan.r1cs, w.wtns and pot.ptau into DIR
    python profiles/bench_zkey_new.py --dir DIR [--new-only]     one process: the keys built and timed, the sweep, then the built key
                                                                 through groth16_zkey_verify_ptau and groth16_zkey_check
    python profiles/bench_zkey_new.py --dir DIR --prove --root ROOT --label L
                                                                 one process of library ROOT: warm proves with the key --dir built

The .ptau is profiles/bench_zkey_verify.py's (the blocks that are read hold the Lagrange values, every other block the identity).
fan.r1cs is the squaring chain with the constant wire added to A, B and C of every constraint under small varying coefficients: three
columns of 1.6 M terms.  --new-only builds each key once per threshold and nothing else (for a run under rocprofv3 --kernel-trace
--stats).  ROOT is a checkout with a built package: a parent commit's build in another directory gives the other side of an
interleaved comparison of the prove path — one process of each per round.  One JSON line per process.
profiles/zkey_new_sweep.txt is the record.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = [16, 32, 64, 128, 256, 1024, 4096, 65536]


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def write_r1cs_fan(S, N):
    """the squaring chain's rows, each with a first term on wire 0: coefficient 1 + (j mod 7) in A, 1 in B, 2 + (j mod 3) in C"""
    j = np.arange(N, dtype=np.uint32)
    prev = np.where(j == 0, 2, j + 2).astype(np.uint32)
    cur = np.where(j == N - 1, 1, j + 3).astype(np.uint32)
    rec = np.zeros((N, 3, 19), dtype=np.uint32)     # {count, wire 0, value[8], wire, value[8]}
    rec[:, :, 0] = 2
    rec[:, 0, 2] = 1 + j % 7
    rec[:, 1, 2] = 1
    rec[:, 2, 2] = 2 + j % 3
    rec[:, 0, 10] = prev
    rec[:, 1, 10] = prev
    rec[:, 2, 10] = cur
    rec[:, :, 11] = 1
    return S._r1cs_file(N + 2, 1, N, 0, rec.tobytes(), (1, 2, 3))


def build(h, pp, out, thr, runs):
    rows = []
    for _ in range(runs):
        t0 = time.perf_counter()
        _, rep = h.new_zkey(pp, out=out, heavy_column_terms=thr)
        rows.append([round(ms(t0), 1), round(rep.upload_ms, 1), round(rep.device_ms, 1), round(rep.download_ms, 1), round(rep.write_ms, 1)])
    return rows, rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make", default="")
    ap.add_argument("--dir", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default="this")
    ap.add_argument("--n", type=int, default=1600000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--proves", type=int, default=20)
    ap.add_argument("--new-only", action="store_true")
    ap.add_argument("--prove", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    K = importlib.import_module("icicle-snark_amd")
    S = importlib.import_module("icicle-snark_amd.synth")
    K.set_device("HIP", 0)
    k = (a.n + 2 - 1).bit_length()                      # benchmark/<n>: n constraints, one public signal
    if a.make:
        sys.path.insert(0, os.path.join(ROOT, "profiles"))
        import bench
        from bench_zkey_verify import write_ptau_for_domain
        t0 = time.perf_counter()
        open(os.path.join(a.make, "c.r1cs"), "wb").write(S.write_r1cs_squaring_chain(a.n))
        open(os.path.join(a.make, "fan.r1cs"), "wb").write(write_r1cs_fan(S, a.n))
        open(os.path.join(a.make, "w.wtns"), "wb").write(S.write_wtns(S.squaring_chain_witness(a.n)))
        t1 = time.perf_counter()
        write_ptau_for_domain(K, S, bench, k, os.path.join(a.make, "pot.ptau"))
        print(json.dumps({"ptau_bytes": os.path.getsize(os.path.join(a.make, "pot.ptau")), "domain_power": k, "make_circuits_s": round(t1 - t0, 1),
                          "make_ptau_s": round(time.perf_counter() - t1, 1)}), flush=True)
        return
    pp, out_path = os.path.join(a.dir, "pot.ptau"), os.path.join(a.dir, "out.zkey")
    if a.prove:
        wtns = open(os.path.join(a.dir, "w.wtns"), "rb").read()
        cm = K.CacheManager()
        cm.load_file("k", out_path)
        pj, qj, _ = cm.prove_mem("k", wtns, 3, 5)
        for _ in range(5):
            cm.prove_mem("k", wtns, 3, 5, resident=True)
        res, up = [], []
        for _ in range(a.proves):
            t0 = time.perf_counter()
            cm.prove_mem("k", wtns, 3, 5, resident=True)
            res.append(ms(t0))
        for _ in range(a.proves):
            t0 = time.perf_counter()
            cm.prove_mem("k", wtns, 3, 5)
            up.append(ms(t0))
        cm.evict("k")
        cm.close()
        span = lambda xs: [round(statistics.median(xs), 3), round(min(xs), 3), round(max(xs), 3)]
        verified = K.groth16_verify_json(pj, qj, K.zkey_export_vk(open(out_path, "rb").read())) if hasattr(K, "zkey_export_vk") else None
        print(json.dumps({"label": a.label, "warm_prove_resident_ms_median_min_max": span(res), "warm_prove_with_upload_ms_median_min_max": span(up),
                          "proof_of_the_built_key_verifies": verified}), flush=True)
        return
    out = {"n": a.n, "domain_power": k, "columns": "wall, upload, device, download, write (ms)"}
    verdicts = []
    for name in ("fan", "c"):                           # c last: out.zkey is then benchmark/1600k's key
        h = K.R1cs(os.path.join(a.dir, name + ".r1cs"))
        if name == "fan":
            sweep = {}
            for thr in THRESHOLDS:
                rows, rep = build(h, pp, out_path, thr, 1 if a.new_only else a.runs)
                sweep[thr] = {"runs": rows, "heavy_columns": rep.heavy_columns, "heavy_items": rep.heavy_items}
            out["fan_sweep"] = sweep
            out["fan_longest_column"] = rep.longest_column
        rows, rep = build(h, pp, out_path, 0, 1 if a.new_only else a.runs + 1)
        out[name + "_default"] = rows
        out[name + "_sizes"] = {"n_vars": rep.n_vars, "domain": rep.domain, "n_coeffs": rep.n_coeffs, "zkey_bytes": rep.zkey_bytes,
                                "longest_column": rep.longest_column, "heavy_columns": rep.heavy_columns, "heavy_items": rep.heavy_items}
        if not a.new_only:
            t0 = time.perf_counter()
            ok, vrep = h.verify_zkey(out_path, pp)
            out[name + "_verify_wall_ms_kind_mask"] = [round(ms(t0), 1), vrep.kind, vrep.failed_mask]
            verdicts.append((name + " verify", ok))
            ok, mrep = h.match_zkey(open(out_path, "rb").read())
            verdicts.append((name + " match", ok))
        h.close()
    out["unexpected_verdicts"] = [v for v in verdicts if not v[1]]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
