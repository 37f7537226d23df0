"""groth16_zkey_check_file on the benchmark/1600k key beside groth16_cache_load_file and the warm prove of the same key.

    python profiles/bench_zkey_check.py --make DIR                      synthesise the key and the witness into DIR
    python profiles/bench_zkey_check.py --root ROOT --dir DIR --label L one process of library ROOT: loads, warm proves, checks

ROOT is a checkout with a built package (default: this one); a parent commit's build in another directory gives the other side
of an interleaved comparison — run one process of each per round.  A library without groth16_zkey_check skips the checks.
--check-only leaves the loads and proves out (for a run under rocprofv3 --kernel-trace --stats).  One JSON line per process.
profiles/zkey_check_sweep.txt holds the figures of such a run.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make", default="")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--dir", default="")
    ap.add_argument("--label", default="this")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--proves", type=int, default=20)
    ap.add_argument("--check-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    K = importlib.import_module("icicle-snark_amd")
    K.set_device("HIP", 0)
    if a.make:
        S = importlib.import_module("icicle-snark_amd.synth")
        import bench
        zkey, wtns = bench.make_inputs(K, S, 1600000)
        open(os.path.join(a.make, "c.zkey"), "wb").write(zkey)
        open(os.path.join(a.make, "w.wtns"), "wb").write(wtns)
        print(json.dumps({"zkey_bytes": len(zkey), "wtns_bytes": len(wtns)}), flush=True)
        return
    zp = os.path.join(a.dir, "c.zkey")
    wtns = open(os.path.join(a.dir, "w.wtns"), "rb").read()
    out = {"label": a.label}
    if not a.check_only:
        cm = K.CacheManager()
        loads = []
        for k in range(a.runs + 1):
            t0 = time.perf_counter()
            cm.load_file("k", zp, wait_tables=False)          # what groth16_cache_load_file itself takes (tables deferred)
            loads.append((time.perf_counter() - t0) * 1e3)
            if k < a.runs:
                cm.tables_ready("k", wait=True)
                cm.evict("k")
        out["load_file_ms"] = [round(x, 1) for x in loads[1:]]     # the first one pays the process's first streams and staging
        out["load_file_first_ms"] = round(loads[0], 1)
        cm.tables_ready("k", wait=True)
        cm.prove_mem("k", wtns, 3, 5)
        for _ in range(5):
            cm.prove_mem("k", wtns, 3, 5, resident=True)
        pr = []
        for _ in range(a.proves):
            t0 = time.perf_counter()
            cm.prove_mem("k", wtns, 3, 5, resident=True)
            pr.append((time.perf_counter() - t0) * 1e3)
        out["warm_prove_ms_median"] = round(statistics.median(pr), 3)
        out["warm_prove_ms_min_max"] = [round(min(pr), 3), round(max(pr), 3)]
        cm.evict("k")
        cm.close()
        K.release_domain()
    if hasattr(K, "zkey_check_file"):
        rows = []
        for k in range(a.runs + 1):
            t0 = time.perf_counter()
            ok, rep = K.zkey_check_file(zp)
            wall = (time.perf_counter() - t0) * 1e3
            assert ok, (rep.kind, rep.section, rep.index)
            rows.append([round(wall, 1), round(rep.upload_ms, 1), round(rep.device_ms, 1), round(rep.pairing_ms, 1)])
        out["check_first_wall_upload_device_pairing_ms"] = rows[0]
        out["check_wall_upload_device_pairing_ms"] = rows[1:]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
