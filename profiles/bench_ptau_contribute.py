"""groth16_ptau_contribute on a ceremony's starting file: one contribution to a powers-of-tau file of a given power.

    python profiles/bench_ptau_contribute.py --make DIR --power P       groth16_ptau_new's file into DIR/pot_P_0000.ptau (host only)
    python profiles/bench_ptau_contribute.py --dir DIR --power P        one process: the contribution timed (the _file entry,
                                                                        DIR/pot_P_0000.ptau → DIR/pot_P_0001.ptau), --runs + 1 times,
                                                                        with secrets from the operating system
    python profiles/bench_ptau_contribute.py --dir DIR --power P --audit   also: groth16_ptau_contributions on the written file, timed

The input is the file of τ = α = β = 1, whose points are all generators: the kernels' work does not depend on the points' values
(every lane walks 256 steps over its own scalar c·τ′^i), and after one contribution the file is a general one — --from-out
contributes to DIR/pot_P_0001.ptau instead, to show it.  --contribute-only contributes once and does nothing else (for a run under
rocprofv3 --kernel-trace --stats, alone: no counters in the same run).  ICICLE_SNARK_TRACE_PTAU_CONTRIBUTE=1 prints the stage
times on stderr.  One JSON line per process.  profiles/ptau_contribute_sweep.txt is the record.
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make", default="")
    ap.add_argument("--dir", default="")
    ap.add_argument("--power", type=int, default=12)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--contribute-only", action="store_true")
    ap.add_argument("--from-out", action="store_true")
    ap.add_argument("--audit", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    K = importlib.import_module("icicle-snark_amd")
    if a.make:
        t0 = time.perf_counter()
        K.ptau_new(a.power, out=os.path.join(a.make, "pot_%d_0000.ptau" % a.power))
        print(json.dumps({"power": a.power, "ptau_bytes": K.ptau_new_size(a.power), "new_ms": round(ms(t0), 1)}), flush=True)
        return
    K.set_device("HIP", 0)
    first, second, third = (os.path.join(a.dir, "pot_%d_%04d.ptau" % (a.power, i)) for i in range(3))
    src, dst = (second, third) if a.from_out else (first, second)
    out = {"power": a.power, "input": os.path.basename(src), "columns": "wall, upload, device, download, write (ms)"}
    rows = []
    for _ in range(1 if a.contribute_only else a.runs + 1):
        t0 = time.perf_counter()
        _, rep = K.ptau_contribute(src, out=dst, name="bench")
        rows.append([round(ms(t0), 1), round(rep.upload_ms, 1), round(rep.device_ms, 1), round(rep.download_ms, 1), round(rep.write_ms, 1)])
    out["contribute"] = rows
    out["sizes"] = {"points": list(rep.points), "ptau_bytes": rep.ptau_bytes, "contribution": rep.contribution}
    if a.audit and not a.contribute_only:
        image = open(dst, "rb").read()
        t0 = time.perf_counter()
        ok, rep = K.ptau_contributions(image)
        out["audit"] = {"ok": ok, "count": rep.count, "ms": round(ms(t0), 1)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
