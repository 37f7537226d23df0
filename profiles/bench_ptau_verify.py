"""groth16_ptau_verify on a ceremony's file: every power against the others, and sections 12 to 15 against 2 to 5.

    python profiles/bench_ptau_verify.py --make DIR --power P         DIR/pot_P.ptau (groth16_ptau_new and ONE contribution with the
                                                                      operating system's secrets: a general file) and
                                                                      DIR/pot_P_prepared.ptau (groth16_ptau_prepare of it); needs the GPU
    python profiles/bench_ptau_verify.py --dir DIR --power P          one process: the unprepared file verified (the _file entry),
                                                                      --runs + 1 times, with seeds from the operating system
    python profiles/bench_ptau_verify.py --dir DIR --power P --prepared   the same for the prepared file

--verify-only verifies once and does nothing else (for a run under rocprofv3 --kernel-trace --stats, alone: no counters in the same
run).  ICICLE_SNARK_TRACE_PTAU_VERIFY=1 prints the stage times on stderr.  The first run of a process is cold (streams, staging,
code objects); the others are what the sweep calls warm.  One JSON line per process.  profiles/ptau_verify_sweep.txt is the record.
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
    ap.add_argument("--prepared", action="store_true")
    ap.add_argument("--verify-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    K = importlib.import_module("icicle-snark_amd")
    K.set_device("HIP", 0)
    d = a.make or a.dir
    start, raw, prepared = (os.path.join(d, "pot_%d%s.ptau" % (a.power, s)) for s in ("_0000", "", "_prepared"))
    if a.make:
        t0 = time.perf_counter()
        K.ptau_new(a.power, out=start)
        K.ptau_contribute(start, out=raw, name="bench")
        t1 = time.perf_counter()
        K.ptau_prepare(raw, out=prepared)
        os.remove(start)
        print(json.dumps({"power": a.power, "bytes": [os.path.getsize(raw), os.path.getsize(prepared)], "new_contribute_ms": round((t1 - t0) * 1e3, 1),
                          "prepare_ms": round(ms(t1), 1)}), flush=True)
        return
    src = prepared if a.prepared else raw
    out = {"power": a.power, "input": os.path.basename(src), "bytes": os.path.getsize(src), "columns": "wall, upload, device, pairing (ms)"}
    rows = []
    for _ in range(1 if a.verify_only else a.runs + 1):
        t0 = time.perf_counter()
        ok, rep = K.ptau_verify(src)
        rows.append([round(ms(t0), 1), round(rep.upload_ms, 1), round(rep.device_ms, 1), round(rep.pairing_ms, 1)])
    out["verify"] = rows
    out["verdict"] = {"ok": ok, "kind": rep.kind_name, "failed": rep.failed, "points": list(rep.points)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
