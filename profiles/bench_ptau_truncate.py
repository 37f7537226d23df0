"""groth16_ptau_truncate file to file: a powers-of-tau file cut down to a lower power.

    python profiles/bench_ptau_truncate.py --make DIR --power P [--prepared]        the input into DIR: groth16_ptau_new's file, one
                                                                                     contribution with secrets from the operating system
                                                                                     (so its points are general ones), and with --prepared
                                                                                     groth16_ptau_prepare of it
    python profiles/bench_ptau_truncate.py --dir DIR --power P --to p [--prepared]   one process: DIR/pot_P[_prepared].ptau →
                                                                                     DIR/pot_P_to_p[_prepared].ptau through the _file
                                                                                     entry, --runs + 1 times
    python profiles/bench_ptau_truncate.py --dir DIR --power P --to p --prepared --truncate-only
                                                                                     once and nothing else (for a run under rocprofv3
                                                                                     --kernel-trace --stats, alone: no counters in the
                                                                                     same run)
    ... --check                                                                      also: groth16_ptau_verify on the written file

Per run the JSON line holds wall, upload, device, download and write time, the bytes in and out and the points fixed up; device is
the wall time of the device part without the uploads and without the host's copy of the container that runs beside the kernels, lane
test and the way back to the file's form included: the kernel alone is rocprofv3's figure.  ICICLE_SNARK_TRACE_PTAU_TRUNCATE=1 prints the stages on stderr.  One JSON line per process.
profiles/ptau_truncate_sweep.txt is the record.
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
    ap.add_argument("--to", type=int, default=8)
    ap.add_argument("--prepared", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--truncate-only", action="store_true")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    K = importlib.import_module("icicle-snark_amd")
    K.set_device("HIP", 0)
    tail = "_prepared" if a.prepared else ""
    src = os.path.join(a.make or a.dir, "pot_%d%s.ptau" % (a.power, tail))
    if a.make:
        t0 = time.perf_counter()
        new, plain = os.path.join(a.make, "pot_%d_0000.tmp" % a.power), os.path.join(a.make, "pot_%d.ptau" % a.power)
        if not os.path.exists(plain):
            K.ptau_new(a.power, out=new)
            K.ptau_contribute(new, out=plain, name="bench")
            os.unlink(new)
        if a.prepared:
            K.ptau_prepare(plain, out=src)
        print(json.dumps({"power": a.power, "prepared": a.prepared, "ptau_bytes": os.path.getsize(src), "make_ms": round(ms(t0), 1)}), flush=True)
        return
    dst = os.path.join(a.dir, "pot_%d_to_%d%s.ptau" % (a.power, a.to, tail))
    out = {"power": a.power, "to": a.to, "prepared": a.prepared, "input": os.path.basename(src), "columns": "wall, upload, device, download, write (ms)"}
    rows = []
    for _ in range(1 if a.truncate_only else a.runs + 1):
        t0 = time.perf_counter()
        _, rep = K.ptau_truncate(src, a.to, out=dst)
        rows.append([round(ms(t0), 1), round(rep.upload_ms, 2), round(rep.device_ms, 2), round(rep.download_ms, 2), round(rep.write_ms, 1)])
    out["truncate"] = rows
    out["sizes"] = {"in_bytes": rep.in_bytes, "out_bytes": rep.out_bytes, "points_fixed": rep.points_fixed}
    if a.check and not a.truncate_only:
        t0 = time.perf_counter()
        ok, vrep = K.ptau_verify(dst)
        out["verify"] = {"ok": ok, "kind": vrep.kind, "failed_mask": vrep.failed_mask, "ms": round(ms(t0), 1)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
