"""The random beacon: what the stretch costs on the host, and groth16_ptau_beacon / groth16_zkey_beacon beside the contribute calls
whose kernels they run.

    python profiles/bench_beacon.py --host                        groth16_beacon_digest for iter_exp 10, 20 and 24, timed (no GPU)
    python profiles/bench_beacon.py --dir DIR --power P           one process: groth16_ptau_new's file into DIR (if absent), then the
                                                                  _file entries of contribute and of beacon on it, --runs + 1 times each
    python profiles/bench_beacon.py --dir DIR --n N               the same for benchmark/<n>'s key (bench.py's, synthesised into DIR if
                                                                  absent) with groth16_zkey_contribute and groth16_zkey_beacon

--iter-exp sets the beacon's (default 10: a stretch of a third of a millisecond, so that the two rows differ by nothing else).  The
written files are audited once each (host), timed: the beacon's audit includes the stretch.  One JSON line per process.
profiles/beacon_sweep.txt is the record.
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASH = bytes(range(64, 96))


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def rows_of(call, runs):
    rows = []
    for _ in range(runs + 1):
        t0 = time.perf_counter()
        rep = call()
        rows.append([round(ms(t0), 1), round(rep.upload_ms, 1), round(rep.device_ms, 1), round(rep.download_ms, 1), round(rep.write_ms, 1)])
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--dir", default="")
    ap.add_argument("--power", type=int, default=-1)
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--iter-exp", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    K = importlib.import_module("icicle-snark_amd")
    if a.host:
        out = {}
        K.beacon_digest(HASH, 0)          # (the library is loaded by its first call)
        for e in (10, 20, 24):
            t0 = time.perf_counter()
            K.beacon_digest(HASH, e)
            out["2^%d hashes, ms" % e] = round(ms(t0), 2)
        print(json.dumps(out), flush=True)
        return
    K.set_device("HIP", 0)
    out = {"iter_exp": a.iter_exp, "columns": "wall, upload, device, download, write (ms)"}
    if a.power >= 0:
        src, c_out, b_out = (os.path.join(a.dir, "pot_%d_%s.ptau" % (a.power, s)) for s in ("0000", "contributed", "beaconed"))
        if not os.path.exists(src):
            K.ptau_new(a.power, out=src)
        out["power"] = a.power
        out["contribute"] = rows_of(lambda: K.ptau_contribute(src, out=c_out, name="bench")[1], a.runs)
        out["beacon"] = rows_of(lambda: K.ptau_beacon(src, HASH, a.iter_exp, name="bench", out=b_out)[1], a.runs)
        audit = K.ptau_contributions
    else:
        S = importlib.import_module("icicle-snark_amd.synth")
        import bench
        src, c_out, b_out = (os.path.join(a.dir, "key_%d%s.zkey" % (a.n, s)) for s in ("", "_contributed", "_beaconed"))
        if not os.path.exists(src):
            open(src, "wb").write(bench.make_inputs(K, S, a.n)[0])
        out["n"] = a.n
        out["contribute"] = rows_of(lambda: K.zkey_contribute(src, name="bench", out=c_out)[1], a.runs)
        out["beacon"] = rows_of(lambda: K.zkey_beacon(src, HASH, a.iter_exp, name="bench", out=b_out)[1], a.runs)
        audit = K.zkey_contributions      # (bench.py's key has γ, δ ≠ 1: POK at record 1 for both files; the verdict is reported, not judged)
    for what, path in (("contribute", c_out), ("beacon", b_out)):
        image = open(path, "rb").read()
        t0 = time.perf_counter()
        ok, rep = audit(image)
        out["audit of " + what] = {"ok": ok, "count": rep.count, "kind": rep.kind, "beacons": len(rep.beacons), "bytes": len(image), "ms": round(ms(t0), 1)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
