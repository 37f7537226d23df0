"""groth16_ptau_prepare on a synthesised ceremony: sections 12 to 15 of a powers-of-tau file of a given power.

    python profiles/bench_ptau_prepare.py --make DIR --power P       synthesise an UNPREPARED file (sections 1 to 7, the synthesiser's
                                                                     τ, α, β) into DIR/pot_P.ptau
    python profiles/bench_ptau_prepare.py --dir DIR --power P        one process: the preparation timed (the _file entry,
                                                                     DIR/pot_P.ptau → DIR/pot_P_final.ptau), --runs + 1 times
    python profiles/bench_ptau_prepare.py --dir DIR --power P --compare   also: the written file against synth.write_ptau's, which
                                                                     knows τ — every byte outside section 12's last block
                                                                     (small powers: the synthesiser's Lagrange values are Python integers)

--prepare-only prepares once and does nothing else (for a run under rocprofv3 --kernel-trace --stats, alone: no counters in the
same run).  ICICLE_SNARK_TRACE_PTAU_PREPARE=1 prints the stage times per section on stderr.  One JSON line per process.
profiles/ptau_prepare_sweep.txt is the record.
"""
import argparse
import importlib
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def section(sid, payload):
    return struct.pack("<IQ", sid, len(payload)) + payload


def make(K, S, power):
    """sections 1 to 7 of synth.write_ptau's layout, the powers multiplied out on the GPU"""
    import bench
    to_mont = bench._to_mont(K)
    tau, alpha, beta = S.toxic_waste()[:3]
    N = 1 << power
    pw = [1] * (2 * N - 1)
    for i in range(1, 2 * N - 1):
        pw[i] = pw[i - 1] * tau % S.R_MOD
    arr = S.ints_to_arr(pw)
    one = lambda k: S.ints_to_arr([k] * N)
    low = np.ascontiguousarray(arr[:N])
    g1 = lambda sc: np.ascontiguousarray(to_mont(K.generator_mul("g1", np.ascontiguousarray(sc)))).tobytes()
    g2 = lambda sc: np.ascontiguousarray(to_mont(K.generator_mul("g2", np.ascontiguousarray(sc)))).tobytes()
    hdr = struct.pack("<I", 32) + S.Q_MOD.to_bytes(32, "little") + struct.pack("<II", power, power)
    secs = [(1, hdr), (2, g1(arr)), (3, g2(low)), (4, g1(K.mul_scalars(low, one(alpha)))), (5, g1(K.mul_scalars(low, one(beta)))),
            (6, g2(S.ints_to_arr([beta]))), (7, struct.pack("<I", 0))]
    return b"ptau" + struct.pack("<II", 1, len(secs)) + b"".join(section(s, p) for s, p in secs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make", default="")
    ap.add_argument("--dir", default="")
    ap.add_argument("--power", type=int, default=12)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--prepare-only", action="store_true")
    ap.add_argument("--compare", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    K = importlib.import_module("icicle-snark_amd")
    S = importlib.import_module("icicle-snark_amd.synth")
    K.set_device("HIP", 0)
    if a.make:
        t0 = time.perf_counter()
        image = make(K, S, a.power)
        open(os.path.join(a.make, "pot_%d.ptau" % a.power), "wb").write(image)
        print(json.dumps({"power": a.power, "ptau_bytes": len(image), "make_s": round(time.perf_counter() - t0, 1)}), flush=True)
        return
    src, dst = os.path.join(a.dir, "pot_%d.ptau" % a.power), os.path.join(a.dir, "pot_%d_final.ptau" % a.power)
    out = {"power": a.power, "columns": "wall, upload, device, download, write (ms)"}
    rows = []
    for _ in range(1 if a.prepare_only else a.runs + 1):
        t0 = time.perf_counter()
        _, rep = K.ptau_prepare(src, out=dst)
        rows.append([round(ms(t0), 1), round(rep.upload_ms, 1), round(rep.device_ms, 1), round(rep.download_ms, 1), round(rep.write_ms, 1)])
    out["prepare"] = rows
    out["sizes"] = {"points": list(rep.points), "ptau_bytes": rep.ptau_bytes}
    if a.compare and not a.prepare_only:
        import bench
        got = open(dst, "rb").read()
        t0 = time.perf_counter()
        want = S.write_ptau(a.power, lambda g, sc: K.generator_mul(g, sc), points_to_mont=bench._to_mont(K))
        N = 1 << a.power
        cut = len(want) - (2 * N - 1) * (128 + 64 + 64) - 3 * 12 - 2 * N * 64      # section 12's last block
        out["equal_to_the_synthesisers_outside_the_last_block"] = len(got) == len(want) and got[:cut] == want[:cut] and got[cut + 2 * N * 64:] == want[cut + 2 * N * 64:]
        out["last_block_differs"] = got[cut:cut + 2 * N * 64] != want[cut:cut + 2 * N * 64]
        out["info_power"] = K.ptau_info(got, domain_power=a.power).power
        out["compare_s"] = round(time.perf_counter() - t0, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
