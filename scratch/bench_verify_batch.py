"""Sweep of groth16_verify_batch (JSON texts in, verdicts out) against the host verifier's loop.

    python scratch/bench_verify_batch.py [--sizes 1,16,256,4096,65536] [--runs 5] [--host-max 256]

Proofs: the golden proofs of tests/golden/groth16.json (one public signal), re-randomised on the host into 256 distinct
valid proofs (A' = θ⁻¹·A, B' = θ·B + ρ·δ₂, C' = C + ρ·A') and tiled to n.  Per size: a warm-up call, then the median and
range of `--runs` wall times, beside the host parse time and the device time (HIP events) the library reports for the
same calls; the host loop (groth16_verify_json per item) is measured for n ≤ --host-max only."""
import argparse
import importlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

R_ORDER = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,256,4096,65536")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-max", type=int, default=256)
    a = ap.parse_args()
    K = importlib.import_module("icicle-snark_amd")
    S = importlib.import_module("icicle-snark_amd.synth")
    from test_gpu_verify_batch import _g2_proj, _rerandomise
    from test_verify import _golden_vk_json
    K.set_device("HIP", 0)
    g, vkj = _golden_vk_json(S)
    delta2 = _g2_proj(K, json.loads(vkj)["vk_delta_2"])
    rnd = random.Random(1)
    distinct = []
    for k in range(256):
        c = g["cases"][k % 2]
        distinct.append((json.dumps(_rerandomise(K, c["proof"], delta2, rnd.randrange(1, R_ORDER), rnd.randrange(R_ORDER))), json.dumps(c["public"])))
    print(f"# groth16_verify_batch sweep: one public signal, {a.runs} timed runs after one warm-up call per size; times in ms")
    print(f"# {'n':>6} {'wall_med':>9} {'wall_min':>9} {'wall_max':>9} {'parse_med':>9} {'dev_med':>9} {'us/proof':>9} {'host_loop':>10} {'host/proof':>10} {'speedup':>8}")
    for n in [int(x) for x in a.sizes.split(",")]:
        proofs = [distinct[i % 256][0] for i in range(n)]
        publics = [distinct[i % 256][1] for i in range(n)]
        assert K.groth16_verify_batch(proofs, publics, vkj) == [1] * n  # warm-up, and the verdicts
        walls, parses, devs = [], [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            K.groth16_verify_batch(proofs, publics, vkj)
            walls.append((time.perf_counter() - t0) * 1e3)
            p, d = K.groth16_verify_batch_last_timings()
            parses.append(p)
            devs.append(d)
        host = ""
        hostper = ""
        speed = ""
        if n <= a.host_max:
            pe, qe, ve = [x.encode() for x in proofs], [x.encode() for x in publics], vkj.encode()
            t0 = time.perf_counter()
            for i in range(n):
                assert K.lib().groth16_verify_json(pe[i], qe[i], ve) == 1
            h = (time.perf_counter() - t0) * 1e3
            host, hostper = f"{h:10.1f}", f"{h / n:10.2f}"
            speed = f"{h / statistics.median(walls):8.1f}"
        wm = statistics.median(walls)
        print(f"  {n:>6} {wm:9.2f} {min(walls):9.2f} {max(walls):9.2f} {statistics.median(parses):9.2f} {statistics.median(devs):9.2f} "
              f"{wm * 1e3 / n:9.1f} {host:>10} {hostper:>10} {speed:>8}", flush=True)


if __name__ == "__main__":
    main()
