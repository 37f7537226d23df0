"""Sweep of groth16_verify_batch_combined against groth16_verify_batch, interleaved in one process on the same inputs.

    python scratch/bench_verify_combined.py [--sizes 1,16,256,4096,65536] [--runs 5] [--out profiles/verify_combined_sweep.txt]
    python scratch/bench_verify_combined.py --trace-n 4096      (one warm-up and one timed call of each, for a kernel trace)

Proofs: the golden proofs of tests/golden/groth16.json (one public signal), re-randomised on the host into 256 distinct valid
proofs and tiled to n, as scratch/bench_verify_batch.py does.  Per size: a warm-up call of each function, then `--runs` rounds
of (per-item call, combined call); the median wall time of each, beside the host parse time and the device time the library
reports (per-item: HIP events, first upload to last verdict; combined: wall time from the end of the parse to the verdicts,
host tail included).  Last, the worst case at n = 4096: one invalid proof, which pays the combined attempt and the fallback."""
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
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-n", type=int, default=0)
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
    batch = lambda n: ([distinct[i % 256][0] for i in range(n)], [distinct[i % 256][1] for i in range(n)])
    if a.trace_n:
        proofs, publics = batch(a.trace_n)
        for _ in range(2):
            assert K.groth16_verify_batch(proofs, publics, vkj) == [1] * a.trace_n
            assert K.groth16_verify_batch_combined(proofs, publics, vkj) == ([1] * a.trace_n, 1)
        return
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, proofs, publics):
        t0 = time.perf_counter()
        fn(proofs, publics, vkj)
        wall = (time.perf_counter() - t0) * 1e3
        return (wall,) + K.groth16_verify_batch_last_timings()

    def rounds(proofs, publics, want, want_path):
        assert K.groth16_verify_batch(proofs, publics, vkj) == want  # warm-up, and the verdicts
        assert K.groth16_verify_batch_combined(proofs, publics, vkj) == (want, want_path)
        per, com = [], []
        for _ in range(a.runs):
            per.append(timed(K.groth16_verify_batch, proofs, publics))
            com.append(timed(K.groth16_verify_batch_combined, proofs, publics))
        med = lambda rows, k: statistics.median(r[k] for r in rows)
        return [med(per, k) for k in range(3)], [med(com, k) for k in range(3)]

    emit(f"# groth16_verify_batch (per-item) and groth16_verify_batch_combined interleaved in one process, all-valid batches, one public")
    emit(f"# signal; medians of {a.runs} runs after one warm-up call of each per size; times in ms; ratios = per-item / combined")
    emit(f"# {'n':>6} {'item_wall':>9} {'item_parse':>10} {'item_dev':>9} {'comb_wall':>9} {'comb_parse':>10} {'comb_dev':>9} {'wall_x':>7} {'dev_x':>7}")
    for n in [int(x) for x in a.sizes.split(",")]:
        proofs, publics = batch(n)
        p, c = rounds(proofs, publics, [1] * n, 1)
        emit(f"  {n:>6} {p[0]:9.2f} {p[1]:10.2f} {p[2]:9.2f} {c[0]:9.2f} {c[1]:10.2f} {c[2]:9.2f} {p[0] / c[0]:7.2f} {p[2] / c[2]:7.2f}")
    n = 4096
    proofs, publics = batch(n)
    pu = json.loads(publics[2777])
    publics[2777] = json.dumps([str(int(pu[0]) ^ 2)] + pu[1:])
    want = [1] * n
    want[2777] = 0
    p, c = rounds(proofs, publics, want, 0)
    emit(f"# worst case, n = {n} with ONE invalid proof: the combined attempt, then the per-item fallback")
    emit(f"  {n:>6} {p[0]:9.2f} {p[1]:10.2f} {p[2]:9.2f} {c[0]:9.2f} {c[1]:10.2f} {c[2]:9.2f} {p[0] / c[0]:7.2f} {p[2] / c[2]:7.2f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
