"""Everything the two host planners — ntt.hip: ntt_plan / ntt_impl and msm_sort.hip: msm_sort_shape / msm_sort_run — can enqueue,
driven once, for a kernel trace of one build held against another's; and the host cost of a launch-bound transform.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python profiles/bench_host_plans.py trace [--root TREE]
    python profiles/bench_host_plans.py ntt-loop [--root TREE] [--rounds 7]

trace      bn254_ntt at every log n in 0 … 22 in a 2^22 domain, forward and inverse, batch 1 and 3; one coset, every ordering and
           columns_batch at 2^11 and 2^17; one prove of a 2^12 stand-in circuit (its key is built here: more transforms and MSMs);
           bn254_msm twice over device-resident bases (classic layout, then the table) at each length of tests/test_gpu_msm_plans.py,
           once over precomputed bases (precompute_factor 2) and once with large_bucket_factor.  Nothing is checked: the suite does that.
           Restricted to the kernels of the two files, the ordered list of (kernel, grid, workgroup, LDS bytes) is a build's plans.
ntt-loop   1000 asynchronous bn254_ntt calls at 2^12 on device data, one stream, wall time per call enqueued and per call finished:
           the transform is launch-bound, so the figure is the host plan's cost.  One JSON line.

--root: the tree whose library and package run (default: this file's).  profiles/host_plans_refactor_ab.txt is the record.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_LENGTHS = (32768, 32769, 65537, 262145, 524289)
CLASSIC_LENGTHS = (257, 1025, 2049, 4097, 131073)


def scalars(rng, n):
    sc = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 60) - 1)
    return sc


def trace(K, S, bench):
    rng = np.random.default_rng(22)
    K.release_domain()
    K.initialize_domain(K.get_root_of_unity(1 << 22))
    data = K.DeviceVec.from_host(scalars(rng, 3 << 22))
    for logn in range(23):
        for inverse in (False, True):
            for batch in (1, 3):
                K.ntt(data, inverse, batch_size=batch, size=1 << logn)
    for logn in (11, 17):
        for inverse in (False, True):
            K.ntt(data, inverse, batch_size=3, size=1 << logn, coset_gen=np.array([5, 0, 0, 0], dtype=np.uint64))
            for ordering in range(6):
                for cols in (False, True):
                    K.ntt(data, inverse, batch_size=3, size=1 << logn, ordering=ordering, columns_batch=cols)
    data.free()
    K.release_domain()

    r, w = S.standin_circuit(4000, 4, 64, seed=7)
    K.initialize_domain(K.get_root_of_unity(1 << 12))
    zkey, _ = S.setup_sparse(r, bench.GpuVec(K), lambda g, sc: K.generator_mul(g, sc), points_to_mont=bench._to_mont(K))
    K.release_domain()
    cm = K.CacheManager()
    cm.load("k", zkey)
    cm.prove_mem("k", S.write_wtns(w), 3, 5)
    cm.evict("k")
    cm.close()
    K.release_domain()

    points = K.generator_mul("g1", scalars(rng, 128))
    for L in sorted(TABLE_LENGTHS + CLASSIC_LENGTHS):
        d_b, d_s = K.DeviceVec.from_host(np.resize(points, (L,) + points.shape[1:])), K.DeviceVec.from_host(scalars(rng, L))
        K.msm("g1", d_s, d_b)
        K.msm("g1", d_s, d_b)
        d_b.free(); d_s.free()
    L = 4097
    bases, sc = np.resize(points, (L,) + points.shape[1:]), scalars(rng, L)
    K.msm("g1", sc, K.msm_precompute_bases("g1", bases, 2), size=L, precompute_factor=2)
    lib = K.lib()
    lib.create_config_extension.restype = C.c_void_p
    ext = C.c_void_p(lib.create_config_extension())
    lib.config_extension_set_int(ext, b"large_bucket_factor", 10)
    K.msm("g1", sc, bases, ext=ext)
    lib.destroy_config_extension(ext)
    print("trace driver done", flush=True)


def ntt_loop(K, rounds):
    n, calls = 1 << 12, 1000
    K.release_domain()
    K.initialize_domain(K.get_root_of_unity(n))
    st = K.IcicleStream()
    data = K.DeviceVec.from_host(scalars(np.random.default_rng(12), n), st)
    cfg = K.NTTConfig.default()
    cfg.batch_size, cfg.are_inputs_on_device, cfg.are_outputs_on_device, cfg.is_async, cfg.stream = 1, True, True, True, st.handle
    fn, p, size, fwd, ref = K.lib().bn254_ntt, K.ptr_of(data), C.c_int(n), C.c_int(0), C.byref(cfg)
    enq, done = [], []
    for k in range(rounds + 2):
        st.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn(p, size, fwd, ref, p)
        t1 = time.perf_counter()
        st.synchronize()
        t2 = time.perf_counter()
        enq.append((t1 - t0) * 1e6 / calls)
        done.append((t2 - t0) * 1e6 / calls)
    data.free()
    K.release_domain()
    stat = lambda xs: {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}
    print(json.dumps({"ntt_2p12_async_calls": calls, "rounds": rounds, "enqueue_us_per_call": stat(enq[2:]), "finished_us_per_call": stat(done[2:])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["trace", "ntt-loop"])
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    K = importlib.import_module("icicle-snark_amd")
    S = importlib.import_module("icicle-snark_amd.synth")
    K.set_device("HIP", 0)
    if a.mode == "trace":
        import bench
        trace(K, S, bench)
    else:
        ntt_loop(K, a.rounds)


if __name__ == "__main__":
    main()
