"""The packed witness on the three benchmark workloads: what the format saves in bytes, what the decode costs, and whether proving
and checking from it are faster than from a .wtns.

    python profiles/bench_wtns_pack.py --workload aadhaar_standin|keyless_standin|1600k [--rounds 12]

One process per workload (bench.py's own inputs), every variant of a figure INTERLEAVED round by round in that process, medians and
minima over --rounds rounds after two warm-up rounds:

    sizes        the .wtns, its packed form, bytes a value; the host packer's and the host decoder's wall time
    decode       groth16_wtns_unpack from a host buffer: the kernel alone (events), the upload of sections 2 to 4, the whole device part
    prove        groth16_prove_mem from a host buffer | groth16_prove_packed | groth16_prove_mem(resident) — wall time of the call
    check        groth16_witness_check | groth16_witness_check_packed — wall time, upload and device time; on 1600k over the
                 workload's own circuit, on a stand-in over a 200 k-constraint circuit of the same generator (synth.standin_circuit:
                 the .r1cs writer is a Python loop), whose witness has the stand-in's mix

One JSON line per process.  profiles/wtns_pack_sweep.txt is the record.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def stat(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="aadhaar_standin")
    ap.add_argument("--rounds", type=int, default=12)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    K = importlib.import_module("icicle-snark_amd")
    S = importlib.import_module("icicle-snark_amd.synth")
    import bench
    K.set_device("HIP", 0)
    zkey, wtns, nc, what, standin = bench.workload_inputs(K, S, a.workload)
    out = {"workload": a.workload, "constraints": nc, "rounds": a.rounds}

    # ---- sizes, and the host's two directions
    t0 = time.perf_counter()
    wtnz, rep = K.wtns_pack(wtns)
    out["host_pack_ms"] = round(ms(t0), 1)
    t0 = time.perf_counter()
    back, _ = K.wtns_unpack(wtnz)
    out["host_unpack_ms"] = round(ms(t0), 1)
    assert back == wtns
    n = rep.n_witness
    out.update({"values": n, "wtns_bytes": len(wtns), "wtnz_bytes": len(wtnz), "bytes_per_value": round(len(wtnz) / n, 3), "ratio": round(len(wtnz) / len(wtns), 4)})

    # ---- the decode alone
    rows = []
    for k in range(a.rounds + 2):
        t0 = time.perf_counter()
        dev, rep = K.wtns_unpack(wtnz, device="HIP")
        rows.append((rep.kernel_ms, rep.upload_ms, rep.device_ms, rep.download_ms, ms(t0)))
    assert dev == wtns
    rows = rows[2:]
    out["decode"] = {name: stat([r[c] for r in rows]) for c, name in enumerate(("kernel_ms", "upload_ms", "device_ms", "download_ms", "wall_ms"))}
    out["decode"]["kernel_ns_per_value"] = round(out["decode"]["kernel_ms"]["median"] * 1e6 / n, 3)

    # ---- the prove, three ways, interleaved
    cm = K.CacheManager()
    cm.load("k", zkey)
    want = cm.prove_mem("k", wtns, 3, 5)[:2]
    assert cm.prove_packed("k", wtnz, 3, 5)[:2] == want
    variants = (("prove_mem_host_buffer", lambda: cm.prove_mem("k", wtns, 3, 5)), ("prove_packed", lambda: cm.prove_packed("k", wtnz, 3, 5)),
                ("prove_resident", lambda: cm.prove_mem("k", wtns, 3, 5, resident=True)))
    times = {name: [] for name, _ in variants}
    for k in range(a.rounds + 2):
        for name, call in variants:
            t0 = time.perf_counter()
            got = call()
            times[name].append(ms(t0))
            assert got[:2] == want
    out["prove"] = {name: stat(v[2:]) for name, v in times.items()}
    cm.evict("k")
    cm.close()
    K.release_domain()

    # ---- the witness check, both ways, interleaved
    if standin:
        r, w = S.standin_circuit(200_000, 4, 4096, seed=11)
        r1cs, cw = S.write_r1cs(r.to_lists()), S.write_wtns(w)
        out["check_circuit"] = "standin_circuit(200000, 4, 4096)"
    else:
        r1cs, cw = S.write_r1cs_squaring_chain(nc), wtns
        out["check_circuit"] = "the workload's"
    cz = K.wtns_pack(cw)[0]
    out["check_wtns_wtnz_bytes"] = [len(cw), len(cz)]
    with K.R1cs(r1cs) as h:
        variants = (("check", lambda: h.check(cw)), ("check_packed", lambda: h.check_packed(cz)))
        times = {name: [] for name, _ in variants}
        for k in range(a.rounds + 2):
            for name, call in variants:
                t0 = time.perf_counter()
                ok, rep = call()
                times[name].append((ms(t0), rep.upload_ms, rep.device_ms))
                assert ok is True
        out["check"] = {name: {col: stat([r[c] for r in v[2:]]) for c, col in enumerate(("wall_ms", "upload_ms", "device_ms"))} for name, v in times.items()}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
