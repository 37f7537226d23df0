"""The packed proving key on the three benchmark workloads: what the format saves in bytes, what packing and unpacking cost file to
file, and what a packed load costs beside the load of the same key unpacked.

    python profiles/bench_zkey_pack.py --workload aadhaar_standin|keyless_standin|1600k [--rounds 7]

One process per workload (bench.py's own inputs), every variant of a figure INTERLEAVED round by round in that process, medians and
minima over --rounds rounds after one warm-up round:

    sizes        the .zkey, its packed form, split into the point sections and section 4, as shares of the .zkey
    files        groth16_zkey_pack_file | groth16_zkey_unpack_file on files in a temporary directory: wall time and the report's
                 split — the sections' copies up, the device part without them, the copies down into the mapped file, msync + rename
    load         groth16_cache_load_file of the .zkey | groth16_cache_load_packed_file of the packed key, both from the page cache
                 (the files were written by this process a moment ago and nothing evicts them: WARM — no cold-file figure is taken),
                 each timed from the call to the end of the first successful prove_mem; the key is evicted between the rounds
    unpack       groth16_points_unpack of section 7's words (G2: the root and the subgroup test) and of section 9's (G1: the root
                 alone) from a host buffer, the report's device part: what the load's unpack kernels are made of

One JSON line per process.  profiles/zkey_pack_sweep.txt is the record.
"""
import argparse
import importlib
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def stat(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def section(image, sid):
    n = struct.unpack_from("<I", image, 8)[0]
    pos = 12
    for _ in range(n):
        s, ln = struct.unpack_from("<IQ", image, pos)
        if s == sid:
            return image[pos + 12:pos + 12 + ln]
        pos += 12 + ln
    raise KeyError(sid)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="1600k")
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    K = importlib.import_module("icicle-snark_amd")
    S = importlib.import_module("icicle-snark_amd.synth")
    import bench
    K.set_device("HIP", 0)
    zkey, wtns, nc, what, standin = bench.workload_inputs(K, S, a.workload)
    out = {"workload": a.workload, "constraints": nc, "rounds": a.rounds}
    tmp = tempfile.mkdtemp(prefix="isnark_zkey_pack_")
    try:
        zp, zz, back = (os.path.join(tmp, n) for n in ("k.zkey", "k.zkez", "back.zkey"))
        with open(zp, "wb") as f:
            f.write(zkey)

        # ---- files, both directions, interleaved
        rows = {"pack": [], "unpack": []}
        for k in range(a.rounds + 1):
            t0 = time.perf_counter()
            _, rep = K.zkey_pack(zp, out=zz)
            rows["pack"].append((ms(t0), rep.upload_ms, rep.device_ms, rep.download_ms, rep.write_ms))
            t0 = time.perf_counter()
            _, urep = K.zkey_unpack(zz, out=back)
            rows["unpack"].append((ms(t0), urep.upload_ms, urep.device_ms, urep.download_ms, urep.write_ms))
        with open(back, "rb") as f:
            assert f.read() == zkey
        os.unlink(back)
        out.update({"zkey_bytes": rep.in_bytes, "zkez_bytes": rep.out_bytes, "ratio": round(rep.out_bytes / rep.in_bytes, 4), "n_coef": rep.n_coef,
                    "points_g1_g2": list(rep.points), "point_bytes": [2 * rep.point_bytes, rep.point_bytes], "section4_bytes": [4 + 44 * rep.n_coef, rep.coef_bytes],
                    "points_share_of_zkey": [round(2 * rep.point_bytes / rep.in_bytes, 4), round(rep.point_bytes / rep.in_bytes, 4)],
                    "section4_share_of_zkey": [round((4 + 44 * rep.n_coef) / rep.in_bytes, 4), round(rep.coef_bytes / rep.in_bytes, 4)],
                    "packed_bound": K.zkey_packed_bound(zkey)})
        out["files"] = {d: {col: stat([r[c] for r in v[1:]]) for c, col in enumerate(("wall_ms", "upload_ms", "device_ms", "download_ms", "write_ms"))} for d, v in rows.items()}

        # ---- the load, both ways, interleaved: until the first prove has succeeded
        cm = K.CacheManager()
        variants = (("load_file", lambda: cm.load_file("k", zp, wait_tables=False)), ("load_packed_file", lambda: cm.load_packed("k", zz, wait_tables=False)))
        times = {name: [] for name, _ in variants}
        want = None
        for k in range(a.rounds + 1):
            for name, call in variants:
                t0 = time.perf_counter()
                call()
                t_load = ms(t0)
                got = cm.prove_mem("k", wtns, 3, 5)[:2]
                times[name].append((ms(t0), t_load))
                want = want or got
                assert got == want
                cm.evict("k")
        out["load"] = {name: {"to_first_proof_ms": stat([r[0] for r in v[1:]]), "load_ms": stat([r[1] for r in v[1:]])} for name, v in times.items()}
        # the stages of one load of each, on stderr
        os.environ["ICICLE_SNARK_TRACE_COLD"] = "1"
        for name, call in variants:
            print(f"[{name}]", file=sys.stderr, flush=True)
            call()
            cm.evict("k")
        del os.environ["ICICLE_SNARK_TRACE_COLD"]
        cm.close()
        K.release_domain()

        # ---- what the unpack kernels are made of
        with open(zz, "rb") as f:
            zkez = f.read()
        parts = {}
        for sid, g2 in ((7, True), (9, False)):
            words = section(zkez, sid)
            dev = []
            for k in range(a.rounds + 1):
                _, prep = K.points_unpack(words, g2=g2)
                dev.append(prep.device_ms)
            n = len(words) // (64 if g2 else 32)
            parts["section_%d" % sid] = {"points": n, "device_ms": stat(dev[1:]), "ns_per_point": round(statistics.median(dev[1:]) * 1e6 / max(n, 1), 2)}
        out["unpack"] = parts
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
