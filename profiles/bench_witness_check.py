"""groth16_r1cs_load_file, groth16_witness_check and groth16_r1cs_match_zkey on benchmark/1600k beside what a caller pays today to
learn less: the warm prove of the same key and the host groth16_verify of its proof.

    python profiles/bench_witness_check.py --make DIR                      synthesise the key, the witness and the .r1cs into DIR
    python profiles/bench_witness_check.py --root ROOT --dir DIR --label L one process of library ROOT

ROOT is a checkout with a built package (default: this one); a parent commit's build in another directory gives the other side of
an interleaved comparison of the prove path — run one process of each per round.  A library without the .r1cs entry points skips
them.  --check-only leaves the key load, the proves and the verify out (for a run under rocprofv3 --kernel-trace --stats, which
gives each kernel alone).  One JSON line per process.  profiles/witness_check_sweep.txt is the record of three interleaved rounds
and one traced process.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make", default="")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--dir", default="")
    ap.add_argument("--label", default="this")
    ap.add_argument("--n", type=int, default=1600000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--proves", type=int, default=20)
    ap.add_argument("--check-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    K = importlib.import_module("icicle-snark_amd")
    S = importlib.import_module("icicle-snark_amd.synth")
    K.set_device("HIP", 0)
    if a.make:
        import bench
        zkey, wtns = bench.make_inputs(K, S, a.n)
        r1cs = S.write_r1cs_squaring_chain(a.n)
        bad = bytearray(wtns)                                  # for the REPL's wtns-check: one wire in the middle of the chain off
        bad[len(bad) - 32 * (a.n // 2)] ^= 1
        for name, data in (("c.zkey", zkey), ("w.wtns", wtns), ("w_bad.wtns", bytes(bad)), ("c.r1cs", r1cs)):
            open(os.path.join(a.make, name), "wb").write(data)
        print(json.dumps({"zkey_bytes": len(zkey), "wtns_bytes": len(wtns), "r1cs_bytes": len(r1cs)}), flush=True)
        return
    zp, rp = os.path.join(a.dir, "c.zkey"), os.path.join(a.dir, "c.r1cs")
    wtns = open(os.path.join(a.dir, "w.wtns"), "rb").read()
    out = {"label": a.label, "n": a.n}
    med = lambda xs: round(statistics.median(xs), 3)
    span = lambda xs: [round(min(xs), 3), round(max(xs), 3)]
    if not a.check_only:
        cm = K.CacheManager()
        cm.load_file("k", zp)
        pj, qj, _ = cm.prove_mem("k", wtns, 3, 5)
        for _ in range(5):
            cm.prove_mem("k", wtns, 3, 5, resident=True)
        res, up = [], []
        for _ in range(a.proves):
            t0 = time.perf_counter()
            cm.prove_mem("k", wtns, 3, 5, resident=True)
            res.append(ms(t0))
        for _ in range(a.proves):
            t0 = time.perf_counter()
            cm.prove_mem("k", wtns, 3, 5)                      # with the witness upload: what a caller with a new witness pays
            up.append(ms(t0))
        out["warm_prove_resident_ms_median"], out["warm_prove_resident_ms_min_max"] = med(res), span(res)
        out["warm_prove_with_upload_ms_median"], out["warm_prove_with_upload_ms_min_max"] = med(up), span(up)
        cm.evict("k")
        cm.close()
        K.release_domain()
        if hasattr(K, "zkey_export_vk"):
            vk = K.zkey_export_vk(open(zp, "rb").read())
            ver = []
            for _ in range(a.runs + 1):
                t0 = time.perf_counter()
                assert K.groth16_verify_json(pj, qj, vk)
                ver.append(ms(t0))
            out["host_verify_ms"] = [round(x, 2) for x in ver[1:]]
    if hasattr(K, "R1cs"):
        loads = []
        for k in range(a.runs + 1):
            t0 = time.perf_counter()
            h = K.R1cs(rp)
            wall = ms(t0)
            i = h.info
            loads.append([round(wall, 1), round(i.walk_ms, 1), round(i.upload_ms, 1), round(i.device_ms, 1)])
            if k < a.runs:
                h.close()
        out["r1cs_terms_device_bytes"] = [i.n_terms, i.device_bytes]
        out["load_first_wall_walk_upload_device_ms"] = loads[0]    # the first one pays the process's first streams and staging
        out["load_wall_walk_upload_device_ms"] = loads[1:]
        t0 = time.perf_counter()
        info = K.r1cs_info(open(rp, "rb").read())
        out["r1cs_info_wall_ms_incl_read"] = round(ms(t0), 1)
        out["r1cs_info_walk_ms"] = round(info.walk_ms, 1)
        rows, verdicts = [], []
        for k in range(a.proves + 1):
            t0 = time.perf_counter()
            ok, rep = h.check(wtns)
            wall = ms(t0)
            verdicts.append(("check", ok, rep.kind, rep.index))
            rows.append((wall, rep.upload_ms, rep.device_ms))
        out["check_first_wall_upload_device_ms"] = [round(x, 3) for x in rows[0]]
        out["check_wall_upload_device_ms_median"] = [med([r[c] for r in rows[1:]]) for c in range(3)]
        out["check_wall_ms_min_max"] = span([r[0] for r in rows[1:]])
        # an unsatisfying witness: the value of one wire in the middle of the chain + 1 (two constraints read or define it)
        bad = bytearray(wtns)
        off = len(bad) - 32 * (a.n // 2)
        bad[off] ^= 1
        bad = bytes(bad)
        t0 = time.perf_counter()
        ok, rep = h.check(bad)
        out["check_bad_wall_ms_kind_index_failed"] = [round(ms(t0), 3), rep.kind, rep.index, rep.failed]
        verdicts.append(("bad witness", not ok, rep.kind, rep.index))
        zkey = open(zp, "rb").read()
        rows = []
        for k in range(a.runs + 1):
            t0 = time.perf_counter()
            ok, rep = h.match_zkey(zkey)
            wall = ms(t0)
            verdicts.append(("match", ok, rep.kind, rep.index))
            rows.append([round(wall, 1), round(rep.device_ms, 1)])
        out["match_first_wall_device_ms"] = rows[0]
        out["match_wall_device_ms"] = rows[1:]
        h.close()
        out["unexpected_verdicts"] = [v for v in verdicts if not v[1]]         # a sound witness refused, a matching key not matched …
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
