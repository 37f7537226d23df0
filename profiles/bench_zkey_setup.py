"""groth16_setup_file on benchmark/1600k's .r1cs with its per-stage split, the ceremony chain it replaces at the same circuit, and
the sweep of its heavy-column threshold over a circuit of the same size with the constant wire in every row.

    python profiles/bench_zkey_setup.py --make DIR              synthesise c.r1cs, fan.r1cs and w.wtns into DIR
    python profiles/bench_zkey_setup.py --dir DIR [--no-chain]  one process: setup (warm), the sweep, the chain, then the setup's
                                                                key through groth16_zkey_check, r1cs-match and one prove + verify

The chain is ptau-new → ptau-contribute → ptau-prepare → zkey-new → zkey-contribute at the circuit's power, each through its _file
entry with the operating system's secrets, timed by wall clock; its intermediate files are removed as soon as the next step has
read them.  fan.r1cs is profiles/bench_zkey_new.py's.  One JSON line.  profiles/zkey_setup_sweep.txt is the record.
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = [8, 64, 512, 1 << 30]


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def setup_runs(h, out, thr, runs):
    rows = []
    for _ in range(runs):
        t0 = time.perf_counter()
        _, rep = h.setup(out=out, heavy_column_terms=thr)
        rows.append({"wall": round(ms(t0), 1), "upload": round(rep.upload_ms, 2), "device": round(rep.device_ms, 1), "lagrange": round(rep.lagrange_ms, 2),
                     "columns": round(rep.columns_ms, 2), "g1": round(rep.g1_ms, 1), "g2": round(rep.g2_ms, 1), "download": round(rep.download_ms, 1),
                     "write": round(rep.write_ms, 1)})
    return rows, rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make", default="")
    ap.add_argument("--dir", default="")
    ap.add_argument("--n", type=int, default=1600000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-chain", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    K = importlib.import_module("icicle-snark_amd")
    S = importlib.import_module("icicle-snark_amd.synth")
    k = (a.n + 2 - 1).bit_length()                      # benchmark/<n>: n constraints, one public signal
    if a.make:
        from bench_zkey_new import write_r1cs_fan
        t0 = time.perf_counter()
        open(os.path.join(a.make, "c.r1cs"), "wb").write(S.write_r1cs_squaring_chain(a.n))
        open(os.path.join(a.make, "fan.r1cs"), "wb").write(write_r1cs_fan(S, a.n))
        open(os.path.join(a.make, "w.wtns"), "wb").write(S.write_wtns(S.squaring_chain_witness(a.n)))
        print(json.dumps({"domain_power": k, "make_circuits_s": round(time.perf_counter() - t0, 1)}), flush=True)
        return
    K.set_device("HIP", 0)
    p = lambda name: os.path.join(a.dir, name)
    out = {"n": a.n, "domain_power": k, "times": "ms"}
    h = K.R1cs(p("c.r1cs"))
    rows, rep = setup_runs(h, p("setup.zkey"), 0, a.runs + 1)   # the first run is the cold one
    out["setup_default"] = rows
    out["setup_sizes"] = {"n_vars": rep.n_vars, "domain": rep.domain, "n_coeffs": rep.n_coeffs, "zkey_bytes": rep.zkey_bytes, "longest_column": rep.longest_column,
                          "heavy_columns": rep.heavy_columns, "heavy_items": rep.heavy_items}
    # the key is a key: the library's judges, one prove and its verification
    verdicts = [("zkey_check", K.zkey_check_file(p("setup.zkey"))[0])]
    key = open(p("setup.zkey"), "rb").read()
    verdicts.append(("match", h.match_zkey(key)[0]))
    cm = K.CacheManager()
    cm.load("k", key)
    pj, qj, _ = cm.prove_mem("k", open(p("w.wtns"), "rb").read(), 3, 5)
    verdicts.append(("prove + verify", K.groth16_verify_json(pj, qj, K.zkey_export_vk(key))))
    cm.close()
    del key
    fan = K.R1cs(p("fan.r1cs"))
    sweep = {}
    for thr in THRESHOLDS:
        rows, rep = setup_runs(fan, p("fan.zkey"), thr, a.runs)
        sweep[thr] = {"runs": rows, "heavy_columns": rep.heavy_columns, "heavy_items": rep.heavy_items}
    out["fan_sweep"] = sweep
    out["fan_longest_column"] = rep.longest_column
    fan.close()
    os.remove(p("fan.zkey"))
    if not a.no_chain:
        chain, t_all = {}, time.perf_counter()
        t0 = time.perf_counter()
        K.ptau_new(k, out=p("pot0.ptau"))
        chain["ptau-new"] = round(ms(t0), 1)
        t0 = time.perf_counter()
        K.ptau_contribute(p("pot0.ptau"), name="one", out=p("pot1.ptau"))
        chain["ptau-contribute"] = round(ms(t0), 1)
        os.remove(p("pot0.ptau"))
        t0 = time.perf_counter()
        K.ptau_prepare(p("pot1.ptau"), out=p("pot.ptau"))
        chain["ptau-prepare"] = round(ms(t0), 1)
        os.remove(p("pot1.ptau"))
        chain["prepared_ptau_bytes"] = os.path.getsize(p("pot.ptau"))
        t0 = time.perf_counter()
        h.new_zkey(p("pot.ptau"), out=p("chain0.zkey"))
        chain["zkey-new"] = round(ms(t0), 1)
        os.remove(p("pot.ptau"))
        t0 = time.perf_counter()
        K.zkey_contribute(p("chain0.zkey"), name="one", out=p("chain.zkey"))
        chain["zkey-contribute"] = round(ms(t0), 1)
        chain["total"] = round(ms(t_all), 1)
        os.remove(p("chain0.zkey"))
        verdicts.append(("chain zkey_check", K.zkey_check_file(p("chain.zkey"))[0]))
        os.remove(p("chain.zkey"))
        out["chain"] = chain
    h.close()
    out["unexpected_verdicts"] = [v for v in verdicts if not v[1]]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
