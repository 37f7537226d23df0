"""groth16_zkey_contribute on benchmark/1600k: 1.6 M points of section 8 and 2.1 M of section 9 times one full-width scalar.

    python profiles/bench_zkey_contribute.py --make DIR                     synthesise benchmark/<n>'s key into DIR/key.zkey (bench.py's)
    python profiles/bench_zkey_contribute.py --dir DIR [--contribute-only]  one process: the contribution timed (the _file entry,
                                                                            DIR/key.zkey → DIR/out.zkey), then the written key through
                                                                            groth16_zkey_check and groth16_zkey_contributions
    python profiles/bench_zkey_contribute.py --dir DIR --compare            also: sections 1 to 9 of out.zkey against the synthesiser's key
                                                                            for δ·δ′, byte for byte (synthesises a second key)

--contribute-only contributes once and does nothing else (for a run under rocprofv3 --kernel-trace --stats, alone: no counters in
the same run).  The synthesised key has γ, δ ≠ 1, so groth16_zkey_contributions must answer POK at record 1 (the chain does not
start from groth16_zkey_new's key): the script reports the verdict, it does not judge it.  One JSON line per process.
profiles/zkey_contribute_sweep.txt is the record.
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECRET = bytes(range(7, 39))
TAG = b"icicle-snark zkey contribution v1"
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def delta_of(secret):
    import hashlib
    sha = lambda x: hashlib.sha256(x).digest()
    return int.from_bytes(sha(secret + TAG + b"\0") + sha(secret + TAG + b"\1"), "big") % R


def sections(image):
    import struct
    pos, out = 12, {}
    for _ in range(struct.unpack_from("<I", image, 8)[0]):
        sid, ln = struct.unpack_from("<IQ", image, pos)
        out[sid] = (pos + 12, ln)
        pos += 12 + ln
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make", default="")
    ap.add_argument("--dir", default="")
    ap.add_argument("--n", type=int, default=1600000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--contribute-only", action="store_true")
    ap.add_argument("--compare", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    K = importlib.import_module("icicle-snark_amd")
    S = importlib.import_module("icicle-snark_amd.synth")
    K.set_device("HIP", 0)
    import bench
    if a.make:
        t0 = time.perf_counter()
        zkey, _ = bench.make_inputs(K, S, a.n)
        open(os.path.join(a.make, "key.zkey"), "wb").write(zkey)
        print(json.dumps({"zkey_bytes": len(zkey), "make_s": round(time.perf_counter() - t0, 1)}), flush=True)
        return
    src, dst = os.path.join(a.dir, "key.zkey"), os.path.join(a.dir, "out.zkey")
    out = {"n": a.n, "columns": "wall, upload, device, download, write (ms)"}
    rows = []
    for _ in range(1 if a.contribute_only else a.runs + 1):
        t0 = time.perf_counter()
        _, rep = K.zkey_contribute(src, secret=SECRET, name="bench", out=dst)
        rows.append([round(ms(t0), 1), round(rep.upload_ms, 1), round(rep.device_ms, 1), round(rep.download_ms, 1), round(rep.write_ms, 1)])
    out["contribute"] = rows
    out["sizes"] = {"points_c": rep.points_c, "points_h": rep.points_h, "zkey_bytes": rep.zkey_bytes, "contribution": rep.contribution}
    if not a.contribute_only:
        got = open(dst, "rb").read()
        t0 = time.perf_counter()
        ok, crep = K.zkey_check(got)
        out["zkey_check_ok_kind_wall_ms"] = [ok, crep.kind, round(ms(t0), 1)]
        t0 = time.perf_counter()
        ok, arep = K.zkey_contributions(got)
        out["contributions_ok_count_kind_index_wall_ms"] = [ok, arep.count, arep.kind, arep.index, round(ms(t0), 1)]
        if a.compare:
            tau, alpha, beta, gamma, delta = S.toxic_waste()
            toxic = (tau, alpha, beta, gamma, delta * delta_of(SECRET) % R)
            S._toxic = lambda seed: toxic                 # setup_squaring_chain draws its toxic waste from here
            t0 = time.perf_counter()
            want, _ = bench.make_inputs(K, S, a.n)
            sg, sw = sections(got), sections(want)
            out["sections_equal_to_the_synthesisers"] = {s: got[sg[s][0]:sg[s][0] + sg[s][1]] == want[sw[s][0]:sw[s][0] + sw[s][1]] for s in range(1, 10)}
            out["compare_s"] = round(time.perf_counter() - t0, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
