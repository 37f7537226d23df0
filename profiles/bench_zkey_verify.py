"""groth16_zkey_verify_ptau on benchmark/1600k and a synthesised power-21 .ptau, beside groth16_zkey_check and
groth16_r1cs_match_zkey on the same key for scale.

    python profiles/bench_zkey_verify.py --make DIR                       synthesise c.zkey, w.wtns, c.r1cs and pot.ptau into DIR
    python profiles/bench_zkey_verify.py --dir DIR [--verify-only]        one process: the three checks, timed

The .ptau is written for this run only: the blocks the verify reads (block k of sections 12 to 15, block k + 1 of section 12) hold
the Lagrange values, every other block of those sections holds the identity, and sections 2 and 3 are left out (the reader demands
neither).  --verify-only runs the verify alone (for a run under rocprofv3 --kernel-trace --stats, which gives each kernel alone).
One JSON line per process.  profiles/zkey_verify_sweep.txt is the record.
"""
import argparse
import importlib
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def write_ptau_for_domain(K, S, bench, k, path):
    """a prepared .ptau of power k whose blocks for the domain 2^k (and 2^(k+1) in section 12) are real, vectorised as
    synth.setup_squaring_chain: [L_j(y)]_j = iNTT([y^i]_i)"""
    tau, alpha, beta = S.toxic_waste()[:3]
    vec = bench.GpuVec(K)
    to_mont = bench._to_mont(K)
    one = S.ints_to_arr([1])
    bcast = lambda x, cnt: np.broadcast_to(S.ints_to_arr([x]), (cnt, 4)).copy()

    def lagrange(size):
        K.release_domain()
        K.initialize_domain(K.get_root_of_unity(size))
        p, step, cnt = one.copy(), tau, 1
        while cnt < size:
            p = np.concatenate([p, vec.mul(p, bcast(step, cnt))])
            step = step * step % S.R_MOD
            cnt <<= 1
        out = vec.intt(p)
        K.release_domain()
        return out

    n = 1 << k
    L, L2 = lagrange(n), lagrange(2 * n)
    g1 = lambda sc: np.ascontiguousarray(to_mont(K.generator_mul("g1", np.ascontiguousarray(sc)))).tobytes()
    g2 = lambda sc: np.ascontiguousarray(to_mont(K.generator_mul("g2", np.ascontiguousarray(sc)))).tobytes()
    hdr = struct.pack("<I", 32) + S.Q_MOD.to_bytes(32, "little") + struct.pack("<II", k, k)
    small = [(1, hdr), (4, g1(S.ints_to_arr([alpha]))), (5, g1(S.ints_to_arr([beta]))), (6, g2(S.ints_to_arr([beta]))), (7, struct.pack("<I", 0))]
    with open(path, "wb") as f:
        f.write(b"ptau" + struct.pack("<II", 1, len(small) + 4))
        for sid, payload in small:
            f.write(struct.pack("<IQ", sid, len(payload)) + payload)
        zeros = lambda count, elem: f.write(bytes(1 << 20) * (count * elem >> 20) + bytes(count * elem & ((1 << 20) - 1)))
        f.write(struct.pack("<IQ", 12, (4 * n - 1) * 64))
        zeros(n - 1, 64)
        f.write(g1(L))
        f.write(g1(L2))
        f.write(struct.pack("<IQ", 13, (2 * n - 1) * 128))
        zeros(n - 1, 128)
        f.write(g2(L))
        for sid, factor in ((14, alpha), (15, beta)):
            f.write(struct.pack("<IQ", sid, (2 * n - 1) * 64))
            zeros(n - 1, 64)
            f.write(g1(vec.mul(L, bcast(factor, n))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make", default="")
    ap.add_argument("--dir", default="")
    ap.add_argument("--n", type=int, default=1600000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--verify-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    K = importlib.import_module("icicle-snark_amd")
    S = importlib.import_module("icicle-snark_amd.synth")
    K.set_device("HIP", 0)
    k = (a.n + 2 - 1).bit_length()                      # benchmark/<n>: n constraints, one public signal
    if a.make:
        import bench
        t0 = time.perf_counter()
        zkey, wtns = bench.make_inputs(K, S, a.n)
        open(os.path.join(a.make, "c.zkey"), "wb").write(zkey)
        open(os.path.join(a.make, "w.wtns"), "wb").write(wtns)      # (for profiles/bench_witness_check.py --dir: the prove path beside a parent build)
        open(os.path.join(a.make, "c.r1cs"), "wb").write(S.write_r1cs_squaring_chain(a.n))
        t1 = time.perf_counter()
        write_ptau_for_domain(K, S, bench, k, os.path.join(a.make, "pot.ptau"))
        print(json.dumps({"zkey_bytes": len(zkey), "ptau_bytes": os.path.getsize(os.path.join(a.make, "pot.ptau")), "domain_power": k,
                          "make_key_s": round(t1 - t0, 1), "make_ptau_s": round(time.perf_counter() - t1, 1)}), flush=True)
        return
    zp, rp, pp = (os.path.join(a.dir, x) for x in ("c.zkey", "c.r1cs", "pot.ptau"))
    out = {"n": a.n, "domain_power": k}
    info = K.ptau_info(pp, domain_power=k)
    out["ptau_power"] = info.power
    h = K.R1cs(rp)
    rows, verdicts = [], []
    for _ in range(a.runs + 1):
        t0 = time.perf_counter()
        ok, rep = h.verify_zkey(zp, pp)
        rows.append([round(ms(t0), 1), round(rep.upload_ms, 1), round(rep.device_ms, 1), round(rep.pairing_ms, 1),
                     round(rep.key.upload_ms, 1), round(rep.key.device_ms, 1), round(rep.key.pairing_ms, 1)])
        verdicts.append(("verify", ok, rep.kind, rep.failed_mask))
    out["columns"] = "wall, upload, device, pairing, then the embedded key check's upload, device, pairing (ms)"
    out["verify_first"] = rows[0]                       # the first call pays the process's first streams, staging and MSM workspaces
    out["verify"] = rows[1:]
    out["verify_wall_ms_median"] = round(statistics.median(r[0] for r in rows[1:]), 1)
    if not a.verify_only:
        zkey = open(zp, "rb").read()
        rows = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            ok, rep = K.zkey_check_file(zp)
            rows.append([round(ms(t0), 1), round(rep.upload_ms, 1), round(rep.device_ms, 1), round(rep.pairing_ms, 1)])
            verdicts.append(("zkey_check", ok, rep.kind, 0))
        out["zkey_check_wall_upload_device_pairing_ms"] = rows
        rows = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            ok, rep = h.match_zkey(zkey)
            rows.append([round(ms(t0), 1), round(rep.device_ms, 1)])
            verdicts.append(("match", ok, rep.kind, 0))
        out["match_wall_device_ms"] = rows
        # a key whose section 8 is another's: two points exchanged in a copy of the file
        bad = os.path.join(a.dir, "bad.zkey")
        image = bytearray(zkey)
        pos = 12
        for _ in range(struct.unpack_from("<I", image, 8)[0]):
            sid, ln = struct.unpack_from("<IQ", image, pos)
            if sid == 8:
                image[pos + 12:pos + 76], image[pos + 76:pos + 140] = image[pos + 76:pos + 140], image[pos + 12:pos + 76]
            pos += 12 + ln
        open(bad, "wb").write(image)
        t0 = time.perf_counter()
        ok, rep = h.verify_zkey(bad, pp)
        out["verify_swapped_c_wall_ms_kind_mask"] = [round(ms(t0), 1), rep.kind, rep.failed_mask]
        verdicts.append(("swapped C refused", (not ok) and rep.kind == K.VERIFY_C, rep.kind, rep.failed_mask))
        os.remove(bad)
    h.close()
    out["unexpected_verdicts"] = [v for v in verdicts if not v[1]]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
