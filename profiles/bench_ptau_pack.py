"""groth16_ptau_pack and groth16_ptau_unpack file to file, beside groth16_ptau_verify's stage trace on the same files.

    python profiles/bench_ptau_pack.py --make DIR --power P [--prepared]   the input into DIR: groth16_ptau_new's file, one contribution
                                                                           with secrets from the operating system (so its points are
                                                                           general ones), and with --prepared groth16_ptau_prepare of it
    python profiles/bench_ptau_pack.py --dir DIR --power P [--prepared]    one process: pack (DIR/pot_P[_prepared].ptau → .ptaz) and
                                                                           unpack (.ptaz → _back.ptau), each --runs + 1 times through the
                                                                           _file entries; the last unpacked file compared with the input
    python profiles/bench_ptau_pack.py --dir DIR --power P [--prepared] --verify   one process: groth16_ptau_verify_file on the input,
                                                                           --runs + 1 times (ICICLE_SNARK_TRACE_PTAU_VERIFY=1 prints its
                                                                           stages on stderr: "pair S: up, lane tests" is the yardstick)

Per direction the JSON line holds wall, upload, device, download and write time per run, the bytes in and out, and the device time
per point of the last run, and for sections 2 (G1) and 3 (G2) alone — through groth16_points_pack / _unpack, one kernel each — the
point count and the device time per point.  device is the wall time of the device part without the uploads: the four (eight) sections' kernels, G1
and G2 together; ICICLE_SNARK_TRACE_PTAU_PACK=1 prints the stages on stderr.  One JSON line per process.
profiles/ptau_pack_sweep.txt is the record.
"""
import argparse
import importlib
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def section(path, sid):
    """the payload of section sid of a .ptau or a packed file"""
    with open(path, "rb") as f:
        nsec = struct.unpack("<I", f.read(12)[8:])[0]
        for _ in range(nsec):
            s, ln = struct.unpack("<IQ", f.read(12))
            if s == sid:
                return f.read(ln)
            f.seek(ln, 1)
    raise KeyError(sid)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make", default="")
    ap.add_argument("--dir", default="")
    ap.add_argument("--power", type=int, default=12)
    ap.add_argument("--prepared", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--verify", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    K = importlib.import_module("icicle-snark_amd")
    K.set_device("HIP", 0)
    stem = os.path.join(a.make or a.dir, "pot_%d%s" % (a.power, "_prepared" if a.prepared else ""))
    src, packed, back = stem + ".ptau", stem + ".ptaz", stem + "_back.ptau"
    if a.make:
        t0 = time.perf_counter()
        new, plain = stem + "_0000.tmp", os.path.join(a.make, "pot_%d.ptau" % a.power)
        K.ptau_new(a.power, out=new)
        K.ptau_contribute(new, out=plain, name="bench")
        os.unlink(new)
        if a.prepared:
            K.ptau_prepare(plain, out=src)
        print(json.dumps({"power": a.power, "prepared": a.prepared, "ptau_bytes": os.path.getsize(src), "make_ms": round(ms(t0), 1)}), flush=True)
        return
    out = {"power": a.power, "prepared": a.prepared, "input": os.path.basename(src)}
    if a.verify:
        rows = []
        for _ in range(a.runs + 1):
            t0 = time.perf_counter()
            ok, rep = K.ptau_verify(src)
            rows.append([round(ms(t0), 1), round(rep.upload_ms, 1), round(rep.device_ms, 1), round(rep.pairing_ms, 1)])
        out.update({"columns": "wall, upload, device, pairing (ms)", "verify": rows, "ok": ok})
        print(json.dumps(out), flush=True)
        return
    out["columns"] = "wall, upload, device, download, write (ms)"
    for what, call, i, o in (("pack", K.ptau_pack, src, packed), ("unpack", K.ptau_unpack, packed, back)):
        rows = []
        for _ in range(a.runs + 1):
            t0 = time.perf_counter()
            _, rep = call(i, out=o)
            rows.append([round(ms(t0), 1), round(rep.upload_ms, 1), round(rep.device_ms, 1), round(rep.download_ms, 1), round(rep.write_ms, 1)])
        out[what] = rows
        out[what + "_bytes"] = [rep.in_bytes, rep.out_bytes]
        out[what + "_device_ns_per_point"] = round(rep.device_ms * 1e6 / (rep.points[0] + rep.points[1]), 1)
    out["points"] = list(rep.points)
    # per group: sections 2 (G1) and 3 (G2) alone through the raw entries, whose device time is one kernel's
    for what, call, path in (("pack", K.points_pack, src), ("unpack", K.points_unpack, packed)):
        for sid, g2 in ((2, False), (3, True)):
            buf = section(path, sid)
            for _ in range(2):
                _, rep = call(buf, g2=g2)
            out["%s_%s_device_ns_per_point" % (what, "g2" if g2 else "g1")] = [rep.n, round(rep.device_ms * 1e6 / rep.n, 1)]
    with open(src, "rb") as f, open(back, "rb") as g:
        same = True
        while same:
            x, y = f.read(1 << 24), g.read(1 << 24)
            same = x == y
            if not x:
                break
    out["round_trip_equal"] = same
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
