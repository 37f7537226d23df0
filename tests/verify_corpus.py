"""The inputs behind tests/golden/verify_messages.json: every text the verifier's tests feed to groth16_verify_json that is
malformed, not JSON, not canonical, off its curve, outside the subgroup, of the wrong length or tampered with (tests/test_verify.py,
test_edges of tests/test_gpu_verify_batch.py), the valid golden proofs beside them, key faults, null arguments, and inputs with two
independent faults.  Test infrastructure (tests/test_verify_messages.py replays it).

    python tests/verify_corpus.py --record      writes the fixture from the library of the tree this file lies in

The fixture pins (return value, groth16_verify_last_error() text) of groth16_verify_json for every case.  Cases with one fault in
the key and one in the proof or the signals are recorded from groth16_verify_batch instead (n = 1; a key fault ends that call before
it touches a device): the batch functions report the first fault in the order key → proof → public signals, and that order is the
contract of all three entry points.  A text is stored by its SHA-256 only, so a drift of this builder shows as a hash mismatch."""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "verify_messages.json")
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R_ORDER = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def build(K, S):
    """[(name, proof text | None, public text | None, key text | None, kind)], kind: "item" (the key is valid), "key" (the key is at
    fault, the item is not) or "key+item" (both are)"""
    from test_verify import _golden_vk_json
    from test_gpu_verify_batch import _g1_json, _g1_proj, _non_subgroup_twist_point
    g, vkj = _golden_vk_json(S)
    c0, c1 = g["cases"]
    proof, pub = c0["proof"], c0["public"]
    pj, qj = json.dumps(proof), json.dumps(pub)
    vk = json.loads(vkj)
    out = []

    def item(name, a, b, v=vkj):
        out.append((name, a, b, v, "item"))

    def tampered(**kw):
        return json.dumps(dict(json.loads(pj), **kw))

    def coord(field, *path, add):
        bad = json.loads(pj)
        at = bad[field]
        for k in path[:-1]:
            at = at[k]
        at[path[-1]] = str(add(int(at[path[-1]])))
        return json.dumps(bad)

    # ---- tests/test_verify.py ---------------------------------------------------------------------------------------------
    for k, c in enumerate(g["cases"]):
        a, b = json.dumps(c["proof"]), json.dumps(c["public"])
        item(f"valid {k}", a, b)
        item(f"signal + 1, case {k}", a, json.dumps([str(int(c["public"][0]) + 1)] + c["public"][1:]))
        item(f"A and C swapped, case {k}", json.dumps(dict(c["proof"], pi_a=c["proof"]["pi_c"][:2] + ["1"], pi_c=c["proof"]["pi_a"][:2] + ["1"])), b)
    item("proof 0 with the signals of case 1", pj, json.dumps(c1["public"]))
    item("proof text cut short", pj[:-5], qj)
    item("pi_a not a number", json.dumps({"pi_a": ["x", "1"], "pi_b": proof["pi_b"], "pi_c": proof["pi_c"]}), qj)
    item("no signals", pj, "[]")
    item("trailing white space", pj + " \n", qj)
    third = pj.index('"1"')
    put = lambda s: pj[:third] + s + pj[third + 3:]
    item("text after the proof", pj + "x", qj)
    item("text after the signals", pj, qj + "]")
    out.append(("text after the key", pj, qj, vkj + "{}", "key"))
    for name, s in (("bare token of high bytes", "\xff\xff"), ("bare 1e", "1e"), ("bare minus", "-"), ("bare nul", "nul"), ("control character in a string", '"1\x08"'),
                    ("non-ASCII bytes in a string", '"1\xc3\xa9"'), ("escape \\q", '"1\\q"'), ("escape \\u12g4", '"\\u12g4"'), ("number for a string", "1")):
        item(name + " in a coordinate that is not read", put(s), qj)
    item("signal as a bare number", pj, "[" + pub[0] + "]")
    item("escapes and literals in fields that are not read", pj[:-1] + ', "note": "a\\n\\u00e9\\"b", "flag": true, "n": -1.5e3, "z": null}', qj)
    item("signal + r", pj, json.dumps([str(int(pub[0]) + R_ORDER)] + pub[1:]))
    item("pi_a x + q", coord("pi_a", 0, add=lambda v: v + Q), qj)
    item("pi_c off the curve", coord("pi_c", 1, add=lambda v: (v + 1) % Q), qj)
    item("pi_a off the curve", coord("pi_a", 1, add=lambda v: (v + 1) % Q), qj)
    item("pi_b off the twist", coord("pi_b", 0, 0, add=lambda v: (v + 1) % Q), qj)
    item("pi_b outside the subgroup", tampered(pi_b=_non_subgroup_twist_point()), qj)
    item("nesting bomb as the proof", "[" * 100000 + "]" * 100000, qj)
    item("nesting bomb as the signals", pj, "[" * 100000)
    # ---- tests/test_gpu_verify_batch.py: test_edges, and the error kinds of its mixed batch ----------------------------------------
    folded = K.ec("g1", "ecadd", _g1_proj(K, vk["IC"][0]), K.ec("g1", "mul_scalar", _g1_proj(K, vk["IC"][1]), int(pub[0])))
    vk0j = json.dumps(dict(vk, IC=[_g1_json(K, folded)], nPublic=0))
    item("key without signals, no signals given", pj, "[]", vk0j)
    item("key without signals, one signal given", pj, qj, vk0j)
    item("identity A", tampered(pi_a=["0", "0", "0"]), qj)
    item("identity B", tampered(pi_b=[["0", "0"], ["0", "0"], ["0", "0"]]), qj)
    item("signal flipped", pj, json.dumps([str(int(pub[0]) ^ 1)] + pub[1:]))
    item("signals cut short", pj, "[1, 2")
    item("signal as a number", pj, json.dumps([int(pub[0])]))
    item("signal not decimal", pj, json.dumps(["12x"]))
    item("proof is an array", "[]", qj)
    item("signals are an object", pj, "{}")
    item("pi_c missing", json.dumps({k: v for k, v in proof.items() if k != "pi_c"}), qj)
    # two faults inside the item: the proof's comes first
    item("pi_b outside the subgroup and signal + r", tampered(pi_b=_non_subgroup_twist_point()), json.dumps([str(int(pub[0]) + R_ORDER)] + pub[1:]))
    item("pi_b outside the subgroup and no signals", tampered(pi_b=_non_subgroup_twist_point()), "[]")
    item("pi_c off the curve and signal as a number", coord("pi_c", 1, add=lambda v: (v + 1) % Q), json.dumps([int(pub[0])]))
    # ---- key faults -----------------------------------------------------------------------------------------------------------
    def vk_with(**kw):
        return json.dumps(dict(vk, **kw))

    def vk_coord(field, *path, add):
        bad = json.loads(vkj)
        at = bad[field]
        for k in path[:-1]:
            at = at[k]
        at[path[-1]] = str(add(int(at[path[-1]])))
        return json.dumps(bad)
    keys = [
        ("key text cut short", vkj[:-2]),
        ("key is an array", "[]"),
        ("nPublic is x", vk_with(nPublic="x")),
        ("nPublic negative", vk_with(nPublic=-1)),
        ("nPublic missing", json.dumps({k: v for k, v in vk.items() if k != "nPublic"})),
        ("IC missing", json.dumps({k: v for k, v in vk.items() if k != "IC"})),
        ("IC is a string", vk_with(IC="x")),
        ("IC shorter than nPublic + 1", vk_with(IC=vk["IC"][:1])),
        ("nPublic larger than IC", vk_with(nPublic=2)),
        ("IC[0] off the curve", vk_coord("IC", 0, 1, add=lambda v: (v + 1) % Q)),
        ("IC[1] off the curve", vk_coord("IC", 1, 1, add=lambda v: (v + 1) % Q)),
        ("IC[1] x + q", vk_coord("IC", 1, 0, add=lambda v: v + Q)),
        ("alpha off the curve", vk_coord("vk_alpha_1", 1, add=lambda v: (v + 1) % Q)),
        ("beta off the twist", vk_coord("vk_beta_2", 0, 0, add=lambda v: (v + 1) % Q)),
        ("gamma outside the subgroup", vk_with(vk_gamma_2=_non_subgroup_twist_point())),
        ("delta missing", json.dumps({k: v for k, v in vk.items() if k != "vk_delta_2"})),
    ]
    for name, v in keys:
        out.append((name, pj, qj, v, "key"))
    # ---- one fault in the key and one in the item: the key's is reported ---------------------------------------------------------
    bad_items = [("proof text cut short", pj[:-5], qj), ("pi_a off the curve", coord("pi_a", 1, add=lambda v: (v + 1) % Q), qj),
                 ("pi_b outside the subgroup", tampered(pi_b=_non_subgroup_twist_point()), qj), ("no signals", pj, "[]"),
                 ("signal + r", pj, json.dumps([str(int(pub[0]) + R_ORDER)] + pub[1:])), ("signal as a number", pj, json.dumps([int(pub[0])]))]
    for kname, v in (keys[0], keys[2], keys[5], keys[7], keys[10], keys[12], keys[14]):
        for iname, a, b in bad_items:
            out.append((f"{kname}; {iname}", a, b, v, "key+item"))
    # ---- null arguments ---------------------------------------------------------------------------------------------------------
    item("null proof", None, qj)
    item("null signals", pj, None)
    out.append(("null key", pj, qj, None, "key"))
    assert len({c[0] for c in out}) == len(out)
    return out


def _enc(s):
    return None if s is None else s.encode()


def text_hash(a, b, v):
    h = hashlib.sha256()
    for s in (a, b, v):
        h.update(b"\x00" if s is None else b"\x01" + s.encode() + b"\x02")
    return h.hexdigest()


def last_error(lib):
    lib.groth16_verify_last_error.restype = C.c_char_p
    return lib.groth16_verify_last_error().decode()


def run_json(lib, a, b, v):
    """(return value, message — "" for 0 / 1) of groth16_verify_json"""
    rc = lib.groth16_verify_json(_enc(a), _enc(b), _enc(v))
    return [rc, last_error(lib) if rc < 0 else ""]


def run_batch(lib, fn, a, b, v, device=b"HIP"):
    """one item through groth16_verify_batch / groth16_verify_batch_combined: (call's code, message — "" for 0, the item's verdict)"""
    pa, qa, out = (C.c_char_p * 1)(_enc(a)), (C.c_char_p * 1)(_enc(b)), (C.c_int32 * 1)(99)
    if fn == "groth16_verify_batch":
        rc = lib.groth16_verify_batch(pa, qa, C.c_int(1), _enc(v), device, out)
    else:
        rc = lib.groth16_verify_batch_combined(pa, qa, C.c_int(1), _enc(v), device, (C.c_uint8 * 32)(*range(32)), out, None)
    return [rc, last_error(lib) if rc != 0 else "", int(out[0])]


def record():
    import importlib
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    K = importlib.import_module("icicle-snark_amd")
    S = importlib.import_module("icicle-snark_amd.synth")
    cases = {}
    for name, a, b, v, kind in build(K, S):
        if kind == "key+item":
            rc, msg, _ = run_batch(K.lib(), "groth16_verify_batch", a, b, v)
            src = "groth16_verify_batch"
        else:
            rc, msg = run_json(K.lib(), a, b, v)
            src = "groth16_verify_json"
        cases[name] = {"kind": kind, "from": src, "rc": rc, "message": msg, "sha256": text_hash(a, b, v)}
    doc = {"about": "(return value, groth16_verify_last_error() text) per case of tests/verify_corpus.py, recorded from the library as it was before "
                    "groth16_verify_json became a caller of the batch parser.  `from` names the entry point that gave the record: cases of kind "
                    "key+item (one fault in the key, one in the item) come from groth16_verify_batch with n = 1, whose order key, proof, public "
                    "signals is the order all three entry points report in; every other case comes from groth16_verify_json itself.",
           "cases": cases}
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, indent=1, ensure_ascii=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {FIXTURE}")


if __name__ == "__main__":
    if "--record" in sys.argv:
        record()
