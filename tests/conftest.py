"""pytest configuration: markers, import paths and shared fixtures.

`-m "not gpu"`  : oracle vs golden vectors, oracle vs oracle/_ref (when built), host logic, ABI checks — CPU only.
`-m gpu`        : parity tests proper — the HIP path (through the C ABI) against the oracle.
"""
import importlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with `-m gpu` on the GPU box)")


@pytest.fixture(scope="session")
def O():
    import oracle
    oracle.lib()
    return oracle


REF_CALLS = os.path.join(GOLDEN, "ref_calls.json")


def _canon(x):
    """JSON-able, type-tagged form of an argument or result of an oracle/_ref call"""
    if isinstance(x, np.ndarray):
        return ["nd", x.dtype.str, list(x.shape), np.ascontiguousarray(x).tobytes().hex()]
    if isinstance(x, (bool, np.bool_)):
        return ["b", bool(x)]
    if isinstance(x, (int, np.integer)):
        return ["i", hex(int(x))]
    if isinstance(x, str):
        return ["s", x]
    if isinstance(x, dict):
        return ["d", [[k, _canon(v)] for k, v in sorted(x.items())]]
    if isinstance(x, (list, tuple)):
        return ["l", [_canon(v) for v in x]]
    raise TypeError(f"cannot record a {type(x).__name__}")


def _uncanon(c):
    tag, v = c[0], c[1:]
    if tag == "nd":
        return np.frombuffer(bytes.fromhex(v[2]), dtype=np.dtype(v[0])).reshape(v[1]).copy()
    if tag == "b":
        return v[0]
    if tag == "i":
        return int(v[0], 16)
    if tag == "s":
        return v[0]
    if tag == "d":
        return {k: _uncanon(x) for k, x in v[0]}
    return [_uncanon(x) for x in v[0]]


def _call_key(name, args, kwargs):
    import hashlib
    blob = json.dumps([_canon(list(args)), _canon(dict(kwargs))], separators=(",", ":"))
    return f"{name}:{hashlib.sha256(blob.encode()).hexdigest()}"


class _RefRecorder:
    """oracle/_ref itself, every call's answer kept for tests/golden/ref_calls.json"""

    def __init__(self, ref):
        self._ref, self.calls = ref, {}

    def __getattr__(self, name):
        f = getattr(self._ref, name)

        def call(*args, **kwargs):
            out = f(*args, **kwargs)
            self.calls[_call_key(name, args, kwargs)] = _canon(out)
            return out
        return call

    def save(self, path):
        calls = dict(load_golden(os.path.basename(path))) if os.path.exists(path) else {}
        calls.update(self.calls)
        with open(path, "w") as f:
            json.dump(dict(sorted(calls.items())), f, indent=0)
            f.write("\n")


class _RefReplay:
    """the answers oracle/_ref gave to the same calls, recorded where it was built (tests/golden/ref_calls.json)"""

    def __init__(self, calls):
        self._calls = calls

    def __getattr__(self, name):
        def call(*args, **kwargs):
            k = _call_key(name, args, kwargs)
            if k not in self._calls:
                raise LookupError(f"ref.{name}(...) with these arguments is not in tests/golden/ref_calls.json: re-record it where "
                                  "oracle/_ref is built (ICICLE_SNARK_RECORD_REF=1 python -m pytest tests -m 'not gpu')")
            return _uncanon(self._calls[k])
        return call


@pytest.fixture(scope="session")
def R():
    """oracle/_ref — the reference's own sources, compiled by `make -C oracle ref` where the reference tree is present; everywhere
    else its recorded answers to the same calls (tests/golden/ref_calls.json), so that the tests need nothing outside the
    repository.  ICICLE_SNARK_RECORD_REF=1 with the live build records them again."""
    import ref
    if not ref.available():
        yield _RefReplay(load_golden(os.path.basename(REF_CALLS)))
    elif os.environ.get("ICICLE_SNARK_RECORD_REF") == "1":
        rec = _RefRecorder(ref)
        yield rec
        rec.save(REF_CALLS)
    else:
        yield ref


@pytest.fixture(scope="session")
def K():
    """the product package (ctypes mirror of the C ABI)"""
    return importlib.import_module("icicle-snark_amd")


@pytest.fixture(scope="session")
def S():
    return importlib.import_module("icicle-snark_amd.synth")


@pytest.fixture(scope="session")
def gpu(K):
    """selects HIP device 0 through the C ABI; fails loudly when there is no device"""
    K.set_device("HIP", 0)
    return K


def load_golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def unhex(h, *shape):
    a = np.frombuffer(bytes.fromhex(h), dtype=np.uint64).copy()
    return a.reshape(*shape) if shape else a


def unhex_int(h):
    return int.from_bytes(bytes.fromhex(h), "little")
