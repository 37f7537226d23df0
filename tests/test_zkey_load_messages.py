"""Codes and messages of the zkey loader against tests/golden/zkey_load_messages.json (built and recorded by tests/zkey_corpus.py).
The container and the header are validated before a device is touched, so groth16_cache_load, groth16_cache_load_file and
groth16_zkey_export_vk replay every malformed key on the CPU.  groth16_prove selects its device before it opens the key (without a
GPU it fails there, whatever the key): its file route — the cold route — replays the cases on the GPU, where the keys the parser
must keep accepting also load and prove."""
import base64
import json

import pytest

import zkey_corpus as ZC
from conftest import load_golden


@pytest.fixture(scope="module")
def corpus():
    doc = load_golden("zkey_load_messages.json")
    cases, ic_cases = ZC.build(), ZC.build_ic()
    for built, record in ((cases, doc["load"]), (ic_cases, doc["export_vk"])):
        assert [n for n, _ in built] == list(record), "tests/zkey_corpus.py and the fixture list different cases"
        for name, z in built:
            assert ZC.sha(z) == record[name]["sha256"], f"{name}: the corpus builder no longer makes the recorded key"
    return cases, doc["load"], ic_cases, doc["export_vk"]


def _want(record, name):
    return [record[name]["rc"], record[name]["message"]]


def test_corpus_covers_the_faults(corpus):
    cases, record, _, ic_record = corpus
    names = [n for n, _ in cases]
    for sid in ZC.LOADER_SECTIONS:
        assert f"section {sid} missing" in names and f"section {sid} duplicated" in names
    assert {r["rc"] for r in record.values()} == {-2} and {r["rc"] for r in ic_record.values()} == {-2}
    assert len({r["message"] for r in record.values()}) >= 24
    # the two-fault cases report the fault the order of checks meets first
    assert record["section 5 missing and n8q 31"]["message"] == record["section 5 missing"]["message"]
    assert record["section 9 duplicated and domain 6"]["message"] == record["section 9 duplicated"]["message"]
    assert record["wrong q and section 7 one point short"]["message"] == record["wrong q"]["message"]


def test_cache_load_replays_recorded_codes_and_messages(K, corpus):
    cases, record, _, _ = corpus
    wrong = [(name, got, _want(record, name)) for name, z in cases for got in [ZC.run_load(K.lib(), z)] if got != _want(record, name)]
    assert not wrong, wrong


def test_cache_load_file_replays_recorded_codes_and_messages(K, corpus, tmp_path):
    cases, record, _, _ = corpus
    wrong = []
    for k, (name, z) in enumerate(cases):
        p = tmp_path / f"{k}.zkey"
        p.write_bytes(z)
        got = ZC.run_load_file(K.lib(), str(p))
        if got != _want(record, name):
            wrong.append((name, got, _want(record, name)))
    assert not wrong, wrong


def test_export_vk_answers_as_the_loader_does(K, corpus):
    """one parser: every key the loader refuses, the export refuses with the same code and text"""
    cases, record, _, _ = corpus
    wrong = [(name, got, _want(record, name)) for name, z in cases for got in [ZC.run_export_vk(K.lib(), z)] if got != _want(record, name)]
    assert not wrong, wrong


def test_export_vk_reports_section_3_which_the_loader_does_not_read(K, corpus):
    _, _, ic_cases, ic_record = corpus
    assert ic_record["section 3 missing"]["message"] == "Missing section 3"
    for name, z in ic_cases:
        assert ZC.run_export_vk(K.lib(), z) == _want(ic_record, name), name


@pytest.fixture(scope="module")
def golden_files(tmp_path_factory):
    g = load_golden("groth16.json")
    d = tmp_path_factory.mktemp("zkey_messages")
    w = d / "golden.wtns"
    w.write_bytes(base64.b64decode(g["wtns"]))
    return g, d, w


@pytest.mark.gpu
def test_prove_from_files_replays_recorded_codes_and_messages(gpu, corpus, golden_files):
    """groth16_prove on a key that is not cached — the cold route — gives a malformed key the loader's code and text"""
    cases, record, _, _ = corpus
    _, d, w = golden_files
    wrong = []
    for k, (name, z) in enumerate(cases):
        p = d / f"bad{k}.zkey"
        p.write_bytes(z)
        got = ZC.run_prove(gpu.lib(), str(p), str(w), str(d))
        if got != _want(record, name):
            wrong.append((name, got, _want(record, name)))
    assert not wrong, wrong


@pytest.mark.gpu
@pytest.mark.parametrize("variant", range(3))
def test_accepted_variants_load_and_prove(gpu, S, golden_files, variant):
    """section 3 removed, unknown sections appended, a wrong declared coefficient count (it is not read): the key loads through
    groth16_cache_load and through the cold groth16_prove, and both proofs verify under the golden verification key"""
    from test_verify import _golden_vk_json
    K = gpu
    g, d, w = golden_files
    _, vkj = _golden_vk_json(S)
    name, z = ZC.accepted_variants()[variant]
    public = g["cases"][0]["public"]
    cm = K.CacheManager()
    try:
        cm.load(name, z)
        pj, qj, _ = cm.prove_mem(name, base64.b64decode(g["wtns"]))
        assert json.loads(qj) == public, name
        assert K.groth16_verify_json(pj, qj, vkj) is True, name
        zp, pp, qp = d / f"variant{variant}.zkey", d / f"proof{variant}.json", d / f"public{variant}.json"
        zp.write_bytes(z)
        assert not cm.contains(f"{zp}_HIP")
        cm.prove_files(str(w), str(zp), str(pp), str(qp))                 # nothing cached: the cold route
        assert cm.contains(f"{zp}_HIP")
        assert json.loads(qp.read_text()) == public, name
        assert K.groth16_verify_json(pp.read_text(), qp.read_text(), vkj) is True, name
    finally:
        cm.close()
    K.release_domain()
