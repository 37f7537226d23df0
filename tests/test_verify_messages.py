"""Codes and messages of the three verifier entry points against tests/golden/verify_messages.json (built and recorded by
tests/verify_corpus.py): groth16_verify_json replays every case on the CPU; on the GPU each case goes through groth16_verify_batch and
groth16_verify_batch_combined as a batch of one."""
import pytest

import verify_corpus as VC
from conftest import load_golden


@pytest.fixture(scope="module")
def corpus(K, S):
    record = load_golden("verify_messages.json")["cases"]
    cases = VC.build(K, S)
    assert [c[0] for c in cases] == list(record), "tests/verify_corpus.py and the fixture list different cases"
    for name, a, b, v, kind in cases:
        assert VC.text_hash(a, b, v) == record[name]["sha256"], f"{name}: the corpus builder no longer makes the recorded text"
        assert kind == record[name]["kind"]
    return cases, record


def test_corpus_covers_every_code_and_kind(corpus):
    _, record = corpus
    assert {r["rc"] for r in record.values()} == {1, 0, -2, -3}
    assert {r["kind"] for r in record.values()} == {"item", "key", "key+item"}
    assert len({r["message"] for r in record.values()}) >= 11


def test_verify_json_replays_recorded_codes_and_messages(K, corpus):
    cases, record = corpus
    wrong = []
    for name, a, b, v, _ in cases:
        got = VC.run_json(K.lib(), a, b, v)
        want = [record[name]["rc"], record[name]["message"]]
        if got != want:
            wrong.append((name, got, want))
    assert not wrong, wrong


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["groth16_verify_batch", "groth16_verify_batch_combined"])
def test_batch_of_one_agrees_with_the_record(gpu, corpus, fn):
    """an item fault (or none) under a valid key: the call succeeds and the item's verdict is the recorded return value; a key
    fault: the call's code and message are the recorded ones"""
    cases, record = corpus
    wrong = []
    for name, a, b, v, kind in cases:
        rc, msg, verdict = VC.run_batch(gpu.lib(), fn, a, b, v)
        want = record[name]
        if kind == "item":
            if (rc, msg, verdict) != (0, "", want["rc"]):
                wrong.append((name, (rc, msg, verdict), want["rc"]))
        elif (rc, msg) != (want["rc"], want["message"]):
            wrong.append((name, (rc, msg), (want["rc"], want["message"])))
    assert not wrong, wrong
