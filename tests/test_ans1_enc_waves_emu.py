"""The cases of the two-wave order-1 rANS encoder (tests/ans1_enc_waves_cases.py) on the execution-model emulator (CPU). The emulator build has the
same two waves, the same ring and the same counts around the C++ step, so the hand-over runs here under the emulator's three orders of the threads
of a workgroup; the hand-written step itself is covered by the MI355X run (tests/test_ans1_enc_waves_gpu.py). This file also pins the
expectations (the lengths, the oracle's streams)."""
import pytest

import ans1_enc_waves_cases as W


@pytest.fixture(scope="module")
def be():
    return W.P.EmuBackend()


@pytest.fixture(params=("fwd", "rev", "rand"))
def sched(request, monkeypatch):
    monkeypatch.setenv("KNZ_EMU_SCHED", request.param)              # thread order inside a workgroup: which wave runs ahead
    return request.param


def test_ans1_enc_waves_case_shapes():
    W.check_case_shapes()


def test_ans1_enc_waves_lengths(be, monkeypatch, sched):
    W.round_trips(be, monkeypatch, "default", W.LENGTH_NAMES)


def test_ans1_enc_waves_lengths_one_wave(be, monkeypatch):
    W.round_trips(be, monkeypatch, "KNZ_ANS1_ENC_ONE_WAVE", W.LENGTH_NAMES)


@pytest.mark.parametrize("name", W.DATA_NAMES)
def test_ans1_enc_waves_data(be, monkeypatch, sched, name):
    W.round_trips(be, monkeypatch, "default", (name,))


@pytest.mark.parametrize("name", W.DATA_NAMES)
def test_ans1_enc_waves_data_one_wave(be, monkeypatch, name):
    W.round_trips(be, monkeypatch, "KNZ_ANS1_ENC_ONE_WAVE", (name,))


@pytest.mark.parametrize("form", W.FORMS)
def test_ans1_enc_waves_chain(be, monkeypatch, form):
    W.round_trips(be, monkeypatch, form, ("chain",))


@pytest.mark.parametrize("form", W.FORMS)
def test_ans1_enc_waves_group_blocks(be, monkeypatch, form):
    W.round_trips(be, monkeypatch, form, ("blocks",), group_blocks=True)


def test_ans1_enc_waves_two_chunks():
    """a million steps take the emulator most of a minute: here the expectation alone is pinned (the oracle's stream of the two chunks decodes to the
    input in the oracle); the device run is test_ans1_enc_waves_two_chunks_gpu"""
    data = W.cases()["two_chunks"][0]
    stream = W.oracle_stream("two_chunks")
    assert len(stream) < len(data) and W.O.decompress(stream, len(data) + 64) == data
