"""The cases of the walk of the order-1 rANS chunk headers (tests/ans1_walk_cases.py) on the execution-model emulator (CPU): the walk is plain C++
over the wave primitives, so the emulator runs the very code the MI355X runs (tests/test_ans1_walk_gpu.py), under its schedules, next to
the generic reader's walk (KNZ_ANS1_WALK_PLAIN). This file also pins the expectations: what the oracle's headers hold, where they start."""
import pytest

import ans1_walk_cases as W


@pytest.fixture(scope="module")
def be():
    return W.P.EmuBackend()


def test_ans1_walk_header_shapes():
    W.check_shapes()


def test_ans1_walk_offsets_cover_a_word():
    assert len(W.offset_cases()) >= 1
    for _name, data in W.offset_cases():
        assert 2 * W.OFFSET_BS < len(data) <= 3 * W.OFFSET_BS          # three blocks


@pytest.mark.parametrize("form", W.FORMS)
@pytest.mark.parametrize("name", [nm for nm, _d in W.shaped_cases()])
def test_ans1_walk_shaped(be, monkeypatch, name, form):
    W.round_trip(be, monkeypatch, form, name)


@pytest.mark.parametrize("form", W.FORMS)
def test_ans1_walk_offsets(be, monkeypatch, form):
    for name, _d in W.offset_cases():
        W.round_trip(be, monkeypatch, form, name)


@pytest.mark.parametrize("form", W.FORMS)
@pytest.mark.parametrize("name", [nm for nm, _d in W.chain_cases()])
def test_ans1_walk_chain(be, monkeypatch, name, form):
    W.round_trip(be, monkeypatch, form, name)


def test_ans1_walk_two_chunks():
    """a million coding steps take the emulator most of a minute: here the expectation alone is pinned (the oracle's stream of the two chunks decodes to
    the input in the oracle); the device run is test_ans1_walk_two_chunks_gpu"""
    data = W.two_chunk_case()
    stream = W.oracle_stream("two_chunks")
    assert len(data) == W.CHUNK + 4099 and len(stream) < len(data)
    assert W.O.decompress(stream, len(data) + 64) == data


@pytest.mark.parametrize("name", [nm for nm, _s in W.damaged_streams()])
def test_ans1_walk_damaged(be, monkeypatch, name):
    W.check_damaged(be, monkeypatch, name)
