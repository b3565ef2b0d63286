"""The cases of the order-1 rANS decoder's hand-written loop (tests/ans1_loop_cases.py) on the execution-model emulator (CPU). The emulator runs
the compiler's loop whichever form is asked for, so this file pins the expectations (the oracle's streams, the lengths, the phases of the
alternation) and the C++ step that the default form leaves a tile's last steps to; the asm itself is covered by the MI355X run in
tests/test_ans1_loop_gpu.py."""
import pytest

import ans1_loop_cases as A


@pytest.fixture(scope="module")
def be():
    return A.P.EmuBackend()


def test_ans1_loop_case_lengths():
    assert [len(d) >> 2 for _nm, d in A.length_cases()][::4] == list(A.Q_EDGES)
    assert [len(d) & 3 for _nm, d in A.length_cases()] == [0, 1, 2, 3] * len(A.Q_EDGES)
    assert all(len(d) == 4 * A.DATA_STEPS + 3 for _nm, d in A.data_cases())
    assert len(A.two_chunk_case()) == (4 << 20) + 4099
    A.check_alternation_phases()


def test_ans1_loop_lengths(be, monkeypatch):
    A.check_lengths(be, monkeypatch, "default")


@pytest.mark.parametrize("name", [nm for nm, _d in A.data_cases()])
def test_ans1_loop_data(be, monkeypatch, name):
    A.check_data(be, monkeypatch, "default", name)


def test_ans1_loop_two_chunks():
    """a million steps take the emulator most of a minute: here the expectation alone is pinned (the oracle's stream of the two chunks decodes to
    the input in the oracle, and holds two chunks' worth of payload); the device run is test_ans1_loop_two_chunks_gpu"""
    data = A.two_chunk_case()
    stream = A.oracle_stream("two_chunks", "", "NONE", 8 << 20)
    assert len(data) == A.CHUNK + 4099 and len(stream) < len(data)
    assert A.O.decompress(stream, len(data) + 64) == data


@pytest.mark.parametrize("two_groups", (False, True), ids=("default_groups", "two_groups"))
@pytest.mark.parametrize("bs", (1 << 14, 1 << 17), ids=("16k", "128k"))
def test_ans1_loop_fused_chain(be, monkeypatch, bs, two_groups):
    A.check_fused_chain(be, monkeypatch, "default", bs, two_groups)
