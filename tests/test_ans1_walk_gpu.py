"""The walk of the order-1 rANS chunk headers (huffman_dec.hip, knz_ans1_walk_header) on the MI355X: the cases of tests/ans1_walk_cases.py as round
trips against the oracle under the default form and under KNZ_ANS1_WALK_PLAIN (the generic reader's walk), and the damaged headers, which must
end in the same code under both. The emulator run (test_ans1_walk_emu.py) pins what the headers hold."""
import pytest

import ans1_walk_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return W.P.GpuBackend()


@pytest.mark.parametrize("form", W.FORMS)
@pytest.mark.parametrize("name", [nm for nm, _d in W.shaped_cases()])
def test_ans1_walk_shaped_gpu(be, monkeypatch, name, form):
    W.round_trip(be, monkeypatch, form, name)


@pytest.mark.parametrize("form", W.FORMS)
def test_ans1_walk_offsets_gpu(be, monkeypatch, form):
    for name, _d in W.offset_cases():
        W.round_trip(be, monkeypatch, form, name)


@pytest.mark.parametrize("form", W.FORMS)
@pytest.mark.parametrize("name", [nm for nm, _d in W.chain_cases()])
def test_ans1_walk_chain_gpu(be, monkeypatch, name, form):
    W.round_trip(be, monkeypatch, form, name)


@pytest.mark.parametrize("form", W.FORMS)
def test_ans1_walk_two_chunks_gpu(be, monkeypatch, form):
    W.round_trip(be, monkeypatch, form, "two_chunks")


@pytest.mark.parametrize("name", [nm for nm, _s in W.damaged_streams()])
def test_ans1_walk_damaged_gpu(be, monkeypatch, name):
    W.check_damaged(be, monkeypatch, name)
