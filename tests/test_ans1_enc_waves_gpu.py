"""The two-wave order-1 rANS encoder (ans1.hip, knz_ans1_encode_asm_kernel) on the MI355X: the cases of tests/ans1_enc_waves_cases.py as round trips
against the oracle under the default form (a coding wave and a placing wave) and under KNZ_ANS1_ENC_ONE_WAVE (the one-wave kernel). This run is
what covers the hand-written step inside the two-wave kernel; the emulator run (test_ans1_enc_waves_emu.py) pins the same expectations."""
import pytest

import ans1_enc_waves_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return W.P.GpuBackend()


@pytest.mark.parametrize("form", W.FORMS)
def test_ans1_enc_waves_lengths_gpu(be, monkeypatch, form):
    W.round_trips(be, monkeypatch, form, W.LENGTH_NAMES)


@pytest.mark.parametrize("name", W.DATA_NAMES)
@pytest.mark.parametrize("form", W.FORMS)
def test_ans1_enc_waves_data_gpu(be, monkeypatch, form, name):
    W.round_trips(be, monkeypatch, form, (name,))


@pytest.mark.parametrize("form", W.FORMS)
def test_ans1_enc_waves_two_chunks_gpu(be, monkeypatch, form):
    W.round_trips(be, monkeypatch, form, ("two_chunks",))


@pytest.mark.parametrize("form", W.FORMS)
def test_ans1_enc_waves_chain_gpu(be, monkeypatch, form):
    W.round_trips(be, monkeypatch, form, ("chain",))


@pytest.mark.parametrize("form", W.FORMS)
def test_ans1_enc_waves_group_blocks_gpu(be, monkeypatch, form):
    W.round_trips(be, monkeypatch, form, ("blocks",), group_blocks=True)
