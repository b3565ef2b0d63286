"""The hand-written loop of the order-1 rANS decoder (ans1.hip, knz_ans1_decode_lds2_kernel) on the MI355X: the cases of tests/ans1_loop_cases.py
as round trips against the oracle under each form of the loop: the default (sixteen steps a turn), round 5's (KNZ_ANS1_R5_LOOP), the compiler's
(KNZ_ANS1_PLAIN) and round 4's (KNZ_ANS1_LOHI_LDS). This run is what covers the asm; the emulator run (test_ans1_loop_emu.py) pins the same
expectations on the compiler's loop."""
import pytest

import ans1_loop_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return A.P.GpuBackend()


@pytest.mark.parametrize("form", A.FORMS)
def test_ans1_loop_lengths_gpu(be, monkeypatch, form):
    A.check_lengths(be, monkeypatch, form)


@pytest.mark.parametrize("name", [nm for nm, _d in A.data_cases()])
@pytest.mark.parametrize("form", A.FORMS)
def test_ans1_loop_data_gpu(be, monkeypatch, form, name):
    if name == "alternation":
        A.check_alternation_phases()
    A.check_data(be, monkeypatch, form, name)


@pytest.mark.parametrize("form", A.FORMS)
def test_ans1_loop_two_chunks_gpu(be, monkeypatch, form):
    A.check_two_chunks(be, monkeypatch, form)


@pytest.mark.parametrize("two_groups", (False, True), ids=("default_groups", "two_groups"))
@pytest.mark.parametrize("bs", (1 << 14, 1 << 17), ids=("16k", "128k"))
@pytest.mark.parametrize("form", A.FORMS)
def test_ans1_loop_fused_chain_gpu(be, monkeypatch, form, bs, two_groups):
    A.check_fused_chain(be, monkeypatch, form, bs, two_groups)
