"""The hand-written packed inverse RANK loop (rank_inv_asm.h) on the MI355X: the standalone chain kernel and the fused ZRLT / RANK chain against the
oracle's inverse RANK, on the sequences of tests/rank_rows_cases.py. This run is what covers the asm; the emulator run (test_rank_rows_emu.py)
pins the same expectations on the C++ form of the steps."""
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import parity_cases as P
    return P.GpuBackend()


def test_rank_rows_lengths_gpu(be):
    import rank_rows_cases as R
    R.check_inverse(be, [nm for nm, _r in R.length_cases()])


def test_rank_rows_class_pairs_gpu(be):
    import rank_rows_cases as R
    R.check_class_pairs_cover()
    R.check_inverse(be, ["class_pairs"])


def test_rank_rows_patterns_gpu(be):
    import rank_rows_cases as R
    R.check_inverse(be, [nm for nm, _r in R.P.rank_patterns()])


@pytest.mark.parametrize("cut", (False, True), ids=("whole", "cut_odd_rows"))
@pytest.mark.parametrize("bs", (1 << 14, 1 << 17), ids=("16k", "128k"))
def test_rank_rows_fused_chain_gpu(be, monkeypatch, bs, cut):
    import rank_rows_cases as R
    R.check_fused_chain(be, monkeypatch, bs, cut)
