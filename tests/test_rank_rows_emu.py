"""The cases of the hand-written packed inverse RANK loop (tests/rank_rows_cases.py) on the execution-model emulator (CPU), which runs the C++
form of the same steps: the expectations (the oracle's inverse RANK, the streams, the coverage of the class pairs) are pinned here; the asm
itself is covered by the MI355X run in tests/test_rank_rows_gpu.py."""
import pytest


@pytest.fixture(scope="module")
def be():
    import parity_cases as P
    return P.EmuBackend()


def test_rank_rows_lengths(be):
    import rank_rows_cases as R
    R.check_inverse(be, [nm for nm, _r in R.length_cases()])


def test_rank_rows_class_pairs(be):
    import rank_rows_cases as R
    R.check_class_pairs_cover()
    R.check_inverse(be, ["class_pairs"])


def test_rank_rows_patterns(be):
    import rank_rows_cases as R
    R.check_inverse(be, [nm for nm, _r in R.P.rank_patterns()])


@pytest.mark.parametrize("cut", (False, True), ids=("whole", "cut_odd_rows"))
@pytest.mark.parametrize("bs", (1 << 14, 1 << 17), ids=("16k", "128k"))
def test_rank_rows_fused_chain(be, monkeypatch, bs, cut):
    import rank_rows_cases as R
    R.check_fused_chain(be, monkeypatch, bs, cut)
