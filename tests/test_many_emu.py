"""knz_dev_compress_many / knz_dev_decompress_many on the execution-model emulator (CPU): every stream of a many call against the single
calls of the same library and against the reference's Writer / Reader (oracle/_ref through tests/ref_lib.py). The same cases run on the
MI355X in tests/test_many_gpu.py."""
import pytest


@pytest.fixture(scope="module")
def be():
    import parity_cases as P
    return P.EmuBackend()


def test_many_coverage_guard():
    import many_cases as M
    M.check_coverage()


def test_many_api(be):
    import many_cases as M
    M.check_api(be)


@pytest.mark.parametrize("bs", (1024, 1 << 14))
@pytest.mark.parametrize("pipe", range(7))
def test_many_shapes(be, monkeypatch, pipe, bs):
    import many_cases as M
    M.check_shapes(be, M.PIPELINES[pipe], bs, monkeypatch)


@pytest.mark.parametrize("k", (1, 2, 37))
def test_many_k(be, k):
    import many_cases as M
    M.check_k(be, M.PIPELINES[k % 3], 1024, k)


def test_many_group_limit(be):
    import many_cases as M
    M.check_group_limit(be, singles=())


def test_many_one_batch(be):
    import many_cases as M
    M.check_one_batch(be)


@pytest.mark.parametrize("pipe", (0, 2))
def test_many_mixed_trouble(be, pipe):
    import many_cases as M
    M.check_mixed_trouble(be, M.PIPELINES[pipe])


@pytest.mark.parametrize("pipe", (0, 2))
def test_many_small_destination(be, pipe):
    import many_cases as M
    M.check_small_destination(be, M.PIPELINES[pipe], sweep=pipe == 0)


def test_many_short_inner_block(be):
    import many_cases as M
    M.check_short_inner(be)


def test_many_lanes(be):
    import many_cases as M
    M.check_lanes(be)


def test_many_alloc_split(be, monkeypatch):
    import many_cases as M
    M.check_alloc_split(be, monkeypatch)
