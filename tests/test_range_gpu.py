"""knz_dev_stream_index / knz_dev_decompress_range / knz_dev_decompress_many_range on the MI355X: the index against a framing walk in plain
Python, every range against the slice of the reference Reader's bytes (oracle/_ref through tests/ref_lib.py), the many form against the single
calls. The cases of tests/test_range_emu.py, here at every block size of the table and on a stream of 1 500 blocks."""
import pytest

import range_cases as RC

pytestmark = pytest.mark.gpu
SIZES = RC.BLOCK_SIZES


@pytest.fixture(scope="module")
def be():
    import parity_cases as P
    return P.GpuBackend()


def test_range_coverage_guard_gpu():
    RC.check_coverage()


@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("pipe", RC.PIPELINES, ids=RC.pipe_id)
def test_range_index_gpu(be, pipe, bs):
    RC.check_index(be, pipe, bs)


@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("pipe", RC.PIPELINES, ids=RC.pipe_id)
def test_range_is_slice_gpu(be, pipe, bs):
    RC.check_ranges(be, pipe, bs, RC.main_stream(pipe, bs))


@pytest.mark.parametrize("n", (1, 0), ids=("one-block", "empty"))
@pytest.mark.parametrize("pipe", RC.PIPELINES, ids=RC.pipe_id)
def test_range_small_streams_gpu(be, pipe, n):
    for bs in SIZES:
        RC.check_ranges(be, pipe, bs, RC.sized_stream(pipe, bs, n * bs))


def test_range_1500_blocks_gpu(be):
    """past 1 023 blocks: NONE&HUFFMAN, 1 500 blocks of 1 KiB and a ragged one"""
    pipe = RC.PIPELINES[1]
    RC.check_ranges(be, pipe, 1024, RC.main_stream(pipe, 1024, 1500))


@pytest.mark.parametrize("pipe", RC.SKIP_PIPES, ids=RC.pipe_id)
def test_range_copy_blocks_gpu(be, pipe):
    RC.check_ranges(be, pipe, 1024, RC.skip_stream(pipe))


@pytest.mark.parametrize("pipe", RC.SHORT_PIPES, ids=RC.pipe_id)
def test_range_short_inner_block_gpu(be, pipe):
    RC.check_ranges(be, pipe, RC.SHORT_BS, RC.device_short_inner(be, pipe), ranges=RC.SHORT_RANGES, slack=RC.SHORT_BS)


def test_range_hints_gpu(be):
    RC.check_hints(be)


@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("pipe", (RC.PIPELINES[1], RC.PIPELINES[2], RC.PIPELINES[3]), ids=RC.pipe_id)
def test_range_capacity_gpu(be, pipe, bs):
    RC.check_capacity(be, pipe, bs)


def test_range_damage_gpu(be):
    RC.check_damage(be)


def test_range_contract_gpu(be):
    RC.check_contract(be)


@pytest.mark.parametrize("k", (1, 7, 40))
@pytest.mark.parametrize("bs", SIZES[:2])
def test_range_many_gpu(be, bs, k):
    RC.check_many(be, RC.PIPELINES[1], bs, k)


@pytest.mark.parametrize("k", (7, 40))
def test_range_many_transforms_gpu(be, k):
    RC.check_many(be, RC.PIPELINES[3], 1024, k)


def test_range_many_lanes_gpu(be):
    RC.check_many(be, RC.PIPELINES[1], 1024, 7, lanes=[0, 0, 0])


def test_range_fused_chain_gpu(be):
    RC.check_fused_chain(be)
