"""knz_dev_write_many / knz_dev_append on the MI355X: the new stream against the reference Writer's stream for the edited input
(tests/write_cases.py over the fixtures of tests/range_cases.py). The cases of tests/test_write_emu.py, here at every block size of the table, at
4 MiB blocks and on a handle of two lanes."""
import pytest

import range_cases as RC
import write_cases as WR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import parity_cases as P
    return P.GpuBackend()


def test_write_coverage_guard_gpu():
    WR.check_coverage()


def test_write_alignment_grid_gpu(be):
    WR.check_alignment_grid(be)


@pytest.mark.parametrize("bs", RC.BLOCK_SIZES)
@pytest.mark.parametrize("pipe", RC.PIPELINES, ids=RC.pipe_id)
def test_write_block_boundaries_gpu(be, pipe, bs):
    WR.check_boundaries(be, pipe, bs)


@pytest.mark.parametrize("pipe", RC.SKIP_PIPES, ids=RC.pipe_id)
def test_write_block_boundaries_skip_gpu(be, pipe):
    WR.check_boundaries(be, pipe, 1024)
    WR.check_copy_blocks(be, pipe)


def test_write_order_gpu(be):
    WR.check_order(be)
    WR.check_order(be, WR.XF_PIPE, 16400)


@pytest.mark.parametrize("bs", RC.BLOCK_SIZES)
@pytest.mark.parametrize("pipe", WR.EMU_WIDE + (WR.XF_PIPE,), ids=RC.pipe_id)
def test_write_headers_gpu(be, pipe, bs):
    WR.check_headers(be, pipe, bs)


def test_write_counters_gpu(be):
    WR.check_counters(be)


def test_write_damage_gpu(be):
    WR.check_damage(be)


@pytest.mark.parametrize("pipe", RC.SHORT_PIPES, ids=RC.pipe_id)
def test_write_short_inner_block_gpu(be, pipe):
    WR.check_short_inner(be, pipe)


def test_write_contract_gpu(be):
    WR.check_contract(be)


def test_write_round_trip_gpu(be):
    WR.check_round_trip(be)
    WR.check_round_trip(be, RC.PIPELINES[2], 65552)


@pytest.mark.parametrize("pipe", (WR.XF_PIPE, RC.PIPELINES[2]), ids=RC.pipe_id)
def test_write_large_blocks_gpu(be, pipe):
    WR.check_large(be, pipe)


def test_write_lanes_gpu(be):
    """a handle of two lanes on device 0: the call runs on the lane that owns d_dst, the stream is the same"""
    assert WR.check_boundaries(be, RC.PIPELINES[1], 1024, lanes=[0, 0]) == WR.check_boundaries(be, RC.PIPELINES[1], 1024)
    WR.check_large(be, RC.PIPELINES[2], lanes=[0, 0])
