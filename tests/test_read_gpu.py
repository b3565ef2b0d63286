"""knz_dev_read_many / knz_dev_read on the MI355X: byte reads against the slices of the bytes the reference's Reader decodes (tests/read_cases.py
over the fixtures of tests/range_cases.py). The cases of tests/test_read_emu.py, here at every block size and pipeline of the table and on a handle
of several lanes."""
import pytest

import range_cases as RC
import read_cases as RD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import parity_cases as P
    return P.GpuBackend()


def test_read_coverage_guard_gpu():
    RD.check_coverage()


def test_read_alignment_grid_gpu(be):
    RD.check_alignment_grid(be)


def test_read_packed_destinations_gpu(be):
    RD.check_packed(be)


@pytest.mark.parametrize("bs", RC.BLOCK_SIZES)
@pytest.mark.parametrize("pipe", RC.PIPELINES, ids=RC.pipe_id)
def test_read_block_boundaries_gpu(be, pipe, bs):
    RD.check_boundaries(be, pipe, bs)


def test_read_end_of_stream_gpu(be):
    RD.check_end(be)


def test_read_dedup_gpu(be):
    RD.check_dedup(be)


def test_read_independence_gpu(be):
    RD.check_independence(be)


@pytest.mark.parametrize("pipe", RC.SHORT_PIPES, ids=RC.pipe_id)
def test_read_short_inner_block_gpu(be, pipe):
    RD.check_short_inner(be, pipe)


def test_read_damage_gpu(be):
    RD.check_damage(be)


def test_read_hints_gpu(be):
    RD.check_hints(be)


def test_read_contract_gpu(be):
    RD.check_contract(be)


@pytest.mark.parametrize("pipe", RC.SKIP_PIPES, ids=RC.pipe_id)
def test_read_copy_blocks_gpu(be, pipe):
    RD.check_copy_blocks(be, pipe)


def test_read_lanes_gpu(be):
    """a handle of three lanes on device 0: the call runs on the lane that owns reads[0].d_dst, the results are the same"""
    assert RD.check_boundaries(be, RC.PIPELINES[1], 1024, lanes=[0, 0, 0]) == RD.check_boundaries(be, RC.PIPELINES[1], 1024)
    RD.check_independence(be, RC.PIPELINES[1], 1024, lanes=[0, 0, 0])


def test_read_single_form_gpu(be):
    RD.check_single(be)
