"""knz_dev_splice_many / knz_dev_concat / knz_dev_slice on the MI355X: every output against the bit-splicer over the reference Writer's streams, and
against the reference Writer itself where the identity applies (tests/splice_cases.py over the fixtures of tests/range_cases.py). The cases of
tests/test_splice_emu.py, here at every block size and pipeline of the table and on a handle of two lanes."""
import pytest

import range_cases as RC
import splice_cases as SP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import parity_cases as P
    return P.GpuBackend()


def test_splice_shifts_guard_gpu():
    SP.check_shifts([(p, bs) for p in RC.PIPELINES for bs in RC.BLOCK_SIZES])


@pytest.mark.parametrize("bs", RC.BLOCK_SIZES)
@pytest.mark.parametrize("pipe", RC.PIPELINES, ids=RC.pipe_id)
def test_splice_concat_gpu(be, pipe, bs):
    SP.check_concat(be, pipe, bs)


@pytest.mark.parametrize("bs", RC.BLOCK_SIZES)
@pytest.mark.parametrize("pipe", RC.PIPELINES, ids=RC.pipe_id)
def test_splice_slice_gpu(be, pipe, bs):
    SP.check_slice(be, pipe, bs)


def test_splice_split_and_regroup_gpu(be):
    SP.check_regroup(be)


@pytest.mark.parametrize("pipe", (SP.RAW, SP.HUF), ids=RC.pipe_id)
def test_splice_tiny_frames_and_empty_pieces_gpu(be, pipe):
    SP.check_tiny(be, pipe)


@pytest.mark.parametrize("bs", RC.BLOCK_SIZES)
@pytest.mark.parametrize("pipe", RC.PIPELINES, ids=RC.pipe_id)
def test_splice_alignment_and_capacity_gpu(be, pipe, bs):
    SP.check_alignment(be, pipe, bs)


def test_splice_trouble_gpu(be):
    SP.check_trouble(be)


def test_splice_damage_gpu(be):
    SP.check_damage(be)


@pytest.mark.parametrize("pipe", RC.SKIP_PIPES, ids=RC.pipe_id)
def test_splice_copy_blocks_gpu(be, pipe):
    SP.check_skip(be, pipe)


@pytest.mark.parametrize("pipe", RC.SHORT_PIPES, ids=RC.pipe_id)
def test_splice_short_inner_block_gpu(be, pipe):
    SP.check_short_inner(be, pipe)


def test_splice_counters_gpu(be):
    SP.check_counters(be)


def test_splice_contract_gpu(be):
    SP.check_contract(be)


def test_splice_lanes_gpu(be):
    """a handle of two lanes on device 0: the call runs on the lane that owns outs[0].d_dst, the streams are the same"""
    assert SP.check_concat(be, SP.HUF, 1024, lanes=[0, 0]) == SP.check_concat(be, SP.HUF, 1024)
