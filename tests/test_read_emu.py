"""knz_dev_read_many / knz_dev_read on the execution-model emulator (CPU): byte reads against the slices of the bytes the reference's Reader decodes
(tests/read_cases.py over the fixtures of tests/range_cases.py). The same functions run on the MI355X in tests/test_read_gpu.py, there at every
block size and pipeline of the table, on the stream of 1 500 blocks and on a handle of several lanes."""
import pytest

import range_cases as RC
import read_cases as RD


@pytest.fixture(scope="module")
def be():
    import parity_cases as P
    return P.EmuBackend()


def test_read_coverage_guard():
    RD.check_coverage()


def test_read_alignment_grid(be):
    RD.check_alignment_grid(be)


def test_read_packed_destinations(be):
    RD.check_packed(be)


@pytest.mark.parametrize("bs", RC.EMU_BLOCK_SIZES)
@pytest.mark.parametrize("pipe", RC.PIPELINES[:4], ids=RC.pipe_id)
def test_read_block_boundaries(be, pipe, bs):
    RD.check_boundaries(be, pipe, bs)


def test_read_end_of_stream(be):
    RD.check_end(be)


def test_read_dedup(be):
    RD.check_dedup(be)


def test_read_independence(be):
    RD.check_independence(be)


@pytest.mark.parametrize("pipe", RC.SHORT_PIPES, ids=RC.pipe_id)
def test_read_short_inner_block(be, pipe):
    RD.check_short_inner(be, pipe)


def test_read_damage(be):
    RD.check_damage(be)


def test_read_hints(be):
    RD.check_hints(be)


def test_read_contract(be):
    RD.check_contract(be)


@pytest.mark.parametrize("pipe", RC.SKIP_PIPES, ids=RC.pipe_id)
def test_read_copy_blocks(be, pipe):
    RD.check_copy_blocks(be, pipe)


def test_read_single_form(be):
    RD.check_single(be)
