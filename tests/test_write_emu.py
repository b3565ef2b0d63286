"""knz_dev_write_many / knz_dev_append on the execution-model emulator (CPU): the new stream against the reference Writer's stream for the edited
input (tests/write_cases.py over the fixtures of tests/range_cases.py). The same functions run on the MI355X in tests/test_write_gpu.py, there at
every block size and pipeline of the table, at 4 MiB blocks and on a handle of two lanes."""
import pytest

import range_cases as RC
import write_cases as WR


@pytest.fixture(scope="module")
def be():
    import parity_cases as P
    return P.EmuBackend()


@pytest.fixture(params=["fwd", "rev"])
def sched(request, monkeypatch):
    monkeypatch.setenv("KNZ_EMU_SCHED", request.param)                      # thread order inside a workgroup: catches missing barriers
    return request.param


def test_write_coverage_guard():
    WR.check_coverage()


def test_write_alignment_grid(be, sched):
    WR.check_alignment_grid(be)


@pytest.mark.parametrize("pipe", RC.PIPELINES + RC.SKIP_PIPES, ids=RC.pipe_id)
def test_write_block_boundaries(be, pipe):
    WR.check_boundaries(be, pipe, 1024)


def test_write_block_boundaries_schedules(be, sched):
    WR.check_boundaries(be, WR.XF_PIPE, 1024, names=("several boundaries", "three blocks and five bytes past L", "append of one byte", "END, empty stream"))


@pytest.mark.parametrize("pipe", WR.EMU_WIDE, ids=RC.pipe_id)
def test_write_block_boundaries_16400(be, pipe):
    WR.check_boundaries(be, pipe, 16400)


@pytest.mark.parametrize("pipe", RC.SKIP_PIPES, ids=RC.pipe_id)
def test_write_copy_blocks(be, pipe):
    WR.check_copy_blocks(be, pipe)


def test_write_order(be, sched):
    WR.check_order(be)


@pytest.mark.parametrize("bs", RC.EMU_BLOCK_SIZES)
@pytest.mark.parametrize("pipe", WR.EMU_WIDE, ids=RC.pipe_id)
def test_write_headers(be, pipe, bs):
    WR.check_headers(be, pipe, bs)


def test_write_headers_transforms(be):
    WR.check_headers(be, WR.XF_PIPE, 1024, names=("none -> true size", "KEEP, no field, growth", "KEEP, a block grows or shrinks"))


def test_write_counters(be):
    WR.check_counters(be)


def test_write_damage(be):
    WR.check_damage(be)


@pytest.mark.parametrize("pipe", RC.SHORT_PIPES, ids=RC.pipe_id)
def test_write_short_inner_block(be, pipe):
    WR.check_short_inner(be, pipe)


def test_write_contract(be):
    WR.check_contract(be)


def test_write_refused_workspace(be, monkeypatch):
    WR.check_workspace(be, monkeypatch)


def test_write_round_trip(be):
    WR.check_round_trip(be)
