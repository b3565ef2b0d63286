"""knz_dev_write_streams on the MI355X: every target of one call against the existing single call for that target alone and against the reference
Writer's stream for the edited input (tests/write_streams_cases.py). The cases of tests/test_write_streams_emu.py, here with 300 targets in one call,
at 4 MiB blocks and on a handle of two lanes."""
import pytest

import range_cases as RC
import write_cases as WR
import write_streams_cases as WS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import parity_cases as P
    return P.GpuBackend()


def test_write_streams_coverage_guard_gpu():
    WS.check_coverage()


@pytest.mark.parametrize("pipe", (WS.GRID_PIPE, WS.XF_PIPE), ids=RC.pipe_id)
def test_write_streams_equivalence_gpu(be, pipe):
    WS.check_equivalence(be, pipe, 1024)


@pytest.mark.parametrize("pipe", WR.EMU_WIDE, ids=RC.pipe_id)
def test_write_streams_equivalence_16400_gpu(be, pipe):
    WS.check_equivalence(be, pipe, 16400)


def test_write_streams_placement_gpu(be):
    WS.check_placement(be)


def test_write_streams_isolation_gpu(be):
    WS.check_isolation(be)


def test_write_streams_counters_gpu(be):
    WS.check_counters(be)


def test_write_streams_contract_gpu(be):
    WS.check_contract(be)


def test_write_streams_many_targets_gpu(be):
    WS.check_many(be, 300)


@pytest.mark.parametrize("pipe,other", ((WR.XF_PIPE, RC.PIPELINES[2]), (RC.PIPELINES[2], WR.XF_PIPE)), ids=("BWT-ANS1", "LZ-ANS0"))
def test_write_streams_large_blocks_gpu(be, pipe, other):
    WS.check_large(be, WS.large_targets(pipe, other), pipe)


def test_write_streams_lanes_gpu(be):
    """a handle of two lanes on device 0: the call runs on the lane that owns targets[0].d_dst, the streams are the same"""
    targets = WS.large_targets(WR.XF_PIPE, RC.PIPELINES[2])
    assert WS.check_large(be, targets, WR.XF_PIPE, lanes=[0, 0]) == WS.check_large(be, targets, WR.XF_PIPE)
    assert WS.check_equivalence(be, WS.GRID_PIPE, 1024, lanes=[0, 0], decode=False) == WS.check_equivalence(be, WS.GRID_PIPE, 1024, decode=False)
