"""knz_dev_write_streams on the execution-model emulator (CPU): every target of one call against the existing single call for that target alone and
against the reference Writer's stream for the edited input (tests/write_streams_cases.py over the fixtures of tests/write_cases.py). The same
functions run on the MI355X in tests/test_write_streams_gpu.py, there with 300 targets, at 4 MiB blocks and on a handle of two lanes."""
import pytest

import write_cases as WR
import write_streams_cases as WS


@pytest.fixture(scope="module")
def be():
    import parity_cases as P
    return P.EmuBackend()


@pytest.fixture(params=["fwd", "rev"])
def sched(request, monkeypatch):
    monkeypatch.setenv("KNZ_EMU_SCHED", request.param)                      # thread order inside a workgroup: catches missing barriers
    return request.param


def test_write_streams_coverage_guard():
    WS.check_coverage()


@pytest.mark.parametrize("pipe", (WS.GRID_PIPE, WS.XF_PIPE), ids=WS.RC.pipe_id)
def test_write_streams_equivalence(be, pipe):
    WS.check_equivalence(be, pipe, 1024)


@pytest.mark.parametrize("pipe", WR.EMU_WIDE, ids=WS.RC.pipe_id)
def test_write_streams_equivalence_16400(be, pipe):
    WS.check_equivalence(be, pipe, 16400)


@pytest.mark.parametrize("pipe", (WS.GRID_PIPE, WS.XF_PIPE), ids=WS.RC.pipe_id)
def test_write_streams_equivalence_schedules(be, pipe, sched):
    WS.check_equivalence(be, pipe, 1024, decode=False)


def test_write_streams_placement(be):
    WS.check_placement(be)


def test_write_streams_isolation(be):
    WS.check_isolation(be)


def test_write_streams_counters(be):
    WS.check_counters(be)


def test_write_streams_contract(be):
    WS.check_contract(be)


def test_write_streams_many_targets(be):
    WS.check_many(be, 70)


def test_write_streams_refused_workspace(be, monkeypatch):
    WS.check_workspace(be, monkeypatch)
