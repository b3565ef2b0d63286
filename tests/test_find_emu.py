"""knz_dev_find_many / knz_dev_find on the execution-model emulator (CPU): the match offsets against bytes.find over the bytes the reference's Reader
decodes (tests/find_cases.py). A quarter of the lengths of tests/test_find_gpu.py; the cases whose answer is an order (dense hits, hits_cap) run under
both thread orders of a workgroup."""
import pytest

import find_cases as F

SCALE = "emu"


@pytest.fixture(scope="module")
def be():
    import parity_cases as P
    return P.EmuBackend()


@pytest.fixture(params=["fwd", "rev"])
def sched(request, monkeypatch):
    monkeypatch.setenv("KNZ_EMU_SCHED", request.param)                      # thread order inside a workgroup: catches missing barriers
    return request.param


def test_find_honesty_guard():
    total, empty = F.check_honesty(SCALE)
    assert total >= 200 and 10 * empty <= total


def test_find_symbols(be):
    F.check_symbols(be)


@pytest.mark.parametrize("bs", F.BLOCK_SIZES)
@pytest.mark.parametrize("pipe", F.PIPES, ids=F.RC.pipe_id)
def test_find_pattern_lengths(be, pipe, bs):
    F.run_job(be, F.lengths_job(pipe, bs, SCALE))


@pytest.mark.parametrize("bs", F.BLOCK_SIZES)
@pytest.mark.parametrize("pipe", F.PIPES, ids=F.RC.pipe_id)
def test_find_block_boundaries(be, pipe, bs):
    F.run_job(be, F.boundary_job(pipe, bs, SCALE))


@pytest.mark.parametrize("bs", F.BLOCK_SIZES)
@pytest.mark.parametrize("pipe", F.PIPES, ids=F.RC.pipe_id)
def test_find_dense_small_tile(be, sched, pipe, bs):
    F.run_job(be, F.dense_job(pipe, bs, SCALE, F.SMALL_TILE))


def test_find_dense_default_tile(be, sched):
    F.run_job(be, F.dense_job(F.PIPES[1], 16384, SCALE, None))


@pytest.mark.parametrize("bs", F.BLOCK_SIZES)
@pytest.mark.parametrize("pipe", F.PIPES[1:3], ids=F.RC.pipe_id)
def test_find_window_edges(be, pipe, bs):
    F.run_job(be, F.edges_job(pipe, bs, SCALE))


@pytest.mark.parametrize("bs", F.BLOCK_SIZES)
def test_find_hits_cap(be, sched, bs):
    F.run_job(be, F.caps_job(F.PIPES[3], bs, SCALE))


@pytest.mark.parametrize("bs", F.BLOCK_SIZES)
def test_find_many(be, bs):
    F.check_many(be, F.PIPES[1], bs, SCALE)


def test_find_damage(be):
    F.check_damage(be, SCALE)


@pytest.mark.parametrize("bs", F.BLOCK_SIZES)
@pytest.mark.parametrize("pipe", (F.PIPES[1], F.PIPES[3]), ids=F.RC.pipe_id)
def test_find_short_inner_block(be, pipe, bs):
    F.run_job(be, F.short_job(pipe, bs, SCALE))


def test_find_contract(be):
    F.check_contract(be, SCALE)


def test_find_no_phantom_entries(be):
    F.check_no_phantom(be, SCALE)
