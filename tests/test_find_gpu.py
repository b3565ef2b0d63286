"""knz_dev_find_many / knz_dev_find on the MI355X: the match offsets against bytes.find over the bytes the reference's Reader
decodes (tests/find_cases.py). The cases of tests/test_find_emu.py at four times the lengths, and on a handle of several lanes."""
import pytest

import find_cases as F

SCALE = "gpu"
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import parity_cases as P
    return P.GpuBackend()


def test_find_honesty_guard_gpu():
    total, empty = F.check_honesty(SCALE)
    assert total >= 200 and 10 * empty <= total


def test_find_symbols_gpu(be):
    F.check_symbols(be)


@pytest.mark.parametrize("bs", F.BLOCK_SIZES)
@pytest.mark.parametrize("pipe", F.PIPES, ids=F.RC.pipe_id)
def test_find_pattern_lengths_gpu(be, pipe, bs):
    F.run_job(be, F.lengths_job(pipe, bs, SCALE))


@pytest.mark.parametrize("bs", F.BLOCK_SIZES)
@pytest.mark.parametrize("pipe", F.PIPES, ids=F.RC.pipe_id)
def test_find_block_boundaries_gpu(be, pipe, bs):
    F.run_job(be, F.boundary_job(pipe, bs, SCALE))


@pytest.mark.parametrize("bs", F.BLOCK_SIZES)
@pytest.mark.parametrize("pipe", F.PIPES, ids=F.RC.pipe_id)
def test_find_dense_small_tile_gpu(be, pipe, bs):
    F.run_job(be, F.dense_job(pipe, bs, SCALE, F.SMALL_TILE))


def test_find_dense_default_tile_gpu(be):
    F.run_job(be, F.dense_job(F.PIPES[1], 16384, SCALE, None))


@pytest.mark.parametrize("bs", F.BLOCK_SIZES)
@pytest.mark.parametrize("pipe", F.PIPES[1:3], ids=F.RC.pipe_id)
def test_find_window_edges_gpu(be, pipe, bs):
    F.run_job(be, F.edges_job(pipe, bs, SCALE))


@pytest.mark.parametrize("bs", F.BLOCK_SIZES)
def test_find_hits_cap_gpu(be, bs):
    F.run_job(be, F.caps_job(F.PIPES[3], bs, SCALE))


@pytest.mark.parametrize("bs", F.BLOCK_SIZES)
def test_find_many_gpu(be, bs):
    F.check_many(be, F.PIPES[1], bs, SCALE)


def test_find_damage_gpu(be):
    F.check_damage(be, SCALE)


@pytest.mark.parametrize("bs", F.BLOCK_SIZES)
@pytest.mark.parametrize("pipe", (F.PIPES[1], F.PIPES[3]), ids=F.RC.pipe_id)
def test_find_short_inner_block_gpu(be, pipe, bs):
    F.run_job(be, F.short_job(pipe, bs, SCALE))


def test_find_contract_gpu(be):
    F.check_contract(be, SCALE)


def test_find_no_phantom_entries_gpu(be):
    F.check_no_phantom(be, SCALE)


def test_find_lanes_gpu(be):
    """a handle of three lanes on device 0: the call runs on the lane that owns finds[0].d_hits, the results are the same"""
    job = F.many_job(F.PIPES[1], 1024, SCALE)
    codec = F.M.codec_for(be, job.pipe, job.bs, devices=[0, 0, 0])
    F.run_job(be, job, codec)
    codec.close()
