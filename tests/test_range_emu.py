"""knz_dev_stream_index / knz_dev_decompress_range / knz_dev_decompress_many_range on the execution-model emulator (CPU): the index against a
framing walk in plain Python, every range against the slice of the reference Reader's bytes (oracle/_ref through tests/ref_lib.py), the many
form against the single calls. The same functions run on the MI355X in tests/test_range_gpu.py, there also at 65 552-byte blocks and on a
stream of 1 500 blocks."""
import pytest

import range_cases as RC

SIZES = RC.EMU_BLOCK_SIZES
# at 16 400-byte blocks the emulator runs the ranges of a few blocks of the transform pipelines (the whole stream once, through dev_decompress)
SHORT = ((1, 2), (38, 39), (19, 20), (19, 24), (39, RC.END), (36, 78))


@pytest.fixture(scope="module")
def be():
    import parity_cases as P
    return P.EmuBackend()


def test_range_coverage_guard():
    RC.check_coverage()


@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("pipe", RC.PIPELINES, ids=RC.pipe_id)
def test_range_index(be, pipe, bs):
    RC.check_index(be, pipe, bs)


@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("pipe", RC.PIPELINES, ids=RC.pipe_id)
def test_range_is_slice(be, pipe, bs):
    RC.check_ranges(be, pipe, bs, RC.main_stream(pipe, bs), ranges=SHORT if (bs > 1024 and pipe[0] != "NONE") else None)


@pytest.mark.parametrize("n", (1, 0), ids=("one-block", "empty"))
@pytest.mark.parametrize("pipe", RC.PIPELINES, ids=RC.pipe_id)
def test_range_small_streams(be, pipe, n):
    for bs in SIZES:
        RC.check_ranges(be, pipe, bs, RC.sized_stream(pipe, bs, n * bs))


@pytest.mark.parametrize("pipe", RC.SKIP_PIPES, ids=RC.pipe_id)
def test_range_copy_blocks(be, pipe):
    RC.check_ranges(be, pipe, 1024, RC.skip_stream(pipe))


@pytest.mark.parametrize("pipe", RC.SHORT_PIPES, ids=RC.pipe_id)
def test_range_short_inner_block(be, pipe):
    RC.check_ranges(be, pipe, RC.SHORT_BS, RC.device_short_inner(be, pipe), ranges=RC.SHORT_RANGES, slack=RC.SHORT_BS)


def test_range_hints(be):
    RC.check_hints(be)


@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("pipe", (RC.PIPELINES[1], RC.PIPELINES[2]), ids=RC.pipe_id)
def test_range_capacity(be, pipe, bs):
    RC.check_capacity(be, pipe, bs)


def test_range_damage(be):
    RC.check_damage(be)


def test_range_contract(be):
    RC.check_contract(be)


@pytest.mark.parametrize("k", (1, 7, 40))
def test_range_many(be, k):
    RC.check_many(be, RC.PIPELINES[1], 1024, k)


def test_range_many_transforms(be):
    RC.check_many(be, RC.PIPELINES[3], 1024, 7)


def test_range_many_lanes(be):
    RC.check_many(be, RC.PIPELINES[1], 1024, 7, lanes=[0, 0, 0])


def test_range_fused_chain(be):
    RC.check_fused_chain(be)
