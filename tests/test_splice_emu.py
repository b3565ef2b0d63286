"""knz_dev_splice_many / knz_dev_concat / knz_dev_slice on the execution-model emulator (CPU): every output against the bit-splicer over the reference
Writer's streams, and against the reference Writer itself where the identity applies (tests/splice_cases.py over the fixtures of
tests/range_cases.py). The same functions run on the MI355X in tests/test_splice_gpu.py, there at every block size of the table and on a handle of
two lanes."""
import pytest

import range_cases as RC
import splice_cases as SP

EMU_BLOCK_SIZES = (1024, 16400)
EMU_WIDE = (RC.PIPELINES[0], RC.PIPELINES[1], RC.PIPELINES[5])   # the pipelines the emulator also runs at 16400 (its LZ and BWT decoders take 8 s to a minute there)
EMU_CASES = [(p, 1024) for p in RC.PIPELINES] + [(p, 16400) for p in EMU_WIDE]


@pytest.fixture(scope="module")
def be():
    import parity_cases as P
    return P.EmuBackend()


@pytest.fixture(params=["fwd", "rev"])
def sched(request, monkeypatch):
    monkeypatch.setenv("KNZ_EMU_SCHED", request.param)                      # thread order inside a workgroup: catches missing barriers
    return request.param


def test_splice_shifts_guard():
    SP.check_shifts(EMU_CASES)


@pytest.mark.parametrize("pipe,bs", EMU_CASES, ids=lambda v: RC.pipe_id(v) if isinstance(v, tuple) else str(v))
def test_splice_concat(be, pipe, bs):
    SP.check_concat(be, pipe, bs)


@pytest.mark.parametrize("pipe,bs", EMU_CASES, ids=lambda v: RC.pipe_id(v) if isinstance(v, tuple) else str(v))
def test_splice_slice(be, pipe, bs):
    SP.check_slice(be, pipe, bs)


def test_splice_split_and_regroup(be, sched):
    SP.check_regroup(be)


@pytest.mark.parametrize("pipe", (SP.RAW, SP.HUF), ids=RC.pipe_id)
def test_splice_tiny_frames_and_empty_pieces(be, pipe, sched):
    SP.check_tiny(be, pipe)


@pytest.mark.parametrize("bs", EMU_BLOCK_SIZES)
@pytest.mark.parametrize("pipe", (SP.HUF, RC.PIPELINES[5]), ids=RC.pipe_id)
def test_splice_alignment_and_capacity(be, pipe, bs):
    SP.check_alignment(be, pipe, bs)


def test_splice_trouble(be, sched):
    SP.check_trouble(be)


def test_splice_damage(be):
    SP.check_damage(be)


@pytest.mark.parametrize("pipe", RC.SKIP_PIPES, ids=RC.pipe_id)
def test_splice_copy_blocks(be, pipe):
    SP.check_skip(be, pipe)


@pytest.mark.parametrize("pipe", RC.SHORT_PIPES, ids=RC.pipe_id)
def test_splice_short_inner_block(be, pipe):
    SP.check_short_inner(be, pipe)


def test_splice_counters(be):
    SP.check_counters(be)


def test_splice_contract(be):
    SP.check_contract(be)
