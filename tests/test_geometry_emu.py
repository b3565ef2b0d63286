"""Block sizes that are multiples of 16 only, pointers at the minimum alignment of include/knz_gpu.h and destinations of the smallest
capacity, on the execution-model emulator (CPU). The cases are tests/geometry_cases.py's; tests/test_geometry_gpu.py runs them on the
MI355X, where the hand-written loops and the hardware's alignment behaviour are. The slow ones here are the three
test_geometry_many_shapes cases (the whole shape list of many_cases.py at 1040-byte blocks, about 40 s each)."""
import pytest

import geometry_cases as G
import many_cases as M
import parity_cases as P


@pytest.fixture(scope="module")
def be():
    return P.EmuBackend()


def test_geometry_coverage_guard():
    G.check_coverage()


def test_geometry_coverage_guard_refuses_aligned_tables():
    """the guard is what it says: power-of-two block sizes and all-zero placements do not pass it"""
    sizes = tuple(1 << 14 if bs == 16400 else bs for bs in G.BLOCK_SIZES)
    with pytest.raises(AssertionError):
        G.check_coverage(gpu_cases=G.stream_cases(True, sizes), emu_cases=G.stream_cases(False, sizes))
    with pytest.raises(AssertionError):
        G.check_coverage(gpu_cases=G.stream_cases(True, big=4 << 20))
    with pytest.raises(AssertionError):
        G.check_coverage(placements=((0, 0, 0, 0),) * 5)
    with pytest.raises(AssertionError):
        G.check_coverage(placements=tuple((s, d, 4, o) for s, d, _t, o in G.PLACEMENTS))


def test_geometry_placement_helper(be):
    for offset in (0, 1, 4, 16, 252, 255):
        ptr, keep, n = G.place(be, b"\x01\x02\x03" * 11, offset)
        assert ptr % 256 == offset and n == 33 and G.fetch(be, keep, n) == b"\x01\x02\x03" * 11
        G.guards_intact(be, keep, n)
        buf, start = keep
        for at in (start - 1, start + n, start + n + 63, 0, len(buf) - 1):
            buf[at] ^= 1
            with pytest.raises(AssertionError):
                G.guards_intact(be, keep, n)
            buf[at] ^= 1
        buf[start + n] = 0
        G.guards_intact(be, keep, n, slack=1)


@pytest.mark.parametrize("case", G.stream_cases(False), ids=G.case_id)
def test_geometry_stream(be, case):
    G.check_stream_geometry(be, *case)


@pytest.mark.parametrize("cfg", (("NONE", "HUFFMAN", 16400, 3, 1234), ("BWT+RANK+ZRLT", "ANS1", 1040, 4, 17), ("LZ", "ANS0", 5008, 3, 5007)))
def test_geometry_block_batch(be, cfg):
    P.check_block_batch(be, *cfg)


@pytest.mark.parametrize("cfg", (("NONE", "ANS0", 16400, 7, 999, 3, 32), ("BWT+RANK+ZRLT", "ANS1", 5008, 5, 77, 2, 64)))
def test_geometry_multi_device_batch(be, cfg):
    P.check_multi_device_batch(be, *cfg)


@pytest.mark.parametrize("ranks", (1, 2, 3))
@pytest.mark.parametrize("cfg", (("HUFFMAN", 16400, 5 * 16400 + 777), ("ANS0", 1040, 7 * 1040 + 3)))
def test_geometry_assemble(be, cfg, ranks):
    P.check_assemble(be, *cfg, ranks)


def test_geometry_short_inner_block(be):
    G.check_short_inner_block(be)


@pytest.mark.parametrize("pipe", (0, 2, 3))
def test_geometry_many_shapes(be, monkeypatch, pipe):
    M.check_shapes(be, M.PIPELINES[pipe], 1040, monkeypatch)


def test_geometry_fuzz(be):
    G.check_fuzz(be, cases=25, seed=20261019, max_n=40000, heavy_max_n=6000)


@pytest.mark.parametrize("pow2", (True, False), ids=("pow2", "mult16"))
@pytest.mark.parametrize("case", G.ALIGN_CASES, ids=lambda c: c[0] + "-" + c[1])
def test_geometry_alignment(be, case, pow2):
    t, e, bs_a, n_a, bs_b, n_b = case
    G.check_alignment(be, t, e, *((bs_a, n_a) if pow2 else (bs_b, n_b)))


@pytest.mark.parametrize("cfg", (("HUFFMAN", 16400, 5 * 16400 + 777), ("ANS0", 1040, 7 * 1040 + 3)))
def test_geometry_sharded_alignment(be, cfg):
    G.check_sharded_alignment(be, *cfg)


@pytest.mark.parametrize("cfg", (("NONE", "HUFFMAN", 16400), ("BWT+RANK+ZRLT", "ANS1", 1040)))
def test_geometry_many_alignment(be, cfg):
    G.check_many_alignment(be, *cfg)


@pytest.mark.parametrize("case", G.TIGHT_CASES, ids=G.case_id)
def test_geometry_tight_capacity(be, case):
    G.check_tight_capacity(be, *case)


@pytest.mark.parametrize("ename", ("HUFFMAN", "ANS0", "ANS1", "FPAQ", "NONE"))
def test_geometry_entropy_objects_unaligned(be, ename):
    G.check_entropy_objects_unaligned(be, ename)


@pytest.mark.parametrize("tname", sorted(P._TID))
def test_geometry_transform_objects_unaligned(be, tname):
    G.check_transform_objects_unaligned(be, tname)
