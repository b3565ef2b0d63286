"""Block sizes that are multiples of 16 only, pointers at the minimum alignment of include/knz_gpu.h and destinations of the smallest
capacity, on the MI355X: the cases of tests/geometry_cases.py against the oracle, and against the reference's Writer (oracle/_ref through
tests/ref_lib.py) where it is built. Every pipeline runs at every block size of the table; blocks of 4 MiB + 16 bytes (a 16-byte second
chunk of the order-1 rANS and FPAQ coders in every block) run through NONE / ANS1 and NONE / FPAQ only."""
import pytest

import geometry_cases as G
import many_cases as M
import parity_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return P.GpuBackend()


def test_geometry_coverage_guard_gpu():
    G.check_coverage()


def test_geometry_placement_helper_gpu(be):
    for offset in (0, 1, 4, 16, 252, 255):
        ptr, keep, n = G.place(be, b"\x01\x02\x03" * 11, offset)
        assert ptr % 256 == offset and n == 33 and G.fetch(be, keep, n) == b"\x01\x02\x03" * 11
        G.guards_intact(be, keep, n)
        buf, start = keep
        for at in (start - 1, start + n):
            buf[at] = 0
            with pytest.raises(AssertionError):
                G.guards_intact(be, keep, n)
            buf[at] = G.FILL


@pytest.mark.parametrize("case", G.stream_cases(True), ids=G.case_id)
def test_geometry_stream_gpu(be, case):
    G.check_stream_geometry(be, *case)


@pytest.mark.parametrize("case", [c for c in G.stream_cases(True) if "BWT" in c[0] and c[2] == 16400], ids=G.case_id)
def test_geometry_stream_list_ranking_gpu(be, monkeypatch, case):
    """the inverse BWT by list ranking on blocks of 16 400 bytes (by default blocks below 64 KiB take the chains kernel)"""
    monkeypatch.setenv("KNZ_BWT_RANK_MIN", "256")
    G.check_stream_geometry(be, *case)


@pytest.mark.parametrize("case", [c for c in G.stream_cases(True) if c[1] == "ANS1" and c[2] in (16400, G.BIG_BLOCK)], ids=G.case_id)
def test_geometry_stream_ans1_plain_loop_gpu(be, monkeypatch, case):
    """the compiler's order-1 rANS encode loop next to the hand-written one (the default on the device): both see the 16-byte tail chunks"""
    monkeypatch.setenv("KNZ_ANS1_ENC_PLAIN", "1")
    G.check_stream_geometry(be, *case)


@pytest.mark.parametrize("cfg", (("NONE", "HUFFMAN", 16400, 3, 1234), ("BWT+RANK+ZRLT", "ANS1", 1040, 4, 17), ("LZ", "ANS0", 5008, 3, 5007)))
def test_geometry_block_batch_gpu(be, cfg):
    P.check_block_batch(be, *cfg)


@pytest.mark.parametrize("cfg", (("NONE", "ANS0", 16400, 7, 999, 3, 32), ("BWT+RANK+ZRLT", "ANS1", 5008, 5, 77, 2, 64)))
def test_geometry_multi_device_batch_gpu(be, cfg):
    P.check_multi_device_batch(be, *cfg)


@pytest.mark.parametrize("ranks", (1, 2, 3))
@pytest.mark.parametrize("cfg", (("HUFFMAN", 16400, 5 * 16400 + 777), ("ANS0", 1040, 7 * 1040 + 3)))
def test_geometry_assemble_gpu(be, cfg, ranks):
    P.check_assemble(be, *cfg, ranks)


def test_geometry_short_inner_block_gpu(be):
    G.check_short_inner_block(be)


@pytest.mark.parametrize("bs", (1040, 16400))
@pytest.mark.parametrize("pipe", (0, 2, 3))
def test_geometry_many_shapes_gpu(be, pipe, bs):
    M.check_shapes(be, M.PIPELINES[pipe], bs)


def test_geometry_fuzz_gpu(be):
    G.check_fuzz(be, cases=60, seed=20261019, max_n=200000)


@pytest.mark.parametrize("pow2", (True, False), ids=("pow2", "mult16"))
@pytest.mark.parametrize("case", G.ALIGN_CASES, ids=lambda c: c[0] + "-" + c[1])
def test_geometry_alignment_gpu(be, case, pow2):
    t, e, bs_a, n_a, bs_b, n_b = case
    G.check_alignment(be, t, e, *((bs_a, n_a) if pow2 else (bs_b, n_b)))


@pytest.mark.parametrize("cfg", (("HUFFMAN", 16400, 5 * 16400 + 777), ("ANS0", 1040, 7 * 1040 + 3)))
def test_geometry_sharded_alignment_gpu(be, cfg):
    G.check_sharded_alignment(be, *cfg)


@pytest.mark.parametrize("cfg", (("NONE", "HUFFMAN", 16400), ("BWT+RANK+ZRLT", "ANS1", 1040)))
def test_geometry_many_alignment_gpu(be, cfg):
    G.check_many_alignment(be, *cfg)


@pytest.mark.parametrize("case", G.TIGHT_CASES, ids=G.case_id)
def test_geometry_tight_capacity_gpu(be, case):
    G.check_tight_capacity(be, *case)


@pytest.mark.parametrize("ename", ("HUFFMAN", "ANS0", "ANS1", "FPAQ", "NONE"))
def test_geometry_entropy_objects_unaligned_gpu(be, ename):
    G.check_entropy_objects_unaligned(be, ename)


@pytest.mark.parametrize("tname", sorted(P._TID))
def test_geometry_transform_objects_unaligned_gpu(be, tname):
    G.check_transform_objects_unaligned(be, tname)
