"""PACK / DNA transforms (alias.hip) on the MI355X: objects, streams (the -l 2 preset DNA+LZ&HUFFMAN also at 4 MiB blocks), batch hooks,
damaged input, each against the reference's own AliasCodec (oracle/_ref through tests/ref_lib.py)."""
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import parity_cases as P
    return P.GpuBackend()


def test_alias_supported_gpu(be):
    import alias_cases as A
    L = A.K.load_library(be.lib)
    assert L.knz_supports((19 << 42) | (3 << 36), 1) == 1
    assert L.knz_supports(18 << 42, 0) == 1


def test_alias_coverage_guard_gpu():
    import alias_cases as A
    A.check_coverage()


def test_alias_objects_gpu(be):
    import alias_cases as A
    A.check_objects(be, None, big=True)


def test_alias_dt_handover_gpu(be):
    import alias_cases as A
    A.check_dt_handover(be, big=True)


@pytest.mark.parametrize("stream", range(6))
def test_alias_streams_gpu(be, stream):
    import alias_cases as A
    A.check_streams(be, big=True, streams=A.STREAMS[stream: stream + 1])


def test_alias_preset_4mib_blocks_gpu(be):
    """DNA+LZ&HUFFMAN as the CLI's -l 2 runs it: 4 MiB blocks, DNA, text and small-alphabet blocks side by side"""
    import alias_cases as A
    bs = 4 << 20
    named = {n: d for n, _r, d in A.inputs(True)}
    dna = (named["dna-motif"] * 40)[: bs + 12_345]
    data = dna + (named["text-plain"] * 90)[:bs] + (named["small-4"] * 16)[: bs // 2 + 3]
    codec = A.K.Codec("DNA+LZ", "HUFFMAN", bs, lib=be.lib)
    A._stream_both_ways(be, codec, data, "DNA+LZ", "HUFFMAN", bs, 0, "4 MiB blocks")
    codec.close()


def test_alias_batch_hooks_gpu(be):
    import alias_cases as A
    A.check_batch_hooks(be, big=True)


def test_alias_damaged_gpu(be):
    import alias_cases as A
    A.check_damaged(be, big=True, guard=False)
