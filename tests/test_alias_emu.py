"""PACK / DNA transforms (alias.hip) on the execution-model emulator (CPU): objects, streams, batch hooks, damaged input, each against the
reference's own AliasCodec (oracle/_ref through tests/ref_lib.py). The same cases run on the MI355X in tests/test_alias_gpu.py."""
import pytest


@pytest.fixture(scope="module")
def be():
    import parity_cases as P
    return P.EmuBackend()


def test_alias_supported(be):
    import alias_cases as A
    L = A.K.load_library(be.lib)
    assert L.knz_supports((19 << 42) | (3 << 36), 1) == 1                 # DNA+LZ & HUFFMAN: the reference's -l 2
    assert L.knz_supports(18 << 42, 0) == 1
    assert L.knz_max_encoded_len(18 << 42, 5000) == 5000 + 1024


def test_alias_coverage_guard():
    import alias_cases as A
    A.check_coverage()


def test_alias_objects(be, monkeypatch):
    import alias_cases as A
    A.check_objects(be, monkeypatch, big=False)


def test_alias_dt_handover(be):
    import alias_cases as A
    A.check_dt_handover(be, big=False)


@pytest.mark.parametrize("stream", range(6))
def test_alias_streams(be, stream):
    import alias_cases as A
    A.check_streams(be, big=False, streams=A.STREAMS[stream: stream + 1], named_from=1 << 16)


def test_alias_batch_hooks(be):
    import alias_cases as A
    A.check_batch_hooks(be, big=False)


def test_alias_damaged(be):
    import alias_cases as A
    A.check_damaged(be, big=False, guard=True)
