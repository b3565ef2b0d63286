"""Cases for the hand-written packed inverse RANK loop (kanzi-go_amd/csrc/rank_inv_asm.h: knz_rank_rows_packed), shared by the emulator run and
the MI355X run. The loop takes two groups of sixteen ranks per turn, has one chain of code per kind of group (with / without a rank of 64 or
more) and lets a high rank's path go on to the next symbol by itself, so the cases aim at what can go wrong there: every remainder of the
unroll in front of the byte-by-byte tail, every ordered pair of symbol classes at every pair of neighbouring positions of a row (inside a word,
across words, groups, the two groups of a turn, and rows), and the fused ZRLT / RANK chain, which enters and leaves the loop row by row.
The reference is the oracle's inverse RANK; it is computed once per sequence and shared."""
import functools

import numpy as np

import oracle_lib as O
import parity_cases as P

K = P.K
RANK = P._TID["RANK"]
CLASSES = ("zero", "low", "r1", "r2", "r3")                   # 0, 1..63, 64..127, 128..191, 192..255
_RANGE = {"zero": (0, 0), "low": (1, 63), "r1": (64, 127), "r2": (128, 191), "r3": (192, 255)}


def _of_class(rng, cls):
    lo, hi = _RANGE[cls]
    return int(rng.choice((lo, hi, int(rng.integers(lo, hi + 1)))))    # the class's ends as often as its inside


def _mixed(rng, n):
    """ranks of every class side by side: about a third zeros, a third low, a third spread over the three high registers"""
    cls = rng.choice(5, n, p=(0.34, 0.33, 0.11, 0.11, 0.11))
    lo = np.array([_RANGE[c][0] for c in CLASSES])[cls]
    hi = np.array([_RANGE[c][1] for c in CLASSES])[cls]
    return (lo + rng.integers(0, 1 << 30, n) % (hi - lo + 1)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def length_cases():
    """64 k + t ranks for k in {1, 2, 3, 4, 5, 7, 8, 9}, t in {0, 1, 63}: every remainder of the unroll, with and without a byte-by-byte tail"""
    rng = np.random.default_rng(0x524B4C)
    out = []
    for k in (1, 2, 3, 4, 5, 7, 8, 9):
        for t in (0, 1, 63):
            out.append(("len64x%d+%d" % (k, t), _mixed(rng, 64 * k + t).tobytes()))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def class_pairs():
    """every ordered pair of classes at every neighbouring position pair (p, p + 1) of a row, p = 0..63 (p = 63: across rows): 25 x 64 rows, one
    sequence of 102 400 ranks. Around the pair the ranks are zeros and low ranks, so the pair decides the kind of its group(s). The row with p = 63
    puts its second rank into the next row, so the row behind it is the one with p = 1, whose own pair leaves position 0 alone."""
    rng = np.random.default_rng(0x50414952)
    n = 25 * 64 * 64
    v = (np.minimum(rng.geometric(0.3, n), 40) - 1).astype(np.uint8)
    at = 0
    placed = []
    for a in CLASSES:
        for b in CLASSES:
            for p in (0, 63) + tuple(range(1, 63)):
                v[at + p], v[at + p + 1] = _of_class(rng, a), _of_class(rng, b)
                placed.append((at + p, a, b))
                at += 64
    return v.tobytes(), tuple(placed)


def class_of(r):
    return "zero" if r == 0 else ("low" if r < 64 else CLASSES[1 + (r >> 6)])


def check_class_pairs_cover():
    """the guard of the sequence itself: all 25 x 64 (pair, position) combinations are there"""
    seq, placed = class_pairs()
    seen = set()
    for pos, a, b in placed:
        assert class_of(seq[pos]) == a and class_of(seq[pos + 1]) == b, (pos, a, b)
        seen.add((a, b, pos % 64))
    assert len(seen) == 25 * 64
    assert len(seq) == 102_400


@functools.lru_cache(maxsize=None)
def sequences():
    """(name, ranks): the lengths, the class pairs and parity_cases.rank_patterns()"""
    return length_cases() + (("class_pairs", class_pairs()[0]),) + tuple(P.rank_patterns())


@functools.lru_cache(maxsize=None)
def decoded(name):
    """the oracle's inverse RANK of a sequence (the reference of every check here)"""
    ranks = dict(sequences())[name]
    return O.transform_inverse(RANK, ranks, len(ranks) + 64)


def check_inverse(be, names):
    """the transform object's inverse (the standalone chain kernel) against the oracle's"""
    c = K.Codec("NONE", "NONE", 1 << 20, lib=be.lib)
    t = K.ByteTransform(c, "RANK")
    seqs = dict(sequences())
    for nm in names:
        ranks = seqs[nm]
        got = t.inverse(ranks, len(ranks) + 512)
        assert got == decoded(nm), (nm, "device inverse RANK != oracle inverse RANK", _first_diff(got, decoded(nm)))
    c.close()


def _first_diff(a, b):
    if len(a) != len(b):
        return ("lengths", len(a), len(b))
    d = np.nonzero(np.frombuffer(a, dtype=np.uint8) != np.frombuffer(b, dtype=np.uint8))[0]
    return None if len(d) == 0 else ("first difference at", int(d[0]), "of", len(d))


@functools.lru_cache(maxsize=None)
def chain_payload():
    """the bytes whose RANK forward is the sequences back to back (forward and inverse are each other's inverse on any byte sequence)"""
    return b"".join(decoded(nm) for nm, _r in sequences())


@functools.lru_cache(maxsize=None)
def chain_stream(bs):
    return O.compress(chain_payload(), "RANK+ZRLT", "ANS1", bs)


_SWITCHES = ("KNZ_NO_RANK_PIPE", "KNZ_RANK_UNPACKED", "KNZ_RANK_CUT", "KNZ_RANK_PIPE_TWO_GROUPS", "KNZ_RANK_PIPE_ONE_GROUP")
CUT_ROWS = 37                                                     # an odd number of rows: the packed loop is left in the middle of a turn's worth of rows


def check_fused_chain(be, monkeypatch, bs, cut):
    """the same sequences through the fused ZRLT / RANK chain under the rANS-1 decoder (rank_pipe.hip), which runs the loop over whatever whole rows
    are ready: RANK+ZRLT / ANS1 streams of the oracle, the long chains in a launch of their own; `cut`: the packed form ends after CUT_ROWS rows"""
    data = chain_payload()
    stream = chain_stream(bs)
    for v in _SWITCHES:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("KNZ_RANK_PIPE_TWO_GROUPS", "1")
    if cut:
        monkeypatch.setenv("KNZ_RANK_CUT", str(64 * CUT_ROWS))
    try:
        c = K.Codec("RANK+ZRLT", "ANS1", bs, lib=be.lib)
        sp, _k1 = be.to_dev(stream)
        out, ko = be.empty(len(data) + 4096)
        nd = c.dev_decompress(sp, len(stream), out, len(data) + 4096)
        got = be.to_host(ko, nd)
        assert nd == len(data) and got == data, (bs, cut, _first_diff(got, data))
        assert c.last_counter(6) >= 1, (bs, cut, "no block took the fused chain")
        c.close()
    finally:
        for v in _SWITCHES:
            monkeypatch.delenv(v, raising=False)
