"""Cases for the hand-written loop of the order-1 rANS decoder (kanzi-go_amd/csrc/ans1.hip: knz_ans1_decode_lds2_kernel), shared by the emulator
run and the MI355X run. The default form takes sixteen steps (of four symbols, one per rANS state) a turn in tiles of 256 steps, leaves what
is no whole turn to the compiler's step, writes a finished output word under the next word's first step and reads a step's renormalisation
words through a cursor that the step before moves: so the cases aim at the loop's edges (q = n >> 2 steps around 16, 32, 256, 1024 and with a
ragged last tile, every n & 3), at data that moves the word cursor differently (up to four words a step, none for long stretches, states
that renormalise in different steps), at a chunk boundary, and at the fused ZRLT / RANK chain that reads the decoder's output while it runs.
Every case is a round trip against the oracle: the device's stream is the oracle's, and the oracle's stream decodes to the input on the
device, under each form of the loop (default, KNZ_ANS1_R5_LOOP, KNZ_ANS1_PLAIN, KNZ_ANS1_LOHI_LDS). The emulator has the compiler's loop only,
whichever form is asked for: its run pins the expectations. The oracle's streams are computed once per case and shared."""
import functools

import numpy as np

import oracle_lib as O
import parity_cases as P

K = P.K
FORMS = ("default", "KNZ_ANS1_R5_LOOP", "KNZ_ANS1_PLAIN", "KNZ_ANS1_LOHI_LDS")
_SWITCHES = FORMS[1:] + ("KNZ_ANS1_TABLE_DECODER", "KNZ_NO_RANK_PIPE", "KNZ_RANK_UNPACKED", "KNZ_RANK_CUT", "KNZ_RANK_PIPE_TWO_GROUPS", "KNZ_RANK_PIPE_ONE_GROUP")
# q = 1 (4..7 bytes) is in the list of lengths that the loop's tests were asked for, but inputs of 32 bytes or less are stored raw and never reach the
# decoder's loop (knz_ans1_raw_kernel takes them): what stays under one turn of sixteen and still reaches it are q = 9, 15 and the ragged last tiles
Q_EDGES = (1, 9, 15, 16, 17, 31, 32, 255, 256, 257, 256 + 16 + 3, 1023, 1024, 1025, 4096 + 5)
DATA_STEPS = 4096 + 5                                  # steps of the data cases: sixteen whole tiles and a ragged one
CHUNK = 4 << 20                                        # bytes of an order-1 rANS chunk
TWO_CHUNKS = CHUNK + 4099


def _skew(rng, n):
    """text-like: a few frequent symbols and a long tail, with order-1 structure (a symbol depends on the one before)"""
    base = np.minimum(rng.geometric(0.12, n), 90).astype(np.uint8)
    v = (base + 31).astype(np.uint8)
    v[1:][base[:-1] < 3] = 32                          # behind the most frequent symbols mostly a space
    return v


def _alternation(n):
    """a costly symbol (one of 255, about eight bits) and a free one (always 0 behind any symbol) in turn. The four rANS states decode the four
    quarters of a chunk side by side, a step takes offset j of every quarter: the costly symbols stand at even j in quarters 0 and 1 and at odd
    j in quarters 2 and 3, so states 0 and 3 renormalise in different steps"""
    rng = np.random.default_rng(0x414C54)
    q = n >> 2
    i = np.arange(n)
    costly = (((i % q) + (i // q >= 2)) & 1) == 0
    v = np.zeros(n, dtype=np.uint8)
    v[costly] = rng.integers(1, 256, int(costly.sum()))
    return v


@functools.lru_cache(maxsize=None)
def length_cases():
    """(name, bytes): n = 4 q + r for q at the loop's edges and r = 0..3 (the bytes behind the last whole step are stored raw behind the payload)"""
    rng = np.random.default_rng(0x4C454E)
    out = []
    for q in Q_EDGES:
        for r in range(4):
            out.append(("q%d+%d" % (q, r), _skew(rng, 4 * q + r).tobytes()))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def data_cases():
    """(name, bytes) of 4 DATA_STEPS + 3 bytes each"""
    rng = np.random.default_rng(0x444154)
    n = 4 * DATA_STEPS + 3
    return (
        ("random", rng.integers(0, 256, n, dtype=np.uint8).tobytes()),         # up to four words a step: a tile takes close to 1024 words
        ("one_symbol", bytes([77]) * n),                                       # a context of frequency 2048 (clamped to 2047): no renormalisation for long stretches
        ("two_symbols", (rng.integers(0, 2, n) * 200 + 5).astype(np.uint8).tobytes()),
        ("last_group", rng.integers(240, 256, n, dtype=np.uint8).tobytes()),   # symbols 240..255: the last group of the two-level search
        ("skew", _skew(rng, n).tobytes()),
        ("alternation", _alternation(n).tobytes()),
    )


@functools.lru_cache(maxsize=None)
def two_chunk_case():
    """4 MiB + 4099 bytes in one block: a full chunk (1 048 576 steps, 4096 tiles, no remainder) and a short second one"""
    rng = np.random.default_rng(0x32434B)
    return _skew(rng, TWO_CHUNKS).tobytes()


@functools.lru_cache(maxsize=None)
def chain_case(bs):
    """three blocks of bs bytes for BWT+RANK+ZRLT / ANS1"""
    return P.corpus(3 * bs, seed=11)


@functools.lru_cache(maxsize=None)
def oracle_stream(kind, name, transform, bs):
    return O.compress(payload(kind, name), transform, "ANS1", bs)


def payload(kind, name):
    if kind == "length":
        return dict(length_cases())[name]
    if kind == "data":
        return dict(data_cases())[name]
    if kind == "two_chunks":
        return two_chunk_case()
    return chain_case(int(name))


def check_alternation_phases():
    """the guard of the alternation itself: quarters 0 and 3 have their costly symbols at opposite offsets"""
    v = np.frombuffer(dict(data_cases())["alternation"], dtype=np.uint8)
    q = len(v) >> 2
    assert q == DATA_STEPS
    q0, q3 = v[:q] != 0, v[3 * q:4 * q] != 0
    assert np.all(q0[0::2]) and not np.any(q0[1::2])
    assert np.all(q3[1::2]) and not np.any(q3[0::2])


def _set_form(monkeypatch, form, extra=()):
    for v in _SWITCHES:
        monkeypatch.delenv(v, raising=False)
    if form != "default":
        monkeypatch.setenv(form, "1")
    for v in extra:
        monkeypatch.setenv(v, "1")


def _first_diff(a, b):
    if len(a) != len(b):
        return ("lengths", len(a), len(b))
    d = np.nonzero(np.frombuffer(a, dtype=np.uint8) != np.frombuffer(b, dtype=np.uint8))[0]
    return None if len(d) == 0 else ("first difference at", int(d[0]), "of", len(d))


def round_trip(be, c, kind, name, transform, bs):
    """check_stream's two halves on one codec: the device's stream is the oracle's, and the oracle's stream decodes to the input on the device"""
    data = payload(kind, name)
    exp = oracle_stream(kind, name, transform, bs)
    n = len(data)
    src, _k0 = be.to_dev(data)
    cap = 2 * n + 262144 * (n // bs + 2)
    dst, kdst = be.empty(cap)
    nb = c.dev_compress(src, n, dst, cap)
    assert nb == len(exp) and be.to_host(kdst, nb) == exp, (kind, name, "device stream != oracle stream", nb, len(exp))
    sp, _k1 = be.to_dev(exp, 4)
    out, kout = be.empty(n + 64)
    nd = c.dev_decompress(sp, len(exp), out, n + 64)
    got = be.to_host(kout, nd)
    assert nd == n and got == data, (kind, name, "decoded bytes != input", _first_diff(got, data))


def check_lengths(be, monkeypatch, form):
    _set_form(monkeypatch, form)
    try:
        c = K.Codec("NONE", "ANS1", 1 << 16, lib=be.lib)
        for name, _d in length_cases():
            round_trip(be, c, "length", name, "NONE", 1 << 16)
        c.close()
    finally:
        _set_form(monkeypatch, "default")


def check_data(be, monkeypatch, form, name):
    _set_form(monkeypatch, form)
    try:
        c = K.Codec("NONE", "ANS1", 1 << 16, lib=be.lib)
        round_trip(be, c, "data", name, "NONE", 1 << 16)
        c.close()
    finally:
        _set_form(monkeypatch, "default")


def check_two_chunks(be, monkeypatch, form):
    _set_form(monkeypatch, form)
    try:
        c = K.Codec("NONE", "ANS1", 8 << 20, lib=be.lib)
        round_trip(be, c, "two_chunks", "", "NONE", 8 << 20)
        c.close()
    finally:
        _set_form(monkeypatch, "default")


def check_fused_chain(be, monkeypatch, form, bs, two_groups):
    """BWT+RANK+ZRLT / ANS1, three blocks: the chain wave takes a block's first quarter from the decoder while the decoder runs (rank_pipe.hip)"""
    _set_form(monkeypatch, form, ("KNZ_RANK_PIPE_TWO_GROUPS",) if two_groups else ())
    try:
        c = K.Codec("BWT+RANK+ZRLT", "ANS1", bs, lib=be.lib)
        round_trip(be, c, "chain", str(bs), "BWT+RANK+ZRLT", bs)
        assert c.last_counter(6) >= 1, (form, bs, two_groups, "no block took the fused chain")
        c.close()
    finally:
        _set_form(monkeypatch, "default")
