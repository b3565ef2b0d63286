"""Cases for the two-wave order-1 rANS encoder (kanzi-go_amd/csrc/ans1.hip: knz_ans1_encode_asm_kernel), shared by the emulator run and the MI355X
run. Wave 0 codes a chunk in turns of 48 steps and leaves the states in front of their renormalisations in an LDS ring of RING turns; wave 1 takes a
turn from the ring, decides which states are words and stores them. So the cases aim at the turn and at the ring: step counts q = n >> 2 around one
group (16), one turn (48), two turns, the ring's length (48 RING) and twice that, with every n & 3 (the bytes behind the last whole step are stored
raw); data that makes all four states renormalise at almost every step, almost never, and in different steps; a chunk boundary (two workgroups);
three blocks behind BWT+RANK+ZRLT; and several launches (KNZ_ANS1_GROUP_BLOCKS=1). Every case is a round trip against the oracle (the device's
stream is the oracle's, and the oracle's stream decodes to the input on the device) under the default form and under KNZ_ANS1_ENC_ONE_WAVE, the
one-wave kernel that places its words itself (on the emulator: the one-wave C++ kernel). Inputs of 32 bytes or less (q <= 8) are stored raw and
never reach the coder: q = 1 is in the list because the list was asked for."""
import functools

import numpy as np

import ans1_loop_cases as A
import oracle_lib as O
import parity_cases as P

K = P.K
FORMS = ("default", "KNZ_ANS1_ENC_ONE_WAVE")
RING = 8                                               # KNZ_A1E_RING
TURN = 48
Q_EDGES = (1, 15, 16, 17, 47, 48, 49, 95, 96, 97, TURN * RING - 1, TURN * RING, TURN * RING + 1, 2 * TURN * RING + 5)
DATA_STEPS = 4096 + 5                                  # 86 turns: the ring goes round ten times
TWO_CHUNKS = A.TWO_CHUNKS
CHAIN_BS = 1 << 14
_SWITCHES = FORMS[1:] + ("KNZ_ANS1_ENC_PLAIN", "KNZ_ANS1_GROUP_BLOCKS")


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (bytes, transform, block size)"""
    rng = np.random.default_rng(0x574156)
    out = {}
    for q in Q_EDGES:
        for r in range(4):
            out["q%d+%d" % (q, r)] = (A._skew(rng, 4 * q + r).tobytes(), "NONE", 1 << 16)
    n = 4 * DATA_STEPS + 3
    out["random"] = (rng.integers(0, 256, n, dtype=np.uint8).tobytes(), "NONE", 1 << 16)      # all four states renormalise at almost every step
    out["one_symbol"] = (bytes([77]) * n, "NONE", 1 << 16)                                       # almost none does
    out["alternation"] = (A._alternation(n).tobytes(), "NONE", 1 << 16)                          # states 0 and 3 renormalise in different steps
    out["two_chunks"] = (A.two_chunk_case(), "NONE", 8 << 20)                                    # two chunks: two workgroups
    out["chain"] = (P.corpus(3 * CHAIN_BS, seed=11), "BWT+RANK+ZRLT", CHAIN_BS)
    out["blocks"] = (A._skew(rng, 5 * 4096 + 1234).tobytes(), "NONE", 4096)                      # six blocks: six launches under KNZ_ANS1_GROUP_BLOCKS=1
    return out


LENGTH_NAMES = tuple("q%d+%d" % (q, r) for q in Q_EDGES for r in range(4))
DATA_NAMES = ("random", "one_symbol", "alternation")


@functools.lru_cache(maxsize=None)
def oracle_stream(name):
    data, transform, bs = cases()[name]
    return O.compress(data, transform, "ANS1", bs)


def check_case_shapes():
    c = cases()
    assert [len(c[nm][0]) >> 2 for nm in LENGTH_NAMES][::4] == list(Q_EDGES)
    assert [len(c[nm][0]) & 3 for nm in LENGTH_NAMES] == [0, 1, 2, 3] * len(Q_EDGES)
    assert all(len(c[nm][0]) == 4 * DATA_STEPS + 3 for nm in DATA_NAMES) and len(c["two_chunks"][0]) == (4 << 20) + 4099
    v = np.frombuffer(c["alternation"][0], dtype=np.uint8)
    q = len(v) >> 2
    assert np.all(v[:q][0::2] != 0) and not np.any(v[:q][1::2]) and np.all(v[3 * q:4 * q][1::2] != 0) and not np.any(v[3 * q:4 * q][0::2])


def _set_form(monkeypatch, form, group_blocks=False):
    for v in _SWITCHES:
        monkeypatch.delenv(v, raising=False)
    if form != "default":
        monkeypatch.setenv(form, "1")
    if group_blocks:
        monkeypatch.setenv("KNZ_ANS1_GROUP_BLOCKS", "1")


def round_trips(be, monkeypatch, form, names, group_blocks=False):
    _set_form(monkeypatch, form, group_blocks)
    try:
        codecs = {}
        for name in names:
            data, transform, bs = cases()[name]
            if (transform, bs) not in codecs:
                codecs[(transform, bs)] = K.Codec(transform, "ANS1", bs, lib=be.lib)
            c = codecs[(transform, bs)]
            exp = oracle_stream(name)
            n = len(data)
            src, _k0 = be.to_dev(data)
            cap = 2 * n + 262144 * (n // bs + 2)
            dst, kdst = be.empty(cap)
            nb = c.dev_compress(src, n, dst, cap)
            assert nb == len(exp) and be.to_host(kdst, nb) == exp, (name, form, "device stream != oracle stream", nb, len(exp))
            sp, _k1 = be.to_dev(exp, 4)
            out, kout = be.empty(n + 64)
            nd = c.dev_decompress(sp, len(exp), out, n + 64)
            assert nd == n and be.to_host(kout, nd) == data, (name, form, "decoded bytes != input")
        for c in codecs.values():
            c.close()
    finally:
        _set_form(monkeypatch, "default")
