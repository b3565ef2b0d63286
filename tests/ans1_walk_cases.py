"""Cases for the block walker's position walk of the order-1 rANS chunk headers (kanzi-go_amd/csrc/huffman_dec.hip: knz_ans1_walk_header, called by
knz_walk_block_body in huffman_par.hip), shared by the emulator run and the MI355X run. The walk finds the bit position of each of a chunk's 256
context headers and of the chunk's end: it reads an alphabet (a flag, or a 5-bit mask count and up to 32 masks of 8 bits), then one bit width per
group of six (fewer than 64 symbols) or eight frequencies, and jumps over the frequencies themselves. So the inputs are built for the header they
give, which header_shape() reads back from the oracle's stream with a parser in plain Python, and every property a case is there for is asserted on
what that parser finds. Every case is a round trip against the oracle (the device's stream is the oracle's; the oracle's stream decodes to the input
on the device) under the default form and under KNZ_ANS1_WALK_PLAIN, the generic reader's walk that the default replaced. Damaged headers are made
from an oracle's stream and must end in the same code under both forms."""
import functools

import numpy as np

import oracle_lib as O
import parity_cases as P

K = P.K
FORMS = ("default", "KNZ_ANS1_WALK_PLAIN")
ERR_PROCESS_BLOCK = 13
CHUNK = 4 << 20
TWO_CHUNKS = CHUNK + 4099
CHAIN_BS = 1 << 14


# ---- the stream in plain Python -------------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self, stream):
        self.b = np.unpackbits(np.frombuffer(stream, dtype=np.uint8))

    def get(self, pos, n):
        v = 0
        for x in self.b[pos:pos + n]:
            v = (v << 1) | int(x)
        return v

    def ones(self, pos, n):
        return int(self.b[pos:pos + n].sum())


def block_payloads(bits):
    """framing of a .knz stream without checksums (CompressedStream.go:1316-1460, :1816-1852) -> [(bit of the frame, bit of the payload, payload bits)]"""
    sz = bits.get(119, 2)
    pos = 121 + 16 * sz + 15 + 24
    out = []
    while True:
        lw = bits.get(pos, 5) + 3
        written = bits.get(pos + 5, lw)
        if written == 0:
            return out
        out.append((pos, pos + 5 + lw, written))
        pos += 5 + lw + written


def chunk_start(bits, payload):
    """block header (:1878-1914, no checksum) -> (bit of the first chunk header, pre-transform length), or None for a copy block"""
    mode = bits.get(payload, 8)
    if mode & 0x80:
        return None
    pos = payload + 8 + (8 if mode & 0x10 else 0)
    nbytes = 1 + ((mode >> 5) & 3)
    return pos + 8 * nbytes, bits.get(pos, 8 * nbytes)


def parse_chunk_header(bits, pos):
    """decodeHeader (ANSRangeCodec.go:605-710) as far as the walk goes -> (lr, [(bit of the context, symbols, lastMask or None, [logMax of each group])],
    bit behind the last context)"""
    lr = 8 + bits.get(pos, 3)
    pos += 3
    llr = 3
    while (1 << llr) <= lr:
        llr += 1
    ctxs = []
    for _k in range(256):
        at, last = pos, None
        if bits.get(pos, 1) == 0:
            count = 0 if bits.get(pos + 1, 1) else 256
            pos += 2
        else:
            last = bits.get(pos + 1, 5)
            count = bits.ones(pos + 6, 8 * (last + 1))
            pos += 6 + 8 * (last + 1)
        chk = 6 if count < 64 else 8
        widths = []
        for i in range(1, count, chk):
            w = bits.get(pos, llr)
            widths.append(w)
            pos += llr + (min(i + chk, count) - i) * w
        ctxs.append((at, count, last, widths))
    return lr, ctxs, pos


@functools.lru_cache(maxsize=None)
def header_shape(name):
    """of a one-block case: (bit of the chunk header, lr, contexts, bit of the size varint)"""
    stream = oracle_stream(name)
    bits = Bits(stream)
    (_f, payload, _n), = block_payloads(bits)
    at, _pre = chunk_start(bits, payload)
    lr, ctxs, end = parse_chunk_header(bits, at)
    return at, lr, ctxs, end


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
def _pairs(rng, spec, reps):
    """spec: [(context byte, [(symbol, times)])] -> bytes in which `context` is followed by `symbol` reps * times times, the pairs of all contexts shuffled"""
    pairs = [(c, s) for c, syms in spec for s, t in syms for _ in range(reps * t)]
    order = rng.permutation(len(pairs))
    return bytes(x for i in order for x in pairs[i])


def _small_alphabets():
    """contexts 201.. with exactly 1, 2, 6, 7, 8, 63, 64 and 65 symbols (10, 11, ...); most contexts have none"""
    rng = np.random.default_rng(0x534D41)
    spec = [(201 + i, [(10 + j, 1) for j in range(m)]) for i, m in enumerate((1, 2, 6, 7, 8, 63, 64, 65))]
    return _pairs(rng, spec, 10)


def _full_alphabets():
    """context 7 with 255 symbols (all but 255: lastMask 31), context 9 with all 256 (the full-alphabet flag)"""
    rng = np.random.default_rng(0x46554C)
    return _pairs(rng, [(7, [(s, 1) for s in range(255)]), (9, [(s, 1) for s in range(256)])], 5)


def _widths():
    """200: 70 symbols, the first one dominant: every group has width 0 (all frequencies 1); 199: the same with 11 symbols (groups of six);
    198: 70 symbols, a middle one dominant: its group of eight has width 11, an 88-bit jump; 197: symbols below 8 (lastMask 0); 196: symbol 250 (lastMask 31)"""
    rng = np.random.default_rng(0x574944)
    spec = [(200, [(1, 1500)] + [(s, 1) for s in range(2, 71)]),
            (199, [(1, 1500)] + [(s, 1) for s in range(2, 12)]),
            (198, [(40, 1500)] + [(s, 1) for s in range(1, 71) if s != 40]),
            (197, [(1, 3), (2, 1), (5, 2)]),
            (196, [(3, 1), (250, 2)])]
    return _pairs(rng, spec, 2)


def _all_pairs():
    """every symbol behind every symbol: the de Bruijn sequence of order 2 over the 256 bytes (its Lyndon words in order: i, then i j for every j > i),
    the byte values renamed by a random permutation: 64 KiB in which every context has (all but a few of) 256 symbols, the shape of the long blocks"""
    rng = np.random.default_rng(0x414C4C)
    seq = []
    for i in range(256):
        seq.append(i)
        for j in range(i + 1, 256):
            seq += (i, j)
    return rng.permutation(256).astype(np.uint8)[np.array(seq)].tobytes()


@functools.lru_cache(maxsize=None)
def shaped_cases():
    """(name, bytes): one block each under NONE / ANS1"""
    rng = np.random.default_rng(0x52414E)
    return (("small_alphabets", _small_alphabets()), ("full_alphabets", _full_alphabets()), ("widths", _widths()), ("all_pairs", _all_pairs()),
            ("random_64k", rng.integers(0, 256, 1 << 16, dtype=np.uint8).tobytes()), ("raw_20", bytes(range(20))), ("raw_32", bytes(range(100, 132))))


SHAPED_BS = 1 << 17


def check_shapes():
    """the guard of the inputs: the oracle's headers have what the cases are there for"""
    def counts(name):
        return [c for _at, c, _l, _w in header_shape(name)[2]]
    assert {0, 1, 2, 6, 7, 8, 63, 64, 65} <= set(counts("small_alphabets")), sorted(set(counts("small_alphabets")))
    full = header_shape("full_alphabets")[2]
    assert full[7][1] == 255 and full[7][2] == 31 and full[9][1] == 256 and full[9][2] is None, (full[7][1:3], full[9][1:3])
    w = header_shape("widths")[2]
    assert w[200][1] == 70 and set(w[200][3]) == {0} and len(w[200][3]) == 9, w[200][1:]            # groups of eight, all of zero width
    assert w[199][1] == 11 and set(w[199][3]) == {0} and len(w[199][3]) == 2, w[199][1:]            # groups of six
    assert w[198][1] == 70 and 11 in w[198][3], w[198][1:]                                          # the dominant symbol's group: 8 x 11 bits
    assert w[197][2] == 0 and w[196][2] == 31, (w[197][1:3], w[196][1:3])
    assert min(counts("all_pairs")) >= 250 and counts("all_pairs").count(256) >= 128, sorted(counts("all_pairs"))[:8]
    assert min(counts("random_64k")) >= 128
    for name in ("small_alphabets", "full_alphabets", "widths", "all_pairs", "random_64k"):
        assert header_shape(name)[1] == 11 and 4096 <= len(dict(shaped_cases())[name]) <= (1 << 16), name


def _skew(rng, n):
    base = np.minimum(rng.geometric(0.12, n), 90).astype(np.uint8)
    v = (base + 31).astype(np.uint8)
    v[1:][base[:-1] < 3] = 32
    return v.tobytes()


OFFSET_BS = 4096


@functools.lru_cache(maxsize=None)
def offset_cases():
    """(name, bytes) of three blocks of 4 KiB each under NONE / ANS1, taken in the order of their seeds as long as a stream's chunk headers start at a bit
    offset mod 32 that no stream taken before has: with the one-block cases above the chunk headers then start at every offset mod 32"""
    seen = set(header_shape(name)[0] & 31 for name, d in shaped_cases() if len(d) > 32)
    out = []
    for seed in range(400):
        if len(seen) == 32:
            break
        data = _skew(np.random.default_rng(0x4F4646 + seed), 3 * OFFSET_BS - 5 * (seed % 7))
        bits = Bits(O.compress(data, "NONE", "ANS1", OFFSET_BS))
        offs = set(chunk_start(bits, p)[0] & 31 for _f, p, _n in block_payloads(bits))
        if not offs <= seen:
            seen |= offs
            out.append(("offsets_%d" % seed, data))
    assert len(seen) == 32, sorted(seen)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def chain_cases():
    """(name, bytes) of three blocks of 16 KiB for BWT+RANK+ZRLT / ANS1"""
    rng = np.random.default_rng(0x434841)
    return (("chain_text", P.corpus(3 * CHAIN_BS, seed=11)), ("chain_random", rng.integers(0, 256, 3 * CHAIN_BS - 77, dtype=np.uint8).tobytes()))


@functools.lru_cache(maxsize=None)
def two_chunk_case():
    """4 MiB + 4099 bytes in one block: the second chunk is found through the first's header and size varint"""
    rng = np.random.default_rng(0x32434B)
    return _skew(rng, TWO_CHUNKS)


def _case(name):
    if name == "two_chunks":
        return two_chunk_case(), "NONE", 8 << 20
    for cases, transform, bs in ((shaped_cases(), "NONE", SHAPED_BS), (chain_cases(), "BWT+RANK+ZRLT", CHAIN_BS)):
        for nm, d in cases:
            if nm == name:
                return d, transform, bs
    return dict(offset_cases())[name], "NONE", OFFSET_BS


@functools.lru_cache(maxsize=None)
def oracle_stream(name):
    data, transform, bs = _case(name)
    return O.compress(data, transform, "ANS1", bs)


# ---- damaged headers ----------------------------------------------------------------------------------------------------------------------------
def _put(stream, pos, n, v):
    b = np.unpackbits(np.frombuffer(stream, dtype=np.uint8))
    b[pos:pos + n] = [(v >> (n - 1 - i)) & 1 for i in range(n)]
    return np.packbits(b).tobytes()


@functools.lru_cache(maxsize=None)
def damaged_streams():
    """(name, stream) made from the oracle's stream of `widths` (one block, one chunk)"""
    stream = oracle_stream("widths")
    at, lr, ctxs, end = header_shape("widths")
    assert lr == 11
    first = next(c for c in ctxs if c[1] > 1)                   # the first context with a group
    wpos = first[0] + (2 if first[2] is None else 6 + 8 * (first[2] + 1))
    bits = Bits(stream)
    (frame, payload, written), = block_payloads(bits)
    lw = bits.get(frame, 5) + 3
    keep = (ctxs[128][0] - payload) & ~7                        # the block ends in the middle of the header
    b = np.unpackbits(np.frombuffer(stream, dtype=np.uint8))
    cut = np.concatenate([b[:frame + 5], [(keep >> (lw - 1 - i)) & 1 for i in range(lw)], b[payload:payload + keep], np.zeros(8 + (-(frame + 5 + lw + keep)) % 8, dtype=np.uint8)])
    return (
        # the three-bit field holds 0..7 (lr 8..15), so no stream reaches the walk's own lr > 16 test. This case takes the largest value: a header that BOTH walks
        # accept (lr <= 16, the same width of the group fields) and the table kernel behind them refuses (lr != 11). It guards that the two walks agree on
        # such a header, positions included (the table kernel checks them), not the walk's error path
        ("lr_15", _put(stream, at, 3, 7)),
        ("width_above_lr", _put(stream, wpos, 4, 15)),
        ("cut_short", np.packbits(cut.astype(np.uint8)).tobytes()),
        ("size_2p27", _put(stream, end, 32, 0x80808040)),      # the varint of 1 << 27 (EntropyUtils.go:278-296), over the size and the first state
    )


# ---- the checks -----------------------------------------------------------------------------------------------------------------------------------
def _set_form(monkeypatch, form):
    monkeypatch.delenv(FORMS[1], raising=False)
    if form != "default":
        monkeypatch.setenv(form, "1")


def round_trip(be, monkeypatch, form, name):
    data, transform, bs = _case(name)
    exp = oracle_stream(name)
    n = len(data)
    _set_form(monkeypatch, form)
    try:
        c = K.Codec(transform, "ANS1", bs, lib=be.lib)
        src, _k0 = be.to_dev(data)
        cap = 2 * n + 262144 * (n // bs + 2)
        dst, kdst = be.empty(cap)
        nb = c.dev_compress(src, n, dst, cap)
        assert nb == len(exp) and be.to_host(kdst, nb) == exp, (name, form, "device stream != oracle stream", nb, len(exp))
        sp, _k1 = be.to_dev(exp, 4)
        out, kout = be.empty(n + 64)
        nd = c.dev_decompress(sp, len(exp), out, n + 64)
        assert nd == n and be.to_host(kout, nd) == data, (name, form, "decoded bytes != input")
        c.close()
    finally:
        _set_form(monkeypatch, "default")


def check_damaged(be, monkeypatch, name):
    """the device returns, and with the code the generic reader's walk gives. (lr_15 is a header both walks accept: there the code comes from the table kernel
    behind them, and the case guards that the two walks agree, not the walk's error path; see damaged_streams)"""
    stream = dict(damaged_streams())[name]
    n = len(dict(shaped_cases())["widths"])
    codes = []
    for form in FORMS:
        _set_form(monkeypatch, form)
        try:
            c = K.Codec("NONE", "ANS1", SHAPED_BS, lib=be.lib)
            sp, _k = be.to_dev(stream, 4)
            out, _ko = be.empty(n + 64)
            try:
                c.dev_decompress(sp, len(stream), out, n + 64)
                codes.append(0)
            except K.KnzError as e:
                codes.append(e.code)
            c.close()
        finally:
            _set_form(monkeypatch, "default")
    assert codes[0] == codes[1] == ERR_PROCESS_BLOCK, (name, codes)
