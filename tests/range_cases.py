"""knz_dev_stream_index / knz_dev_decompress_range / knz_dev_decompress_many_range: the index of a .knz stream and the decode of a range of its
blocks. Cases shared by the emulator run (tests/test_range_emu.py) and the MI355X run (tests/test_range_gpu.py). The checkers are the reference's
own Writer and Reader (oracle/_ref through tests/ref_lib.py): the expected bytes of a range are the slice of R.decompress(stream) at the block
boundaries (multiples of the block size for a stream the reference's Writer wrote, the known segment lengths for the short-inner-block stream),
and the index is checked against a framing walk in plain Python (frames(), many_cases.stream_end_bit extended to every frame)."""
import ctypes as C
import functools

import numpy as np

import geometry_cases as G
import many_cases as M
import parity_cases as P
import ref_lib as R

K = P.K
END = None                                                                  # to_block: through the last block (KNZ_BLOCK_END)
assert K.api.BLOCK_END == 0xFFFFFFFF                                        # (the binding of the range calls: nothing here runs without it)
ERR_MISSING_PARAM, ERR_WRITE_FILE, ERR_PROCESS_BLOCK, ERR_INVALID_PARAM, ERR_CRC_CHECK = 1, 12, 13, 18, 19

# (transform, entropy, checksum bits, -s)
PIPELINES = (("NONE", "NONE", 0, False), ("NONE", "HUFFMAN", 32, False), ("LZ", "ANS0", 0, False), ("BWT+RANK+ZRLT", "ANS1", 64, False),
             ("TEXT+UTF+BWT+RANK+ZRLT", "ANS0", 0, False), ("DNA+LZ", "HUFFMAN", 0, False))
BLOCK_SIZES = (1024, 16400, 65552)                                          # the minimum ; a block that ends in a 16-byte chunk ; 64 KiB + 16
EMU_BLOCK_SIZES = BLOCK_SIZES[:2]
BLOCKS, TAIL = 37, 777
SKIP_PIPES = (("NONE", "HUFFMAN", 32, True), ("BWT+RANK+ZRLT", "ANS1", 64, True))
SHORT_PIPES = (("NONE", "HUFFMAN", 0, False), ("BWT+RANK+ZRLT", "ANS0", 0, False))
SHORT_BS = 1 << 14
SHORT_RANGES = ((1, 2), (1, 3), (2, 3), (2, 4), (3, 4), (3, END), (2, END), (1, END), (5, 6), (6, END))


def pipe_id(pipe):
    return f"{pipe[0]}-{pipe[1]}" + ("-s" if pipe[3] else "")


# ---- the framing walk in plain Python ---------------------------------------------------------------------------------------------------
def frames(stream):
    """header and framing of a .knz stream (CompressedStream.go:1316-1460, :1816-1852) -> (info dict as knz_stream_info without n_blocks,
    [(bit of the frame, bit of the payload, payload bits)], bit behind the end marker)"""
    b = M._bits
    ck = b(stream, 36, 2)
    sz = b(stream, 119, 2)
    pos = 121 + 16 * sz + 15 + 24
    info = {"transform": b(stream, 43, 48), "entropy": b(stream, 38, 5), "block_size": b(stream, 91, 28) << 4, "checksum_bits": (0, 32, 64)[ck],
            "bs_version": b(stream, 32, 4), "output_size": b(stream, 121, 16 * sz) if sz else 0, "header_bits": pos}
    out = []
    while True:
        lw = b(stream, pos, 5) + 3
        written = b(stream, pos + 5, lw)
        if written == 0:
            return info, out, pos + 5 + lw
        out.append((pos, pos + 5 + lw, written))
        pos += 5 + lw + written


def splice_streams(header_of, parts):
    """the header of stream header_of, the frames of every stream of parts back to back, one end marker: what knz_dev_assemble builds from segments"""
    hb = frames(header_of)[0]["header_bits"]
    acc, nbits = int.from_bytes(header_of, "big") >> (8 * len(header_of) - hb), hb
    for p in parts:
        info, fr, end = frames(p)
        lo, hi = info["header_bits"], (fr[-1][1] + fr[-1][2]) if fr else info["header_bits"]
        seg = (int.from_bytes(p, "big") >> (8 * len(p) - hi)) & ((1 << (hi - lo)) - 1)
        acc, nbits = (acc << (hi - lo)) | seg, nbits + hi - lo
    acc, nbits = acc << 8, nbits + 8
    pad = -nbits % 8
    return (acc << pad).to_bytes((nbits + pad) // 8, "big")


# ---- streams, computed once ----------------------------------------------------------------------------------------------------------------
def _ref(pipe, bs, data, hs=None):
    t, e, ck, skip = pipe
    return R.compress(data, t, e, bs, ck, header_size=hs, skip_blocks=skip)


def _bounds(n, bs):
    return list(range(0, n, bs)) + [n]


@functools.lru_cache(maxsize=None)
def main_stream(pipe, bs, blocks=BLOCKS, tail=TAIL):
    """(data, the reference Writer's stream, block boundaries): `blocks` full blocks and a ragged one"""
    return sized_stream(pipe, bs, blocks * bs + tail)


@functools.lru_cache(maxsize=None)
def sized_stream(pipe, bs, n):
    """... of n bytes: one block exactly (n = bs), the empty input (header + end marker)"""
    data = G.make_input(pipe[0], n, 3) if n else b""
    stream = _ref(pipe, bs, data)
    assert R.decompress(stream, n + 64) == data
    return data, stream, _bounds(n, bs) if n else [0]


@functools.lru_cache(maxsize=None)
def skip_stream(pipe, bs=1024):
    """text blocks with incompressible ones between them under -s: the Writer turns those into copy blocks"""
    rng = np.random.default_rng(5)
    text = P.corpus(3 * bs, 9)
    data = b"".join(text[i * bs:(i + 1) * bs] if i % 3 != 1 else rng.integers(0, 256, bs, dtype=np.uint8).tobytes() for i in range(9)) + text[:TAIL]
    stream = _ref(pipe, bs, data)
    assert R.decompress(stream, len(data) + 64) == data
    return data, stream, _bounds(len(data), bs)


def copy_blocks(stream):
    """block ids (from 1) whose mode byte carries _COPY_BLOCK_MASK"""
    return [i + 1 for i, (_f, p, _n) in enumerate(frames(stream)[1]) if M._bits(stream, p, 8) & 0x80]


def short_parts(bs=SHORT_BS):
    return P.corpus(bs + 4321, 7), P.corpus(2 * bs + 99, 8)


@functools.lru_cache(maxsize=None)
def short_inner_stream(pipe, bs=SHORT_BS):
    """many_cases.check_short_inner's stream from the reference's outputs alone: the frames of two streams behind one header. Block 2 is short."""
    a, b = short_parts(bs)
    n = len(a) + len(b)
    stream = splice_streams(_ref(pipe, bs, a + b, n), [_ref(pipe, bs, a), _ref(pipe, bs, b)])
    assert R.decompress(stream, n + 64) == a + b
    return a + b, stream, [0, bs, len(a), len(a) + bs, len(a) + 2 * bs, n]


def device_short_inner(be, pipe, bs=SHORT_BS):
    """... and as many_cases.check_short_inner builds it: two knz_dev_compress_blocks segments joined by knz_dev_assemble. The same bytes."""
    a, b = short_parts(bs)
    c = M.codec_for(be, pipe, bs)
    segs, bits, keep = [], [], []
    for part in (a, b):
        src, ks = be.to_dev(part)
        cap = 2 * len(part) + 65536
        dst, kd = be.empty(cap)
        bits.append(c.dev_compress_blocks(src, len(part), dst, cap))
        segs.append(dst)
        keep += [ks, kd]
    n = len(a) + len(b)
    out, kout = be.empty(2 * n + 65536)
    total = c.dev_assemble(n, segs, bits, out, 2 * n + 65536)
    got = be.to_host(kout, total)
    c.close()
    data, stream, bounds = short_inner_stream(pipe, bs)
    assert got == stream, ("knz_dev_assemble's stream != the splice of the reference's frames", M._diff(got, stream))
    return data, stream, bounds


def ranges_of(n):
    """the ranges of a stream of n blocks: (from, to), ids from 1, to exclusive, END = through the last block"""
    k = max(1, n // 2)
    rs = [(1, 2), (1, END), (n, n + 1), (n, END), (k, k + 1), (k, k + 5), (2, n), (n + 1, END), (n + 5, END), (3, n + 40)]
    out = []
    for f, t in rs:
        if f >= 1 and (t is END or t > f) and (f, t) not in out:
            out.append((f, t))
    return out


def span(rng, n):
    """(first, behind the last) block index from 0 of a range over n blocks, clamped"""
    f, t = rng
    hi = n if t is END else min(t - 1, n)
    lo = min(f - 1, hi)
    return lo, hi


def expected(data, bounds, rng):
    lo, hi = span(rng, len(bounds) - 1)
    return data[bounds[lo]:bounds[hi]]


# ---- coverage guard: the reference's streams and the Python walk alone ----------------------------------------------------------------------
def check_coverage(block_sizes=EMU_BLOCK_SIZES):
    first8 = first32 = shared = widths = one = ragged = False
    for bs in block_sizes:
        for pipe in PIPELINES:
            _d, stream, bounds = main_stream(pipe, bs)
            _i, fr, _e = frames(stream)
            n = len(bounds) - 1
            assert n == len(fr) == BLOCKS + 1
            for rng in ranges_of(n):
                lo, hi = span(rng, n)
                if hi <= lo:
                    continue
                first8 |= fr[lo][0] % 8 != 0
                first32 |= fr[lo][0] % 32 != 0
                end = fr[hi - 1][1] + fr[hi - 1][2]
                shared |= hi < n and end % 32 != 0 and fr[hi][0] == end
                one |= hi - lo == 1
                ragged |= hi == n and bounds[n] - bounds[n - 1] == TAIL
            widths |= any(a[1] - a[0] != b[1] - b[0] for a, b in zip(fr, fr[1:]))
    assert first8 and first32, "no range starts at a frame off a byte / off a 32-bit word"
    assert shared, "no range ends inside a word that the next frame shares"
    assert widths, "no two neighbouring frames with length fields of different widths"
    assert one and ragged
    for pipe in SKIP_PIPES:
        _d, stream, bounds = skip_stream(pipe)
        cp = copy_blocks(stream)
        n = len(bounds) - 1
        assert cp and len(cp) < n, (pipe, cp)
        assert any(span(r, n)[0] < c <= span(r, n)[1] for r in ranges_of(n) for c in cp), "no copy block inside a range"
    for pipe in SHORT_PIPES:
        _d, stream, bounds = short_inner_stream(pipe)
        lens = [b - a for a, b in zip(bounds, bounds[1:])]
        assert len(frames(stream)[1]) == 5 and lens[1] < SHORT_BS and lens[2] == SHORT_BS, lens      # a short block with a full one behind it
        n = len(lens)
        assert any(span(r, n)[1] == 1 for r in SHORT_RANGES) and any(span(r, n)[0] == 2 for r in SHORT_RANGES)      # ranges on either side of it
        assert any(span(r, n)[0] <= 1 < span(r, n)[1] - 1 for r in SHORT_RANGES)                                   # ... and across it


# ---- device calls ------------------------------------------------------------------------------------------------------------------------
def range_call(be, codec, sp, nbytes, cap, rng, from_bit=0):
    """knz_dev_decompress_range into a destination of exactly cap bytes with 256 guard bytes behind it -> (bytes or None, status)"""
    dst, kd = M._guarded(be, cap)
    try:
        nb = codec.dev_decompress_range(sp, nbytes, dst, cap, rng[0], rng[1], from_bit)
    except K.KnzError as e:
        be.sync()
        assert M._guard_intact(be, kd, cap), "bytes behind dst_cap were written by a call that failed"
        return None, e.code
    be.sync()
    assert M._guard_intact(be, kd, cap), "bytes behind dst_cap were written"
    assert nb <= cap
    return be.to_host(kd, nb), 0


def full_call(be, codec, sp, nbytes, cap):
    dst, kd = M._guarded(be, cap)
    try:
        nb = codec.dev_decompress(sp, nbytes, dst, cap)
    except K.KnzError as e:
        return None, e.code
    be.sync()
    return be.to_host(kd, nb), 0


# ---- 1. index ------------------------------------------------------------------------------------------------------------------------------
def check_index(be, pipe, bs):
    t, e, ck, _s = pipe
    codec = M.codec_for(be, pipe, bs)
    data, big, _b = main_stream(pipe, bs)
    cases = [(big, len(data))]                                              # size field of 16 or 32 bits, then none, then the other width
    cases.append((_ref(pipe, bs, data[: 3 * bs + 5], 0), 0))
    small = data[:3000] if len(data) >= 65536 else G.make_input(t, 70_000, 5)
    cases.append((_ref(pipe, bs, small), len(small)))
    cases.append((_ref(pipe, bs, b""), 0))                                  # header + end marker
    widths = set()
    for stream, hs in cases:
        want, fr, end = frames(stream)
        widths.add(want["header_bits"])
        sp, _k = be.to_dev(stream, 4)
        info, pos = codec.dev_stream_index(sp, len(stream))
        assert {k: info[k] for k in want} == want, (pipe, bs, info, want)
        assert (info["transform"], info["entropy"], info["block_size"], info["checksum_bits"], info["output_size"]) == \
               (K.api.transform_type(t), K.api.entropy_type(e), bs, ck, hs), info
        assert info["n_blocks"] == len(fr) and pos == [(f, n) for f, _p, n in fr], (pipe, bs, info["n_blocks"], len(fr))
        assert info["end_bit"] == end and (end + 7) // 8 == len(stream), (info["end_bit"], end, len(stream))
        if fr:
            assert pos[0][0] == info["header_bits"]
        part = max(0, len(fr) - 3)
        info2, pos2 = codec.dev_stream_index(sp, len(stream), pos_cap=part)  # fewer rows than blocks: that many, and the true count
        assert info2 == info and pos2 == pos[:part]
        info3, pos3 = codec.dev_stream_index(sp, len(stream), pos_cap=0)     # pos = NULL
        assert info3 == info and pos3 == []
    assert len(widths) == 3, widths                                         # size fields of 0, 16 and 32 bits
    codec.close()


# ---- 2. range == slice, 3. hint invariance ----------------------------------------------------------------------------------------------------
def check_ranges(be, pipe, bs, case, ranges=None, hints=True, slack=0):
    """every range of the stream, walked from the header and from the index's bit: the slice of the reference Reader's bytes, counter 7 the blocks of
    the range. case: (data, stream, block boundaries). slack: room behind the range's bytes (a short inner block is packed after the decode)."""
    data, stream, bounds = case
    n = len(bounds) - 1
    codec = M.codec_for(be, pipe, bs)
    sp, _k = be.to_dev(stream, 4)
    _info, pos = codec.dev_stream_index(sp, len(stream))
    assert len(pos) == n
    ranges = ranges_of(n) if ranges is None else ranges
    if (1, END) in ranges:                                                  # {1, END, 0} is knz_dev_decompress
        whole, rc = full_call(be, codec, sp, len(stream), len(data) + slack)
        assert rc == 0 and whole == data and codec.last_counter(7) == n, (pipe, bs, rc, codec.last_counter(7), n)
    for rng in ranges:
        lo, hi = span(rng, n)
        exp = expected(data, bounds, rng)
        for hint in ((False, True) if hints and rng[0] <= n else (False,)):
            got, rc = range_call(be, codec, sp, len(stream), len(exp) + slack, rng, pos[rng[0] - 1][0] if hint else 0)
            assert rc == 0 and got == exp, (pipe, bs, rng, hint, rc, None if got is None else M._diff(got, exp))
            assert codec.last_counter(7) == hi - lo, (pipe, bs, rng, hint, codec.last_counter(7), hi - lo)
        if rng == (1, END):
            assert exp == whole
    codec.close()


def check_hints(be, pipe=PIPELINES[1], bs=1024):
    """hints outside the blocks are refused; one moved by a bit into the stream comes back with an error code or bytes that fail their checksum,
    never (checksum 32 on) as wrong bytes, and never writes behind dst_cap"""
    assert pipe[2] == 32
    data, stream, bounds = main_stream(pipe, bs)
    n = len(bounds) - 1
    info, fr, _end = frames(stream)
    codec = M.codec_for(be, pipe, bs)
    sp, _k = be.to_dev(stream, 4)
    for bad in (1, info["header_bits"] - 1, 8 * len(stream), 8 * len(stream) + 5, 1 << 40):
        got, rc = range_call(be, codec, sp, len(stream), 4 * bs, (2, 4), bad)
        assert rc == ERR_INVALID_PARAM and got is None, (bad, rc)
    got, rc = range_call(be, codec, sp, len(stream), 4 * bs, (1, 3), info["header_bits"])          # the smallest hint that is one
    assert rc == 0 and got == data[: 2 * bs]
    for blk in (2, n // 2, n):
        for off in (1, -1, 7, 13, fr[blk - 1][1] - fr[blk - 1][0], 200):
            hint = fr[blk - 1][0] + off
            exp = expected(data, bounds, (blk, blk + 2))
            got, rc = range_call(be, codec, sp, len(stream), 2 * bs, (blk, blk + 2), hint)
            assert rc != 0 or got == exp, (blk, off, "a wrong hint came back as wrong bytes")
            assert rc != 0, (blk, off, "a hint inside a payload decoded")  # (with a 32-bit checksum per block a chance hit is out of reach)
    codec.close()


# ---- 4. capacity, pointers at the minimum alignments ------------------------------------------------------------------------------------------
def check_capacity(be, pipe, bs):
    data, stream, bounds = main_stream(pipe, bs)
    n = len(bounds) - 1
    codec = M.codec_for(be, pipe, bs)
    for i, pl in enumerate(G.PLACEMENTS):
        _osrc, _odst, o_str, o_out = pl
        rng = ((n - 1, END), (2, 4), (n, n + 1), (1, 2), (3, n + 40))[i]
        exp = expected(data, bounds, rng)
        sp, _ks = G.place_stream(be, stream, o_str)
        out, kout, _ = G.place(be, len(exp), o_out)
        nb = codec.dev_decompress_range(sp, len(stream), out, len(exp), rng[0], rng[1])
        assert nb == len(exp) and G.fetch(be, kout, nb) == exp, (pipe, bs, pl, rng)
        G.guards_intact(be, kout, len(exp))
        out, kout, _ = G.place(be, len(exp) - 1, o_out)
        try:
            codec.dev_decompress_range(sp, len(stream), out, len(exp) - 1, rng[0], rng[1])
            raise AssertionError((pipe, bs, pl, rng, "a destination one byte short was accepted"))
        except K.KnzError as e:
            assert e.code == ERR_WRITE_FILE, e.code
        G.guards_intact(be, kout, len(exp) - 1)
    codec.close()


# ---- 5. damage -------------------------------------------------------------------------------------------------------------------------------
def check_damage(be, pipe=PIPELINES[1], bs=1024):
    assert pipe[2] == 32
    data, stream, bounds = main_stream(pipe, bs)
    n = len(bounds) - 1
    _info, fr, _end = frames(stream)
    codec = M.codec_for(be, pipe, bs)

    def flipped(blk):
        b = bytearray(stream)
        b[(fr[blk - 1][1] + fr[blk - 1][2] // 2) // 8] ^= 0x10             # the middle of block blk's payload
        return bytes(b)

    rng = (10, 14)
    exp = expected(data, bounds, rng)
    for blk in (3, 9, 14, n):                                               # a payload byte flipped outside the range: the same bytes
        sp, _k = be.to_dev(flipped(blk), 4)
        got, rc = range_call(be, codec, sp, len(stream), len(exp), rng)
        assert rc == 0 and got == exp, (blk, rc)
    for blk in (10, 13):                                                    # ... inside it: the code of the whole decode
        bad = flipped(blk)
        sp, _k = be.to_dev(bad, 4)
        _w, want = full_call(be, codec, sp, len(bad), len(data) + 64)
        got, rc = range_call(be, codec, sp, len(bad), len(exp), rng)
        assert want != 0 and rc == want and got is None, (blk, rc, want)
    cut = stream[: (fr[5][1] + fr[5][2] // 2) // 8]                         # cut inside block 6, in front of the range: the code of the whole decode
    sp, _k = be.to_dev(cut, 4)
    _w, want = full_call(be, codec, sp, len(cut), len(data) + 64)
    got, rc = range_call(be, codec, sp, len(cut), len(exp), rng)
    assert want != 0 and rc == want, (rc, want)
    cut = stream[: (fr[13][0] + 7) // 8]                                    # cut behind the range (in front of block 14's frame): success
    sp, _k = be.to_dev(cut, 4)
    assert full_call(be, codec, sp, len(cut), len(data) + 64)[1] != 0
    got, rc = range_call(be, codec, sp, len(cut), len(exp), rng)
    assert rc == 0 and got == exp, rc
    codec.close()


def check_contract(be):
    """bad arguments, through ctypes on the library itself: the codes check_entry_contract pins for knz_dev_decompress / knz_dev_decompress_many"""
    pipe, bs = PIPELINES[1], 1024
    data, stream, _b = main_stream(pipe, bs)
    one = M.codec_for(be, pipe, bs)
    two = M.codec_for(be, pipe, bs, devices=[0, 0])
    L = one.L
    Range, Stream, Info = K.api._BlockRange, K.api._Stream, K.api._StreamInfo
    sp, _k = be.to_dev(stream, 4)
    back, _kb = be.empty(len(data) + 64)
    out, info = C.c_uint64(), Info()
    o, cap = C.byref(out), len(data) + 64
    good = Range(2, 4, 0)
    assert L.knz_dev_decompress_range(None, sp, len(stream), C.byref(good), back, cap, o, None) == ERR_MISSING_PARAM
    assert L.knz_dev_stream_index(None, sp, len(stream), C.byref(info), None, 0, None) == ERR_MISSING_PARAM
    st1 = (Stream * 1)()
    st1[0].d_src, st1[0].n, st1[0].d_dst, st1[0].dst_cap = sp, len(stream), back, cap
    assert L.knz_dev_decompress_many_range(None, st1, C.byref(good), 1, None) == ERR_MISSING_PARAM
    for c in (one, two):
        h = c.h
        assert L.knz_dev_decompress_range(h, sp, len(stream), None, back, cap, o, None) == ERR_MISSING_PARAM
        assert L.knz_dev_decompress_range(h, None, len(stream), C.byref(good), back, cap, o, None) == ERR_MISSING_PARAM
        assert L.knz_dev_decompress_range(h, sp, len(stream), C.byref(good), None, cap, o, None) == ERR_MISSING_PARAM
        assert L.knz_dev_decompress_range(h, sp, len(stream), C.byref(good), back, cap, None, None) == ERR_MISSING_PARAM
        assert L.knz_dev_stream_index(h, None, len(stream), C.byref(info), None, 0, None) == ERR_MISSING_PARAM
        assert L.knz_dev_stream_index(h, sp, len(stream), None, None, 0, None) == ERR_MISSING_PARAM
        assert L.knz_dev_decompress_many_range(h, None, C.byref(good), 1, None) == ERR_MISSING_PARAM
        assert L.knz_dev_decompress_many_range(h, st1, None, 1, None) == ERR_MISSING_PARAM
        assert L.knz_dev_decompress_many_range(h, st1, None, 0, None) == 0 and L.knz_dev_decompress_many_range(h, None, None, -1, None) == 0
        assert L.knz_dev_decompress_range(h, sp + 1, len(stream) - 1, C.byref(good), back, cap, o, None) == ERR_INVALID_PARAM
        assert L.knz_dev_stream_index(h, sp + 1, len(stream) - 1, C.byref(info), None, 0, None) == ERR_INVALID_PARAM
        for f, t in ((0, 3), (0, 0xFFFFFFFF), (3, 3), (4, 2), (0xFFFFFFFF, 0xFFFFFFFF)):
            bad = Range(f, t, 0)
            assert L.knz_dev_decompress_range(h, sp, len(stream), C.byref(bad), back, cap, o, None) == ERR_INVALID_PARAM, (f, t)
            assert L.knz_dev_decompress_many_range(h, st1, C.byref(bad), 1, None) == ERR_INVALID_PARAM and st1[0].status == ERR_INVALID_PARAM
        st1[0].d_src = sp + 1
        assert L.knz_dev_decompress_many_range(h, st1, C.byref(good), 1, None) == ERR_INVALID_PARAM and st1[0].status == ERR_INVALID_PARAM
        st1[0].d_src = sp
        assert L.knz_dev_decompress_range(h, sp, len(stream), C.byref(good), back, cap, o, None) == 0 and out.value == 2 * bs   # the handles still work
        assert be.to_host(_kb, 2 * bs) == data[bs: 3 * bs]
    assert L.knz_last_counter(one.h, 7, o) == 0 and out.value == 2
    one.close()
    two.close()


# ---- 6. many form ----------------------------------------------------------------------------------------------------------------------------
def many_streams(pipe, bs):
    """five distinct streams of one configuration: (data, stream, block boundaries)"""
    out = [main_stream(pipe, bs)]
    for i, n in enumerate((bs, 5 * bs + 1, 2 * bs + 99, 11 * bs)):
        data = G.make_input(pipe[0], n, 11 + i)
        out.append((data, _ref(pipe, bs, data, 0 if i % 2 else None), _bounds(n, bs)))
    return out


def many_range_call(be, codec, entries):
    """entries: [(device stream pointer, stream bytes, dst_cap, range, from_bit)] -> ([(bytes or None, status)], return code)"""
    keep, call = [], []
    for sp, nbytes, cap, rng, bit in entries:
        dst, kd = M._guarded(be, cap)
        keep.append((kd, cap))
        call.append((sp, nbytes, dst, cap, rng[0], rng[1], bit))
    res = codec.dev_decompress_many_range(call)
    be.sync()
    out = []
    for (nb, status), (kd, cap) in zip(res, keep):
        assert M._guard_intact(be, kd, cap), "bytes behind a dst_cap were written"
        assert nb <= cap
        out.append((be.to_host(kd, nb) if status == 0 else None, status))
    return out, codec.last_many_rc


def check_many(be, pipe, bs, k, lanes=None):
    """k entries over five streams (the same d_src several times), ranges from the list; with k >= 7 one entry damaged inside its range and one with a
    destination a byte short. Every entry equals its single call, the return value is the first failing entry's status, counter 7 the sum."""
    assert pipe[2] != 0
    streams = many_streams(pipe, bs)
    codec = M.codec_for(be, pipe, bs, **({"devices": lanes} if lanes else {}))
    single = M.codec_for(be, pipe, bs)
    dev = []
    for data, stream, bounds in streams:
        sp, keep = be.to_dev(stream, 4)
        _i, pos = single.dev_stream_index(sp, len(stream))
        dev.append((sp, keep, pos))
    data0, stream0, bounds0 = streams[0]
    fr0 = frames(stream0)[1]
    hurt = bytearray(stream0)
    hurt[(fr0[4][1] + fr0[4][2] // 2) // 8] ^= 0x10                         # the middle of block 5's payload
    hp, _hk = be.to_dev(bytes(hurt), 4)
    entries, want, blocks = [], [], 0
    for j in range(k):
        s = (j * 3) % len(streams)
        data, stream, bounds = streams[s]
        n = len(bounds) - 1
        rs = ranges_of(n)
        rng = rs[(j * 7 + j // len(streams)) % len(rs)]
        exp = expected(data, bounds, rng)
        sp, nbytes, cap, bit = dev[s][0], len(stream), len(exp), (dev[s][2][rng[0] - 1][0] if (j % 2 and rng[0] <= n) else 0)
        if k >= 7 and j == 2:
            sp, nbytes, n, rng, bit = hp, len(stream0), len(bounds0) - 1, (4, 7), 0     # damage inside the range
            exp, cap = None, 3 * bs
        if k >= 7 and j == 5:
            rng, bit = (1, 3), 0
            exp, cap = None, min(2 * bs, len(data)) - 1                     # a destination one byte short
        entries.append((sp, nbytes, cap, rng, bit))
        want.append(exp)
        lo, hi = span(rng, n)
        blocks += hi - lo
    got, rc = many_range_call(be, codec, entries)
    for j, ((g, s), exp, ent) in enumerate(zip(got, want, entries)):
        sg, ss = range_call(be, single, ent[0], ent[1], ent[2], ent[3], ent[4])
        assert (g, s) == (sg, ss), (pipe, bs, k, j, ent[3], s, ss, "entry of the many call != its single call")
        if exp is not None:
            assert s == 0 and g == exp, (pipe, bs, k, j, ent[3], s)
        else:
            assert s != 0
    if k >= 7:
        assert got[5][1] == ERR_WRITE_FILE and got[2][1] != 0
    assert rc == M.first_failure(got), (rc, [s for _g, s in got])
    if not lanes:
        assert codec.last_counter(7) == blocks, (codec.last_counter(7), blocks)
    assert codec.dev_decompress_many_range([]) == [] and codec.last_many_rc == 0
    codec.close()
    single.close()


# ---- 7. the fused ZRLT / RANK chain ------------------------------------------------------------------------------------------------------------
def check_fused_chain(be, bs=G.BLOCK_SIZES[0]):
    """BWT+RANK+ZRLT&ANS1 at the smallest block size at which geometry_cases sees the fused chain taken: a range that does not start at block 1
    takes it too"""
    pipe = ("BWT+RANK+ZRLT", "ANS1", 0, False)
    n = 4 * bs + G.TAIL
    data, stream = G.make_input(pipe[0], n, 3), G.expected(pipe[0], pipe[1], bs, n, 3)
    bounds = _bounds(n, bs)
    codec = M.codec_for(be, pipe, bs)
    sp, _k = be.to_dev(stream, 4)
    for rng in ((2, 4), (3, END), (4, 5)):
        exp = expected(data, bounds, rng)
        got, rc = range_call(be, codec, sp, len(stream), len(exp), rng)
        assert rc == 0 and got == exp, (rng, rc)
        assert codec.last_counter(6) >= 1, (rng, "no block of the range took the fused chain")
        lo, hi = span(rng, 5)
        assert codec.last_counter(7) == hi - lo
    codec.close()
