"""knz_dev_read_many / knz_dev_read: byte reads (source, offset, length) from .knz streams into destinations of any alignment. Cases shared by the
emulator run (tests/test_read_emu.py) and the MI355X run (tests/test_read_gpu.py). Streams and helpers are range_cases': the reference's own Writer
wrote them and its Reader (oracle/_ref through tests/ref_lib.py) decodes them to `data` there, so the expected bytes of a read are always
data[offset : offset + length] (for the short-inner-block stream: the rule of include/knz_gpu.h over the known segment lengths).

Every destination lies in one arena filled with a known byte, 32 guard bytes on both sides of each (the destinations themselves are pre-filled with
it too): after each call the whole arena is fetched and everything but the bytes [0, out_bytes) of every read has to be that byte still."""
import ctypes as C

import numpy as np

import many_cases as M
import range_cases as RC

K = RC.K
GUARD, FILL = 32, 0xA5
ERR_MISSING_PARAM, ERR_INVALID_PARAM = RC.ERR_MISSING_PARAM, RC.ERR_INVALID_PARAM
GRID_PIPE, GRID_BS = RC.PIPELINES[1], 1024                                   # NONE&HUFFMAN/32
GRID_LENGTHS = (0, 1, 3, 15, 16, 17, 31, 32, 33, 47, 100)
XF_PIPE = RC.PIPELINES[3]                                                    # BWT+RANK+ZRLT&ANS1/64


# ---- what a read has to deliver --------------------------------------------------------------------------------------------------------------
def block_lens(bounds):
    return [b - a for a, b in zip(bounds, bounds[1:])]


def expected(data, bounds, bs, offset, length):
    """bytes in order from block offset // bs at offset % bs until the length is served or a block that decoded to fewer than bs bytes ends"""
    lens = block_lens(bounds)
    b, w, out = offset // bs, offset % bs, b""
    while length > 0 and b < len(lens) and w < lens[b]:
        take = min(length, lens[b] - w)
        out += data[bounds[b] + w: bounds[b] + w + take]
        length -= take
        if lens[b] < bs:
            break
        b, w = b + 1, 0
    return out


def writer_expected(data, bounds, bs, offset, length):
    """... of a stream a Writer wrote (only the last block short): the slice of the decoded stream"""
    exp = data[offset: offset + length]
    assert exp == expected(data, bounds, bs, offset, length)
    return exp


# ---- the case lists (pure: check_coverage looks at what they yield) ----------------------------------------------------------------------------
def grid_reads(n):
    """(offset, length, destination mod 16): every pairing of offset mod 16 and destination mod 16, the lengths cycling"""
    out = []
    for sm in range(16):
        for dm in range(16):
            i = sm * 16 + dm
            out.append((16 * ((i * 37) % (n // 16 - 8)) + sm, GRID_LENGTHS[i % len(GRID_LENGTHS)], dm))
    return out


def boundary_reads(n, bs):
    """n: decoded bytes of a main_stream (BLOCKS full blocks and TAIL bytes)"""
    assert n == RC.BLOCKS * bs + RC.TAIL
    return [(3 * bs - 100, 100, 3), (5 * bs, 50, 8), (2 * bs - 1, 2, 15), (bs - 2, 3 * bs + 5, 1), (0, n, 5), (RC.BLOCKS * bs + 700, 50, 9),
            (n - 10, 100, 2)]


def check_coverage():
    n = RC.BLOCKS * GRID_BS + RC.TAIL
    grid = grid_reads(n)
    assert {(o % 16, d) for o, _l, d in grid} == {(s, d) for s in range(16) for d in range(16)}, "not every (source mod 16, destination mod 16) pair"
    assert {l for _o, l, _d in grid} == set(GRID_LENGTHS)
    assert all(o + l <= n for o, l, _d in grid)
    for bs in RC.BLOCK_SIZES:
        n = RC.BLOCKS * bs + RC.TAIL
        rs = boundary_reads(n, bs)
        assert any((o + l - 1) // bs - o // bs > 1 for o, l, _d in rs), "no read across more than one block boundary"
        assert any(o < n < o + l for o, l, _d in rs), "no read that ends short"
        assert any((o + l) % bs == 0 for o, l, _d in rs) and any(o % bs == 0 and l < bs for o, l, _d in rs)
        assert any(o // bs == RC.BLOCKS and o + l <= n for o, l, _d in rs), "no read inside the ragged last block"


# ---- device calls ------------------------------------------------------------------------------------------------------------------------------
def _view(be, keep):
    return keep[1] if be.name == "emu" else keep


def read_call(be, codec, sources, reads, packed_from=None):
    """sources: [(device pointer, stream bytes[, index rows])] ; reads: [(source, offset, length, destination mod 16)]. The destinations get GUARD bytes
    on both sides (packed_from = m: they follow each other to the byte, the first at an address = m mod 16). -> ([(bytes, status)], return code).
    Asserts that nothing but the bytes [0, out_bytes) of every read has changed."""
    at, cur = [], GUARD
    for _s, _o, length, dm in reads:
        if packed_from is None:
            cur += GUARD
            cur += (dm - cur) % 16
        elif not at:
            cur += (packed_from - cur) % 16
        at.append(cur)
        cur += min(length, 1 << 24)                                         # (a length past any stream: the guard check covers what a stream can give)
    size = cur + 2 * GUARD
    ptr, keep = be.empty(size)
    assert ptr % 16 == 0
    _view(be, keep)[:size] = FILL
    res = codec.dev_read_many(sources, [(s, o, l, ptr + a) for (s, o, l, _d), a in zip(reads, at)])
    be.sync()
    got = be.to_host(keep, size)
    clean = bytearray(got)
    out = []
    for (nb, status), (_s, _o, length, _d), a in zip(res, reads, at):
        assert nb <= length and (status == 0 or nb == 0), (nb, length, status)
        out.append((got[a: a + nb], status))
        clean[a: a + nb] = bytes([FILL]) * nb
    bad = [i for i in np.flatnonzero(np.frombuffer(bytes(clean), dtype=np.uint8) != FILL)[:4]]
    assert not bad, ("bytes outside [0, out_bytes) of the reads were written", bad, at[:4])
    return out, codec.last_many_rc


def _dev(be, stream):
    return be.to_dev(stream, 4)


def _check_writer_reads(be, codec, case, bs, reads, index=None):
    data, stream, bounds = case
    sp, _k = _dev(be, stream)
    got, rc = read_call(be, codec, [(sp, len(stream), index)], [(0, o, l, d) for o, l, d in reads])
    for (g, s), (o, l, _d) in zip(got, reads):
        assert s == 0 and g == writer_expected(data, bounds, bs, o, l), (bs, o, l, s, M._diff(g, data[o: o + l]))
    assert rc == 0
    return got


# ---- 1. alignment grid, 2. packed destinations ---------------------------------------------------------------------------------------------------
def check_alignment_grid(be):
    case = RC.main_stream(GRID_PIPE, GRID_BS)
    codec = M.codec_for(be, GRID_PIPE, GRID_BS)
    _check_writer_reads(be, codec, case, GRID_BS, grid_reads(len(case[0])))
    codec.close()


def check_packed(be):
    data, stream, bounds = RC.main_stream(GRID_PIPE, GRID_BS)
    codec = M.codec_for(be, GRID_PIPE, GRID_BS)
    rng = np.random.default_rng(11)
    reads = [(0, int(rng.integers(0, len(data) - 64)), 1 + i % 40, 0) for i in range(300)]
    sp, _k = _dev(be, stream)
    got, rc = read_call(be, codec, [(sp, len(stream))], reads, packed_from=1)
    assert rc == 0 and all(s == 0 for _g, s in got)
    assert b"".join(g for g, _s in got) == b"".join(data[o: o + l] for _s, o, l, _d in reads)
    codec.close()


# ---- 3. block boundaries, 13. the single form ----------------------------------------------------------------------------------------------------
def check_boundaries(be, pipe, bs, lanes=None):
    case = RC.main_stream(pipe, bs)
    codec = M.codec_for(be, pipe, bs, **({"devices": lanes} if lanes else {}))
    got = _check_writer_reads(be, codec, case, bs, boundary_reads(len(case[0]), bs))
    codec.close()
    return got


def check_single(be, pipe=GRID_PIPE, bs=GRID_BS):
    data, stream, bounds = RC.main_stream(pipe, bs)
    codec = M.codec_for(be, pipe, bs)
    sp, _k = _dev(be, stream)
    reads = [r for r in boundary_reads(len(data), bs) if r[1] < len(data)][:5]
    assert len(reads) == 5
    many, _rc = read_call(be, codec, [(sp, len(stream))], [(0, o, l, d) for o, l, d in reads])
    for (o, l, dm), (g, s) in zip(reads, many):
        size = l + 2 * GUARD + 16
        ptr, keep = be.empty(size)
        _view(be, keep)[:size] = FILL
        nb = codec.dev_read(sp, len(stream), o, l, ptr + GUARD + dm)
        be.sync()
        back = be.to_host(keep, size)
        assert s == 0 and back[GUARD + dm: GUARD + dm + nb] == g == data[o: o + l], (o, l)
        assert back[: GUARD + dm] == bytes([FILL]) * (GUARD + dm) and back[GUARD + dm + nb:] == bytes([FILL]) * (size - GUARD - dm - nb)
    codec.close()


# ---- 4. end of stream ------------------------------------------------------------------------------------------------------------------------------
def check_end(be, pipe=GRID_PIPE, bs=GRID_BS):
    data, stream, bounds = RC.main_stream(pipe, bs)
    n = len(data)
    codec = M.codec_for(be, pipe, bs)
    sp, _k = _dev(be, stream)
    reads = [(0, n - 300, 1000, 3), (0, n, 10, 0), (0, n + 10 * bs, 10, 7), (0, 2 ** 40, 10, 1), (0, n - 1, 2 ** 40, 5), (0, 17, 0, 4)]
    got, rc = read_call(be, codec, [(sp, len(stream))], reads)
    assert rc == 0 and [s for _g, s in got] == [0] * len(reads)
    assert [g for g, _s in got] == [data[n - 300:], b"", b"", b"", data[n - 1:], b""]
    _d0, empty, _b0 = RC.sized_stream(pipe, bs, 0)
    ep, _ke = _dev(be, empty)
    got, rc = read_call(be, codec, [(ep, len(empty))], [(0, 0, 100, 0), (0, 5, 1, 3), (0, bs, 2 * bs, 9)])
    assert rc == 0 and got == [(b"", 0)] * 3, got
    assert codec.last_counter(7) == 0
    codec.close()


# ---- 5. every covering block decodes once ------------------------------------------------------------------------------------------------------------
def check_dedup(be, pipe=GRID_PIPE, bs=GRID_BS):
    data, stream, bounds = RC.main_stream(pipe, bs)
    codec = M.codec_for(be, pipe, bs)
    sp, _k = _dev(be, stream)
    src = [(sp, len(stream))]
    rng = np.random.default_rng(5)
    reads = [(0, 7 * bs + int(rng.integers(0, bs - 100)), int(rng.integers(1, 100)), i % 16) for i in range(64)]
    reads += [(0, 20 * bs + int(rng.integers(0, bs - 100)), int(rng.integers(1, 100)), i % 16) for i in range(8)]
    got, rc = read_call(be, codec, src, reads)
    assert rc == 0 and codec.last_counter(7) == 2, codec.last_counter(7)
    assert got == [(data[o: o + l], 0) for _s, o, l, _d in reads]
    reads = [(0, 10 * bs + 5, 2 * bs + 100, 6)] + [(0, (10 + i % 3) * bs + 13 * i + 5, 50 + i, i) for i in range(10)]
    got, rc = read_call(be, codec, src, reads)
    assert rc == 0 and codec.last_counter(7) == 3, codec.last_counter(7)
    assert got == [(data[o: o + l], 0) for _s, o, l, _d in reads]
    for r, g in zip(reads, got):                                            # each read issued alone: identical
        alone, rc = read_call(be, codec, src, [r])
        assert rc == 0 and alone == [g]
    # two rows with the same d_src are two sources: the same block once per source
    got, rc = read_call(be, codec, src * 2, [(0, 3 * bs + 1, 10, 0), (1, 3 * bs + 50, 10, 0)])
    assert rc == 0 and codec.last_counter(7) == 2 and got == [(data[3 * bs + 1: 3 * bs + 11], 0), (data[3 * bs + 50: 3 * bs + 60], 0)]
    codec.close()


# ---- 6. independence, 12. lanes --------------------------------------------------------------------------------------------------------------------
def mixed_reads(cases, bs, k, seed=9):
    """k reads over the sources: inside a block, across one and several boundaries, across the end, behind it, empty"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(k):
        s = i % len(cases)
        n = len(cases[s][0])
        kind = i % 6
        o = int(rng.integers(0, max(n - 1, 1)))
        l = (int(rng.integers(1, 200)), bs + int(rng.integers(1, bs)), 3 * bs + 7, 500, 10, 0)[kind]
        if kind == 3:
            o = max(n - 100, 0)
        if kind == 4:
            o = n + int(rng.integers(0, 3 * bs))
        out.append((s, o, l, int(rng.integers(0, 16))))
    return out


def check_independence(be, pipe=XF_PIPE, bs=1024, lanes=None):
    cases = [RC.main_stream(pipe, bs)] + RC.many_streams(pipe, bs)[2:4]
    codec = M.codec_for(be, pipe, bs, **({"devices": lanes} if lanes else {}))
    one = M.codec_for(be, pipe, bs)
    keep = [_dev(be, c[1]) for c in cases]
    src = [(k[0], len(c[1])) for k, c in zip(keep, cases)]
    reads = mixed_reads(cases, bs, 40)
    got, rc = read_call(be, codec, src, reads)
    assert rc == 0
    for (s, o, l, _d), (g, st) in zip(reads, got):
        assert st == 0 and g == writer_expected(cases[s][0], cases[s][2], bs, o, l), (s, o, l, st)
    back, rc = read_call(be, codec, src, reads[::-1])
    assert rc == 0 and back[::-1] == got, "the reversed read list gives other results"
    for r, g in zip(reads, got):
        alone, rc = read_call(be, one, [src[r[0]]], [(0,) + r[1:]])
        assert alone == [g], (r, "a read of the call != the same read alone")
    codec.close()
    one.close()


# ---- 7. short inner block ----------------------------------------------------------------------------------------------------------------------------
def check_short_inner(be, pipe):
    bs = RC.SHORT_BS
    data, stream, bounds = RC.device_short_inner(be, pipe)
    lens = block_lens(bounds)
    assert lens[0] == bs and lens[1] < bs and lens[2] == bs
    codec = M.codec_for(be, pipe, bs)
    sp, _k = _dev(be, stream)
    reads = [(0, bs - 100, 2 * bs + 500, 3),                                # from block 1 into block 3's territory: ends where block 2's bytes end
             (0, 2 * bs, 300, 11),                                          # addressed at block 3: block 3's bytes
             (0, bs + lens[1] - 5, 50, 6),                                  # the last 5 bytes of the short block
             (0, bs + lens[1], 50, 2), (0, bs + lens[1] + 77, 50, 0),       # behind the short block's decoded length: nothing
             (0, 2 * bs + bs - 3, 10, 9)]                                   # blocks 3 and 4 are full: across their boundary
    got, rc = read_call(be, codec, [(sp, len(stream))], reads)
    assert rc == 0 and [s for _g, s in got] == [0] * len(reads)
    want = [expected(data, bounds, bs, o, l) for _s, o, l, _d in reads]
    assert want[0] == data[bs - 100: bounds[2]] and len(want[0]) == 100 + lens[1]
    assert want[1] == data[bounds[2]: bounds[2] + 300] and want[2] == data[bounds[2] - 5: bounds[2]] and want[3] == want[4] == b""
    assert want[5] == data[bounds[3] - 3: bounds[3] + 7]
    assert [g for g, _s in got] == want, [M._diff(g, w) for (g, _s), w in zip(got, want)]
    codec.close()


# ---- 8. damage ------------------------------------------------------------------------------------------------------------------------------------------
def check_damage(be, pipe=GRID_PIPE, bs=GRID_BS):
    assert pipe[2] == 32
    data, stream, bounds = RC.main_stream(pipe, bs)
    _info, fr, _end = RC.frames(stream)
    hurt = bytearray(stream)
    hurt[(fr[4][1] + fr[4][2] // 2) // 8] ^= 0x10                           # the middle of block 5's payload
    codec = M.codec_for(be, pipe, bs)
    hp, _kh = _dev(be, bytes(hurt))
    sp, _ks = _dev(be, stream)
    _g, want = RC.range_call(be, codec, hp, len(hurt), bs, (5, 6))
    assert want != 0
    src = [(hp, len(hurt)), (sp, len(stream))]
    #        touch block 5 ...                                                            ... blocks 3, 4, 6, 20                          the clean source
    reads = [(0, 4 * bs + 10, 20, 1), (0, 3 * bs + 900, 300, 2), (0, 2 * bs, 4 * bs, 3), (0, 2 * bs + 7, 100, 4), (0, 3 * bs, bs, 5), (0, 5 * bs, 64, 6),
             (0, 19 * bs + 1, 999, 7), (1, 4 * bs + 10, 20, 8), (1, 2 * bs, 4 * bs, 9), (0, 5 * bs - 1, 1, 10), (0, 5 * bs - 1, 2, 11)]
    hit = [(o + l - 1) // bs >= 4 >= o // bs and s == 0 for s, o, l, _d in reads]
    assert sum(hit) == 5
    for rs in (reads, reads[3:] + reads[:3]):
        got, rc = read_call(be, codec, src, rs)
        h = [(o + l - 1) // bs >= 4 >= o // bs and s == 0 for s, o, l, _d in rs]
        for (s, o, l, _d), (g, st), bad in zip(rs, got, h):
            assert (g, st) == ((b"", want) if bad else (data[o: o + l], 0)), (s, o, l, st, want)
        assert rc == M.first_failure(got) == want
    # block 2's length field damaged: reads at blocks >= 3 that walk from the header fail with the walk's code, with the index of the undamaged stream they complete
    cut = bytearray(stream)
    cut[(fr[1][0] + 5) // 8] ^= 0x80 >> ((fr[1][0] + 5) % 8)               # (its leading bit: the walk lands inside block 2's payload)
    cp, _kc = _dev(be, bytes(cut))
    _i, pos = codec.dev_stream_index(sp, len(stream))
    reads = [(0, 10, 100, 1), (0, 2 * bs + 5, 100, 2), (0, 6 * bs - 3, 10, 3)]
    _g, walk = RC.range_call(be, codec, cp, len(cut), bs, (3, 4))
    got, rc = read_call(be, codec, [(cp, len(cut))], reads)
    assert walk != 0 and got == [(data[10:110], 0), (b"", walk), (b"", got[2][1])] and got[2][1] != 0 and rc == walk, (got, walk)
    got, rc = read_call(be, codec, [(cp, len(cut), pos)], reads)
    assert rc == 0 and got == [(data[o: o + l], 0) for _s, o, l, _d in reads]
    codec.close()


# ---- 9. hints -------------------------------------------------------------------------------------------------------------------------------------------
def check_hints(be, blocks=1500, pipe=GRID_PIPE, bs=GRID_BS):
    data, stream, bounds = RC.main_stream(pipe, bs, blocks)
    info, fr, _end = RC.frames(stream)
    codec = M.codec_for(be, pipe, bs)
    sp, _k = _dev(be, stream)
    _i, pos = codec.dev_stream_index(sp, len(stream))
    assert len(pos) == blocks + 1
    rng = np.random.default_rng(3)
    reads = [(0, int(rng.integers(0, len(data))), int(rng.integers(1, 3000)), int(rng.integers(0, 16))) for _ in range(199)] + [(0, 0, len(data), 3)]
    plain, rc = read_call(be, codec, [(sp, len(stream))], reads)
    assert rc == 0 and plain == [(data[o: o + l], 0) for _s, o, l, _d in reads]
    touched = codec.last_counter(7)
    assert touched == blocks + 1                                            # (the whole-stream read: every block, once)
    for rows in (pos, pos[:700]):
        got, rc = read_call(be, codec, [(sp, len(stream), rows)], reads)
        assert rc == 0 and got == plain and codec.last_counter(7) == touched
    few = [(0, 3 * bs + 5, 10, 1), (0, 8 * bs - 4, 8, 2), (0, 20 * bs, 100, 3)]      # blocks 4 ; 8 and 9 ; 21
    for bad in (8 * len(stream), 8 * len(stream) + 5, 1 << 40, info["header_bits"] - 1, 1, 0):
        rows = list(pos[:30])
        rows[7] = (bad, rows[7][1])                                         # block 8's hint
        got, rc = read_call(be, codec, [(sp, len(stream), rows)], few)
        assert got == [(data[o: o + l], 0) if i != 1 else (b"", ERR_INVALID_PARAM) for i, (_s, o, l, _d) in enumerate(few)], (bad, got)
        assert rc == ERR_INVALID_PARAM
    for off in (3, 1, 13, fr[7][1] - fr[7][0]):
        rows = list(pos[:30])
        rows[7] = (rows[7][0] + off, rows[7][1])
        got, rc = read_call(be, codec, [(sp, len(stream), rows)], few)      # it returns ; (the guards are read_call's)
        assert got[0] == (data[3 * bs + 5: 3 * bs + 15], 0) and got[2] == (data[20 * bs: 20 * bs + 100], 0)
        assert got[1][1] != 0 or len(got[1][0]) <= 8, got[1]
        assert got[1][1] != 0, (off, "a hint inside a frame decoded")       # (a 32-bit checksum per block: a chance hit is out of reach)
    codec.close()


# ---- 10. contract ---------------------------------------------------------------------------------------------------------------------------------------
def check_contract(be):
    pipe, bs = GRID_PIPE, GRID_BS
    data, stream, _b = RC.main_stream(pipe, bs)
    _d2, other, _b2 = RC.main_stream(RC.PIPELINES[2], bs)                   # another transform and entropy codec in the header
    codec = M.codec_for(be, pipe, bs)
    L = codec.L
    Source, Read = K.api._Source, K.api._Read
    sp, _k = _dev(be, stream)
    op, _ko = _dev(be, other)
    tp, _kt = _dev(be, stream[:10])
    back, kb = be.empty(4096)
    src, rd = (Source * 1)(), (Read * 1)()
    src[0].d_src, src[0].n = sp, len(stream)
    rd[0].source, rd[0].offset, rd[0].length, rd[0].d_dst = 0, 5, 10, back
    out = C.c_uint64()
    assert L.knz_dev_read_many(None, src, 1, rd, 1, None) == ERR_MISSING_PARAM
    assert L.knz_dev_read_many(codec.h, src, 1, rd, 0, None) == 0 and L.knz_dev_read_many(codec.h, None, 0, None, -1, None) == 0
    assert L.knz_dev_read_many(codec.h, None, 1, rd, 1, None) == ERR_MISSING_PARAM
    assert L.knz_dev_read_many(codec.h, src, 1, None, 1, None) == ERR_MISSING_PARAM
    assert L.knz_dev_read(codec.h, sp, len(stream), 0, 10, back, None, None) == ERR_MISSING_PARAM
    assert L.knz_dev_read(codec.h, sp, len(stream), 0, 10, None, C.byref(out), None) == ERR_MISSING_PARAM
    assert L.knz_dev_read(codec.h, None, len(stream), 0, 10, back, C.byref(out), None) == ERR_MISSING_PARAM
    assert L.knz_dev_read(codec.h, sp + 1, len(stream) - 1, 0, 10, back, C.byref(out), None) == ERR_INVALID_PARAM
    assert codec.dev_read_many([], []) == [] and codec.last_many_rc == 0
    srcs = [(sp, len(stream)), (op, len(other)), (tp, 10), (sp, len(stream))]
    reads = [(0, 5, 10, 0), (4, 5, 10, 1), (0, 2 ** 64 - 5, 10, 2), (1, 5, 10, 3), (2, 5, 10, 4), (3, bs - 1, 2, 5), (0, 2 ** 64 - 11, 10, 6)]
    got, rc = read_call(be, codec, srcs, reads)
    short = codec.last_source_status[2]
    assert short != 0 and codec.last_source_status == [0, ERR_INVALID_PARAM, short, 0]
    assert got == [(data[5:15], 0), (b"", ERR_INVALID_PARAM), (b"", ERR_INVALID_PARAM), (b"", ERR_INVALID_PARAM), (b"", short), (data[bs - 1: bs + 1], 0),
                   (b"", 0)], got
    assert rc == ERR_INVALID_PARAM
    try:
        codec.dev_read_many(srcs, [(s, o, l, back) for s, o, l, _d in reads], check=True)
        raise AssertionError("check=True did not raise")
    except K.KnzError as e:
        assert e.code == ERR_INVALID_PARAM
    dst, kd = be.empty(len(data) + 64)                                      # the handle still works
    assert codec.dev_decompress(sp, len(stream), dst, len(data) + 64) == len(data)
    be.sync()
    assert be.to_host(kd, len(data)) == data
    codec.close()


# ---- 11. copy blocks and -s ---------------------------------------------------------------------------------------------------------------------------------
def check_copy_blocks(be, pipe):
    bs = 1024
    case = RC.skip_stream(pipe, bs)
    data, stream, bounds = case
    cp = RC.copy_blocks(stream)
    assert cp
    codec = M.codec_for(be, pipe, bs)
    reads = [((c - 1) * bs - 9, bs + 20, (3 * c) % 16) for c in cp] + [((cp[0] - 1) * bs + 100, 50, 7), (0, len(data), 13)]
    _check_writer_reads(be, codec, case, bs, reads)
    codec.close()
