"""knz_dev_write_many / knz_dev_append: byte writes (offset, length, data) into a .knz stream, one new stream out. Cases shared by the emulator run
(tests/test_write_emu.py) and the MI355X run (tests/test_write_gpu.py). Streams and helpers are range_cases': the reference's own Writer wrote the
sources, and the expected stream of a call is the reference Writer's too: many_cases.ref_stream(pipe, bs, edited, header size), `edited` being the
writes applied to the source's data here in Python. Where damaged or short frames are carried verbatim the expectation is put together from
reference streams with range_cases.frames() / splice_streams().

The destination and the data of the writes live in arenas filled with a known byte, guards on both sides: after a call that fails the whole
destination arena has to be that byte still, after a good one everything behind the stream's last 32-bit word."""
import ctypes as C

import numpy as np

import many_cases as M
import range_cases as RC

K = RC.K
END = K.api.OFFSET_END                                                     # (the binding of the write calls: nothing here runs without it)
KEEP = K.api.HEADER_SIZE_KEEP
assert END == 2 ** 64 - 1 and KEEP == -1
GUARD, FILL = 32, 0xA5
ERR_MISSING_PARAM, ERR_WRITE_FILE, ERR_INVALID_PARAM = RC.ERR_MISSING_PARAM, RC.ERR_WRITE_FILE, RC.ERR_INVALID_PARAM
COUNTER_DECODE_BLOCKS, COUNTER_ENCODE_BLOCKS = 7, 16
GRID_PIPE, GRID_BS = RC.PIPELINES[1], 1024                                  # NONE&HUFFMAN/32
GRID_LENGTHS = (1, 3, 15, 16, 17, 31, 32, 33, 47, 100)
GRID_STEP = 144                                                             # a write every 144 bytes: disjoint at every length, offset mod 16 free
XF_PIPE = RC.PIPELINES[3]                                                   # BWT+RANK+ZRLT&ANS1/64
EMU_WIDE = (RC.PIPELINES[1], RC.PIPELINES[2])                               # the pipelines the emulator also runs at 16400


# ---- what a call has to deliver -----------------------------------------------------------------------------------------------------------------
class Hole(Exception):
    def __init__(self, index):
        self.index = index


def payload(n, seed, text=False):
    if text:
        return RC.P.corpus(max(n, 64), 40 + seed)[:n]
    return np.random.default_rng(1000 + seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def apply(data, writes):
    """the writes in index order, a later one over an earlier one ; END: the length as it stands ; a write behind the end: Hole"""
    out = bytearray(data)
    for i, (o, d) in enumerate(writes):
        o = len(out) if o == END else o
        if o > len(out):
            raise Hole(i)
        out[o: o + len(d)] = d
    return bytes(out)


def touched_blocks(n_old, bs, writes):
    """block indices from 0 of the old stream that a call decodes: those a write covers, and the last one where a write reaches it or uses END"""
    nb = (n_old + bs - 1) // bs
    out, cur = set(), n_old
    for o, d in writes:
        reach = o == END or o + len(d) > (nb - 1) * bs
        o = cur if o == END else o
        if d:
            out |= set(range(o // bs, min((o + len(d) - 1) // bs + 1, nb)))
        if reach and nb:
            out.add(nb - 1)
        cur = max(cur, o + len(d))
    return out


def header_size_of(stream):
    return RC.frames(stream)[0]["output_size"]


def expected_stream(pipe, bs, data, stream, writes, header_size=KEEP):
    """(edited, the reference Writer's stream for it under the header the call asks for)"""
    edited = apply(data, writes)
    hs = header_size
    if hs == KEEP:
        hs = header_size_of(stream) + len(edited) - len(data) if header_size_of(stream) else 0
    return edited, M.ref_stream(pipe, bs, edited, hs)


def run_shifts(old, new, touched):
    """(new bit - old bit) mod 32 of every maximal run of untouched frames, from the two streams' framing alone"""
    fo, fn = RC.frames(old)[1], RC.frames(new)[1]
    out, prev = set(), True
    for b in range(len(fo)):
        if b in touched or b >= len(fn):
            prev = True
            continue
        assert fo[b][2] == fn[b][2], "an untouched frame changed its size"
        if prev:
            out.add((fn[b][0] - fo[b][0]) % 32)
        prev = False
    return out


# ---- the case lists (pure: the coverage guards look at what they yield) ----------------------------------------------------------------------------
def grid_writes():
    """256 disjoint writes: every pairing of offset mod 16 and data address mod 16, the lengths cycling -> [(offset, data, data mod 16)]"""
    out = []
    for sm in range(16):
        for dm in range(16):
            i = sm * 16 + dm
            out.append((GRID_STEP * i + sm, payload(GRID_LENGTHS[i % len(GRID_LENGTHS)], i), dm))
    return out


def boundary_cases(bs):
    """name -> (source length, [(offset, data)]) ; sources are range_cases.sized_stream(pipe, bs, length)"""
    n = RC.BLOCKS * bs + RC.TAIL
    p = payload
    return {
        "one boundary": (n, [(3 * bs - 50, p(100, 1))]),
        "several boundaries": (n, [(5 * bs - 10, p(2 * bs + 30, 2))]),
        "one whole block": (n, [(9 * bs, p(bs, 3))]),
        "to a block's last byte": (n, [(12 * bs - 40, p(40, 4))]),
        "inside the ragged block": (n, [(RC.BLOCKS * bs + 100, p(200, 5))]),
        "ending at L": (n, [(n - 50, p(50, 6))]),
        "one byte past L": (n, [(n - 10, p(11, 7))]),
        "three blocks and five bytes past L": (n, [(n - 20, p(20 + 3 * bs + 5, 8))]),
        "END, ragged": (n, [(END, p(300, 9))]),
        "END, full blocks": (4 * bs, [(END, p(bs + 7, 10))]),
        "END, empty stream": (0, [(END, p(2 * bs + 100, 11))]),
        "append of one byte": (4 * bs, [(END, p(1, 12))]),
        "append of nothing": (n, [(END, b"")]),
    }


def order_cases(bs):
    n = RC.BLOCKS * bs + RC.TAIL
    p = payload
    return {
        "overlap, same range, nested": (n, [(100, p(500, 20)), (300, p(500, 21)), (300, p(500, 22)), (350, p(50, 23)), (bs - 20, p(100, 24)), (bs + 10, p(10, 25)),
                                            (100, p(500, 26)), (0, p(3 * bs, 27)), (bs + 5, p(bs, 28))]),
        "two END writes": (n, [(END, p(100, 29)), (END, p(bs + 900, 30))]),
        "an offset inside an earlier write's growth": (n, [(END, p(100, 31)), (n + 50, p(200, 32)), (n - 5, p(10, 33))]),
    }


def header_cases(bs):
    """name -> (source length, source header size (None: the true one), [(offset, data)], header_input_size of the call)"""
    n = RC.BLOCKS * bs + RC.TAIL
    p = payload
    small, grow = [(2 * bs + 7, p(60, 40))], [(END, p(30000, 41))]
    return {
        "none -> true size": (n, 0, small, n),
        "true size -> none": (n, None, small, 0),
        "KEEP, field, no growth": (n, None, [(7 * bs + 1, p(333, 42))], KEEP),
        "KEEP, no field, no growth": (n, 0, small, KEEP),
        "KEEP, no field, growth": (n, 0, [(END, p(500, 43))], KEEP),
        "KEEP, field, growth (16 -> 32 bits at 1024)": (n, None, grow, KEEP),
        "none -> 32 bits": (n, 0, [(20 * bs + 3, p(41, 44))], 70000),
        "KEEP, a block grows or shrinks": (n, None, [(4 * bs, p(bs, 45, text=True)), (15 * bs + 100, bytes(600))], KEEP),
    }


def source(pipe, bs, n, hs=None):
    data, stream, _b = RC.sized_stream(pipe, bs, n)
    if hs is not None:
        stream = RC._ref(pipe, bs, data, hs)
    return data, stream


def check_coverage(block_sizes=(1024,), pipes=(GRID_PIPE, XF_PIPE)):
    grid = grid_writes()
    assert {(o % 16, dm) for o, _d, dm in grid} == {(s, d) for s in range(16) for d in range(16)}, "not every (offset mod 16, data mod 16) pair"
    assert {len(d) for _o, d, _dm in grid} == set(GRID_LENGTHS)
    spans = sorted((o, o + len(d)) for o, d, _dm in grid)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= RC.BLOCKS * GRID_BS, "the grid's writes are not disjoint"
    shifts, widths = set(), set()
    for bs in block_sizes:
        for pipe in pipes:
            for n, hs, writes, hsz in header_cases(bs).values():
                data, stream = source(pipe, bs, n, hs)
                _e, new = expected_stream(pipe, bs, data, stream, writes, hsz)
                shifts |= run_shifts(stream, new, touched_blocks(n, bs, writes))
                widths |= {RC.frames(stream)[0]["header_bits"], RC.frames(new)[0]["header_bits"]}
            for n, writes in boundary_cases(bs).values():
                data, stream = source(pipe, bs, n)
                _e, new = expected_stream(pipe, bs, data, stream, writes)
                shifts |= run_shifts(stream, new, touched_blocks(n, bs, writes))
    assert len(widths) == 3, widths                                         # size fields of 0, 16 and 32 bits
    assert 0 in shifts and any(s % 2 for s in shifts) and 16 in shifts and len(shifts) >= 6, sorted(shifts)
    for bs in block_sizes:
        cases = boundary_cases(bs)
        n = RC.BLOCKS * bs + RC.TAIL
        assert any(o != END and (o + len(d) - 1) // bs - o // bs > 1 for _n, ws in cases.values() for o, d in ws)
        assert any(o != END and o % bs == 0 and len(d) == bs for _n, ws in cases.values() for o, d in ws)
        assert any(o != END and (o + len(d)) % bs == 0 and len(d) < bs for _n, ws in cases.values() for o, d in ws)
        assert any(o != END and o + len(d) == n for m, ws in cases.values() for o, d in ws if m == n)
        assert any(o != END and o + len(d) == n + 1 for m, ws in cases.values() for o, d in ws if m == n)
        assert any(o == END and len(d) == 1 and m % bs == 0 for m, ws in cases.values() for o, d in ws)
        assert any(m == 0 for m, _ws in cases.values()) and any(d == b"" for _m, ws in cases.values() for _o, d in ws)


# ---- device calls ------------------------------------------------------------------------------------------------------------------------------
def _view(be, keep):
    return keep[1] if be.name == "emu" else keep


def out_cap(stream, writes):
    """room for the new stream (random bytes in 1 KiB blocks under the order-1 rANS coder come to several times their size: its headers)"""
    return 2 * len(stream) + 16 * sum(len(w[1]) for w in writes) + (1 << 16)


def write_call(be, codec, stream, writes, header_size=KEEP, cap=None, dst_mod=4, single=False):
    """writes: [(offset, data[, data address mod 16])] -> (the new stream or None, [status], return code). The data of every write sits in an arena at the
    address asked for, the destination in an arena of its own at an address = dst_mod mod 16. Asserts what must not be written."""
    sp, _ks = be.to_dev(stream, 4)
    at, cur = [], GUARD
    for i, w in enumerate(writes):
        dm = w[2] if len(w) > 2 else (5 * i + 1) % 16
        cur += GUARD
        cur += (dm - cur) % 16
        at.append(cur)
        cur += len(w[1])
    dsize = cur + 2 * GUARD
    dptr, dkeep = be.empty(dsize)
    assert dptr % 16 == 0
    arena = np.full(dsize, FILL, dtype=np.uint8)
    for w, a in zip(writes, at):
        arena[a: a + len(w[1])] = np.frombuffer(w[1], dtype=np.uint8)
    if be.name == "emu":
        dkeep[1][:dsize] = arena
    else:
        dkeep[:dsize] = be.torch.from_numpy(arena).to(be.dev)
    cap = out_cap(stream, writes) if cap is None else cap
    size = GUARD + 16 + cap + GUARD
    optr, okeep = be.empty(size)
    assert optr % 16 == 0 and dst_mod % 4 == 0
    _view(be, okeep)[:size] = FILL
    lead = GUARD + dst_mod
    if single:
        assert len(writes) == 1 and writes[0][0] == END
        nb = codec.dev_append(sp, len(stream), dptr + at[0], len(writes[0][1]), optr + lead, cap, header_size)
        st = [codec.last_many_rc]
    else:
        nb, st = codec.dev_write_many(sp, len(stream), [(w[0], len(w[1]), dptr + a) for w, a in zip(writes, at)], optr + lead, cap, header_size)
    rc = codec.last_many_rc
    be.sync()
    got = be.to_host(okeep, size)
    if rc != 0:
        assert nb == 0 and got == bytes([FILL]) * size, ("a call that failed wrote to the destination", rc)
        return None, st, rc
    assert nb <= cap and all(s == 0 for s in st), (nb, cap, st)
    words = (nb + 3) // 4 * 4
    assert got[:lead] == bytes([FILL]) * lead and got[lead + words:] == bytes([FILL]) * (size - lead - words), "bytes outside the stream's words were written"
    return got[lead: lead + nb], st, 0


def _check(be, codec, pipe, bs, data, stream, writes, header_size=KEEP, **kw):
    edited, want = expected_stream(pipe, bs, data, stream, [(w[0], w[1]) for w in writes], header_size)
    got, st, rc = write_call(be, codec, stream, writes, header_size, **kw)
    assert rc == 0 and got == want, (pipe, bs, rc, st, None if got is None else M._diff(got, want))
    return edited, got


# ---- 1. alignment grid ----------------------------------------------------------------------------------------------------------------------------------
def check_alignment_grid(be):
    data, stream = source(GRID_PIPE, GRID_BS, RC.BLOCKS * GRID_BS + RC.TAIL)
    codec = M.codec_for(be, GRID_PIPE, GRID_BS)
    for dst_mod in (0, 12):
        _check(be, codec, GRID_PIPE, GRID_BS, data, stream, grid_writes(), dst_mod=dst_mod)
    codec.close()


# ---- 2. boundaries, 9. round trip ------------------------------------------------------------------------------------------------------------------------
def check_boundaries(be, pipe, bs, lanes=None, names=None):
    codec = M.codec_for(be, pipe, bs, **({"devices": lanes} if lanes else {}))
    out = []
    for name, (n, writes) in boundary_cases(bs).items():
        if names is not None and name not in names:
            continue
        data, stream = source(pipe, bs, n)
        hs = 0 if name == "append of nothing" else KEEP                     # (the stream comes back under another header)
        _e, got = _check(be, codec, pipe, bs, data, stream, writes, hs, single=name.startswith("append"), dst_mod=(0, 4, 8, 12)[len(out) % 4])
        out.append(got)
    codec.close()
    return out


def check_copy_blocks(be, pipe, bs=1024):
    """-s: random bytes over a text block make it a copy block, text over a random block makes it a coded one"""
    data, stream, _b = RC.skip_stream(pipe, bs)
    before = RC.copy_blocks(stream)
    assert 1 not in before and 2 in before
    codec = M.codec_for(be, pipe, bs)
    writes = [(0, payload(bs, 50)), (bs, payload(bs, 51, text=True))]
    _e, got = _check(be, codec, pipe, bs, data, stream, writes)
    after = RC.copy_blocks(got)
    assert 1 in after and 2 not in after and [c for c in after if c > 2] == [c for c in before if c > 2], (before, after)
    codec.close()


def check_round_trip(be, pipe=XF_PIPE, bs=1024):
    n = RC.BLOCKS * bs + RC.TAIL
    data, stream = source(pipe, bs, n)
    writes = boundary_cases(bs)["three blocks and five bytes past L"][1] + [(3 * bs - 50, payload(100, 1)), (9 * bs, payload(bs, 3))]
    codec = M.codec_for(be, pipe, bs)
    edited, got = _check(be, codec, pipe, bs, data, stream, writes)
    sp, _k = be.to_dev(got, 4)
    dst, kd = be.empty(len(edited) + 64)
    assert codec.dev_decompress(sp, len(got), dst, len(edited) + 64) == len(edited)
    be.sync()
    assert be.to_host(kd, len(edited)) == edited
    back, kb = be.empty(sum(len(d) for _o, d in writes) + 64)
    reads, at = [], 0
    for o, d in writes:
        reads.append((0, o, len(d), back + at))
        at += len(d)
    res = codec.dev_read_many([(sp, len(got))], reads)
    be.sync()
    assert codec.last_many_rc == 0 and res == [(len(d), 0) for _o, d in writes]
    assert be.to_host(kb, at) == b"".join(edited[o: o + len(d)] for o, d in writes)
    codec.close()


# ---- 3. order ------------------------------------------------------------------------------------------------------------------------------------------
def check_order(be, pipe=GRID_PIPE, bs=GRID_BS):
    codec = M.codec_for(be, pipe, bs)
    for n, writes in order_cases(bs).values():
        data, stream = source(pipe, bs, n)
        _check(be, codec, pipe, bs, data, stream, writes)
    n = RC.BLOCKS * bs + RC.TAIL
    data, stream = source(pipe, bs, n)
    for writes, bad in (([(n + 1, payload(10, 60))], 0), ([(10, payload(10, 61)), (END, payload(5, 62)), (n + 6, payload(3, 63)), (0, payload(1, 64))], 2),
                        ([(n + bs, b"")], 0)):
        try:
            apply(data, writes)
            raise AssertionError("no hole in the case")
        except Hole as h:
            assert h.index == bad
        got, st, rc = write_call(be, codec, stream, writes)
        assert got is None and rc == ERR_INVALID_PARAM and st[bad] == ERR_INVALID_PARAM, (rc, st)
    codec.close()


# ---- 4. header and shifts ----------------------------------------------------------------------------------------------------------------------------------
def check_headers(be, pipe, bs, names=None):
    codec = M.codec_for(be, pipe, bs)
    for name, (n, hs, writes, hsz) in header_cases(bs).items():
        if names is not None and name not in names:
            continue
        data, stream = source(pipe, bs, n, hs)
        _check(be, codec, pipe, bs, data, stream, writes, hsz)
    codec.close()


# ---- 5. once and only the touched ----------------------------------------------------------------------------------------------------------------------------
def check_counters(be, pipe=GRID_PIPE, bs=GRID_BS):
    n = RC.BLOCKS * bs + RC.TAIL
    data, stream = source(pipe, bs, n)
    codec = M.codec_for(be, pipe, bs)
    rng = np.random.default_rng(8)
    blocks = (2, 7, 8, 20, 30)
    writes = [(blocks[i % 5] * bs + int(rng.integers(0, bs - 100)), payload(int(rng.integers(1, 100)), 70 + i)) for i in range(64)]
    writes.append((END, payload(2 * bs, 99)))
    assert touched_blocks(n, bs, writes) == set(blocks) | {RC.BLOCKS}
    _check(be, codec, pipe, bs, data, stream, writes)
    assert codec.last_counter(COUNTER_DECODE_BLOCKS) == 6 and codec.last_counter(COUNTER_ENCODE_BLOCKS) == 8, \
        (codec.last_counter(COUNTER_DECODE_BLOCKS), codec.last_counter(COUNTER_ENCODE_BLOCKS))
    _check(be, codec, pipe, bs, data, stream, [(5 * bs + 1, payload(10, 1))])                      # one block, the last one not needed
    assert codec.last_counter(COUNTER_DECODE_BLOCKS) == 1 and codec.last_counter(COUNTER_ENCODE_BLOCKS) == 1
    empty, estream = source(pipe, bs, 0)
    _check(be, codec, pipe, bs, empty, estream, [(END, payload(bs + 1, 2))])
    assert codec.last_counter(COUNTER_DECODE_BLOCKS) == 0 and codec.last_counter(COUNTER_ENCODE_BLOCKS) == 2
    codec.close()


# ---- 6. damage ---------------------------------------------------------------------------------------------------------------------------------------------
def check_damage(be, pipe=GRID_PIPE, bs=GRID_BS):
    assert pipe[2] == 32
    n = RC.BLOCKS * bs + RC.TAIL
    data, stream = source(pipe, bs, n)
    _info, fr, _end = RC.frames(stream)
    at = (fr[4][1] + fr[4][2] // 2) // 8                                    # the middle of block 5's payload
    hurt = bytearray(stream)
    hurt[at] ^= 0x10
    hurt = bytes(hurt)
    codec = M.codec_for(be, pipe, bs)
    hp, _kh = be.to_dev(hurt, 4)
    _g, want = RC.range_call(be, codec, hp, len(hurt), bs, (5, 6))
    assert want != 0
    for writes in ([(4 * bs + 10, payload(20, 1))], [(2 * bs, payload(10, 2)), (3 * bs + 1000, payload(100, 3)), (9 * bs, payload(5, 4))]):
        got, st, rc = write_call(be, codec, hurt, writes)
        assert got is None and rc == want and [s for s in st if s] == [want], (rc, st, want)
    # the same flip in a block no write touches: the frame travels bit for bit (here behind a block that changed its size: shifted)
    writes = [(2 * bs, payload(bs, 5, text=True)), (7 * bs + 100, payload(50, 6))]
    edited, clean = expected_stream(pipe, bs, data, stream, writes)
    _i2, fn, _e2 = RC.frames(clean)
    assert fn[4][2] == fr[4][2]
    bit = fn[4][1] + (8 * at + 3 - fr[4][1])                                # (0x10 is bit 3 of its byte)
    want_stream = bytearray(clean)
    want_stream[bit // 8] ^= 0x80 >> (bit % 8)
    got, st, rc = write_call(be, codec, hurt, writes)
    assert rc == 0 and got == bytes(want_stream), (rc, st, None if got is None else M._diff(got, bytes(want_stream)))
    # a damaged length field, in front of the writes and behind them: the framing walk's code
    cut = bytearray(stream)
    cut[(fr[10][0] + 5) // 8] ^= 0x80 >> ((fr[10][0] + 5) % 8)             # block 11's (its leading bit: the walk lands inside the payload)
    cut = bytes(cut)
    cp, _kc = be.to_dev(cut, 4)
    try:
        codec.dev_stream_index(cp, len(cut))
        raise AssertionError("the damaged framing was walked to an end marker")
    except K.KnzError as e:
        walk = e.code
    for writes in ([(2 * bs, payload(10, 7))], [(20 * bs + 5, payload(10, 8))], [(END, payload(10, 9))]):
        got, st, rc = write_call(be, codec, cut, writes)
        assert got is None and rc == walk and st == [walk], (rc, st, walk)
    codec.close()


# ---- 7. short inner block ------------------------------------------------------------------------------------------------------------------------------------
def check_short_inner(be, pipe):
    bs = RC.SHORT_BS
    data, stream, bounds = RC.short_inner_stream(pipe)
    a, b = RC.short_parts(bs)
    codec = M.codec_for(be, pipe, bs)
    got, st, rc = write_call(be, codec, stream, [(bs + 10, payload(20, 1))])                       # addressed at block 2, the short one
    assert got is None and rc == ERR_INVALID_PARAM and st == [ERR_INVALID_PARAM]
    new = payload(300, 2, text=True)
    got, st, rc = write_call(be, codec, stream, [(3 * bs + 100, new)])                             # block 4: the second block of part b
    b2 = b[: bs + 100] + new + b[bs + 400:]
    want = RC.splice_streams(RC._ref(pipe, bs, a + b, len(a) + len(b)), [RC._ref(pipe, bs, a), RC._ref(pipe, bs, b2)])
    assert rc == 0 and got == want, (rc, st, None if got is None else M._diff(got, want))
    assert codec.last_counter(COUNTER_DECODE_BLOCKS) == 1
    codec.close()


# ---- 8. contract ---------------------------------------------------------------------------------------------------------------------------------------------
def check_contract(be):
    pipe, bs = GRID_PIPE, GRID_BS
    n = RC.BLOCKS * bs + RC.TAIL
    data, stream = source(pipe, bs, n)
    codec = M.codec_for(be, pipe, bs)
    L = codec.L
    Write = K.api._Write
    sp, _k = be.to_dev(stream, 4)
    dp, _kd = be.to_dev(payload(64, 1))
    cap = out_cap(stream, [])
    back, kb = be.empty(cap)
    _view(be, kb)[:cap] = FILL
    out = C.c_uint64(77)
    o = C.byref(out)
    w = (Write * 2)()
    w[0].offset, w[0].length, w[0].d_data = 10, 20, dp
    w[1].offset, w[1].length, w[1].d_data = 50, 5, dp
    assert L.knz_dev_write_many(None, sp, len(stream), w, 2, KEEP, back, cap, o, None) == ERR_MISSING_PARAM
    assert L.knz_dev_write_many(codec.h, sp, len(stream), w, 0, KEEP, back, cap, o, None) == 0 and out.value == 0
    out.value = 77
    assert L.knz_dev_write_many(codec.h, None, 0, None, -1, KEEP, None, 0, o, None) == 0 and out.value == 0
    assert L.knz_dev_write_many(codec.h, sp, len(stream), None, 2, KEEP, back, cap, o, None) == ERR_MISSING_PARAM
    assert L.knz_dev_write_many(codec.h, None, len(stream), w, 2, KEEP, back, cap, o, None) == ERR_MISSING_PARAM
    assert L.knz_dev_write_many(codec.h, sp, len(stream), w, 2, KEEP, None, cap, o, None) == ERR_MISSING_PARAM
    assert L.knz_dev_write_many(codec.h, sp, len(stream), w, 2, KEEP, back, cap, None, None) == ERR_MISSING_PARAM
    assert L.knz_dev_append(codec.h, sp, len(stream), dp, 10, KEEP, back, cap, None, None) == ERR_MISSING_PARAM
    assert L.knz_dev_append(codec.h, sp, len(stream), None, 10, KEEP, back, cap, o, None) == ERR_MISSING_PARAM
    assert L.knz_dev_write_many(codec.h, sp + 1, len(stream) - 1, w, 2, KEEP, back, cap, o, None) == ERR_INVALID_PARAM
    assert [w[0].status, w[1].status] == [ERR_INVALID_PARAM] * 2
    assert L.knz_dev_write_many(codec.h, sp, len(stream), w, 2, KEEP, back + 2, cap - 2, o, None) == ERR_INVALID_PARAM
    w[1].d_data = None
    assert L.knz_dev_write_many(codec.h, sp, len(stream), w, 2, KEEP, back, cap, o, None) == ERR_MISSING_PARAM
    assert [w[0].status, w[1].status] == [0, ERR_MISSING_PARAM] and out.value == 0
    w[1].length = 0                                                         # (no data needed for no bytes)
    assert L.knz_dev_write_many(codec.h, sp, len(stream), w, 2, KEEP, back, cap, o, None) == 0 and out.value != 0
    w[1].d_data, w[1].length = dp, 5
    w[0].offset, w[0].length = 2 ** 64 - 5, 10
    _view(be, kb)[:cap] = FILL
    assert L.knz_dev_write_many(codec.h, sp, len(stream), w, 2, KEEP, back, cap, o, None) == ERR_INVALID_PARAM
    assert [w[0].status, w[1].status] == [ERR_INVALID_PARAM, 0] and out.value == 0
    be.sync()
    assert be.to_host(kb, cap) == bytes([FILL]) * cap
    # a handle whose configuration differs from the source's header, in each of the four fields
    writes = [(3 * bs + 5, payload(40, 2))]
    for other, obs in ((("LZ", "HUFFMAN", 32, False), bs), (("NONE", "ANS0", 32, False), bs), (pipe, 2 * bs), (("NONE", "HUFFMAN", 64, False), bs)):
        c2 = M.codec_for(be, other, obs)
        got, st, rc = write_call(be, c2, stream, writes)
        assert got is None and rc == ERR_INVALID_PARAM and st == [ERR_INVALID_PARAM], (other, obs, rc, st)
        c2.close()
    # dst_cap: whole big-endian words are stored, the stream plus up to 7 bytes has to fit
    _e, want = expected_stream(pipe, bs, data, stream, writes)
    fit = (len(want) + 3) // 4 * 4 + 4
    got, st, rc = write_call(be, codec, stream, writes, cap=fit - 4)
    assert got is None and rc == ERR_WRITE_FILE and st == [ERR_WRITE_FILE], (rc, st)
    for c in (fit - 1, 7, 0):
        assert write_call(be, codec, stream, writes, cap=c)[2] == ERR_WRITE_FILE, c
    got, st, rc = write_call(be, codec, stream, writes, cap=fit)           # ... and the handle still works
    assert rc == 0 and got == want
    try:
        codec.dev_write_many(sp, len(stream), [(n + 5, 1, dp)], back, cap, check=True)
        raise AssertionError("check=True did not raise")
    except K.KnzError as e:
        assert e.code == ERR_INVALID_PARAM
    codec.close()


def check_workspace(be, monkeypatch, pipe=RC.PIPELINES[2], bs=16400):
    """KNZ_TEST_ALLOC_LIMIT (bytes one workspace buffer may hold): the call gives the right stream, in halves where it has to, or fails with the
    workspace's code and leaves the destination alone ; with room again the same handle works"""
    n = RC.BLOCKS * bs + RC.TAIL
    data, stream = source(pipe, bs, n)
    writes = [(3 * bs + 5, payload(12 * bs, 1, text=True)), (END, payload(2 * bs, 2))]
    _e, want = expected_stream(pipe, bs, data, stream, writes)
    codec = M.codec_for(be, pipe, bs)
    seen = set()
    for limit in ("100000", "300000", "600000", None):
        if limit is None:
            monkeypatch.delenv("KNZ_TEST_ALLOC_LIMIT", raising=False)
        else:
            monkeypatch.setenv("KNZ_TEST_ALLOC_LIMIT", limit)
            try:
                codec.dev_decompress(*_whole(be, stream, n))                # (where it fits, another call's workspace is in place when the limit bites)
            except K.KnzError as e:
                assert e.code in (4, 5)
        got, st, rc = write_call(be, codec, stream, writes)
        assert (rc == 0 and got == want) or (rc in (4, 5) and st == [rc] * 2), (limit, rc, st)
        seen.add(rc == 0)
    assert rc == 0 and seen == {True, False}
    codec.close()


def _whole(be, stream, n):
    sp, _k = be.to_dev(stream, 4)
    dst, _kd = be.empty(n + 64)
    _whole.keep = (_k, _kd)
    return sp, len(stream), dst, n + 64


# ---- 10. large blocks (MI355X only) ----------------------------------------------------------------------------------------------------------------------------
def check_large(be, pipe, lanes=None, bs=4 << 20):
    n = 3 * bs + bs - 1000
    data = RC.G.make_input(pipe[0], n, 3)
    stream = M.ref_stream(pipe, bs, data, n)
    writes = [(bs + 12345, payload(100, 1)), (END, payload(3000, 2, text=True))]
    edited, want = expected_stream(pipe, bs, data, stream, writes)
    codec = M.codec_for(be, pipe, bs, **({"devices": lanes} if lanes else {}))
    got, st, rc = write_call(be, codec, stream, writes)
    assert rc == 0 and got == want, (pipe, rc, st, None if got is None else M._diff(got, want))
    own, code = M.single_compress(be, codec, edited, len(edited))
    assert code == 0 and got == own, "the call's stream != the device's own dev_compress of the edited input"
    if not lanes:
        assert codec.last_counter(COUNTER_ENCODE_BLOCKS) == 3
    codec.close()
