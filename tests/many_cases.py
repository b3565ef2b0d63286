"""knz_dev_compress_many / knz_dev_decompress_many: K independent .knz streams in one device batch. Cases shared by the emulator run
(tests/test_many_emu.py) and the MI355X run (tests/test_many_gpu.py). Two checkers, both must hold: the single-stream calls of the same
library (dev_compress / dev_decompress), and independently the reference's own Writer / Reader (oracle/_ref through tests/ref_lib.py).
Every input comes from a seeded generator of parity_cases.py."""
import numpy as np

import parity_cases as P
import ref_lib as R

K = P.K
GUARD = 256
ERR_WRITE_FILE, ERR_INVALID_PARAM = 12, 18

# (transform, entropy, checksum bits, -s)
PIPELINES = (("NONE", "HUFFMAN", 0, False), ("LZ", "ANS0", 0, False), ("BWT+RANK+ZRLT", "ANS1", 32, False), ("TEXT+UTF+BWT+RANK+ZRLT", "ANS0", 0, False),
             ("DNA+LZ", "HUFFMAN", 0, False), ("BWT", "FPAQ", 64, False), ("NONE", "ANS0", 0, True))


def shape_lengths(bs):
    """the lengths of case 1, plus one stream of 2^16 bytes or more whose true size goes into its header (a second width of the size field).
    At 64 KiB blocks 5 * bs + 1 is 327 681 bytes: the one input above 300 KB, kept because the shape list is what case 1 is about."""
    return [0, 1, 15, 16, 17, bs - 1, bs, bs + 1, 2 * bs, 3 * bs + 777, 5 * bs + 1, 70_001]


_TEXT = {}


def make_input(n, seed):
    """corpus / text / random bytes / nucleotides in turn (random blocks are what -s turns into copy blocks)"""
    kind = seed % 4
    if n == 0:
        return b""
    if kind == 0:
        return P.corpus(n, 100 + seed)
    if kind == 1:
        if "plain" not in _TEXT:
            _TEXT["plain"] = dict(P.text_inputs(50_000))["plain"]
        t = _TEXT["plain"]
        return (t[seed * 37 % 1000:] + t * (n // len(t) + 1))[:n]
    rng = np.random.default_rng(seed)
    if kind == 2:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes()


def shape_streams(bs, reverse=False):
    """[(data, header_input_size)]: 0 (unknown) for the even places, the true size for the odd ones and for the last"""
    lens = shape_lengths(bs)
    items = []
    for i, n in enumerate(lens):
        items.append((make_input(n, i), n if (i % 2 == 1 or i == len(lens) - 1) else 0))
    return items[::-1] if reverse else items


def codec_for(be, pipe, bs, **kw):
    t, e, ck, skip = pipe
    return K.Codec(t, e, bs, ck, lib=be.lib, skip_blocks=skip, **kw)


def ref_stream(pipe, bs, data, hs):
    t, e, ck, skip = pipe
    return R.compress(data, t, e, bs, ck, header_size=hs, skip_blocks=skip)


def out_cap(n):
    return 2 * n + (1 << 17)


def _guarded(be, cap):
    ptr, keep = be.empty(cap + GUARD)
    view = keep[1] if be.name == "emu" else keep
    view[cap: cap + GUARD] = 0xA5
    return ptr, keep


def _guard_intact(be, keep, cap):
    return be.to_host(keep, cap + GUARD)[cap:] == b"\xa5" * GUARD


def compress_many(be, codec, items, caps=None):
    """items: [(data, header size)] -> ([(bytes or None, status)], return code); the guards behind every dst_cap are checked here"""
    keep, call = [], []
    for i, (data, hs) in enumerate(items):
        src, ks = be.to_dev(data)
        cap = caps[i] if caps else out_cap(len(data))
        dst, kd = _guarded(be, cap)
        keep.append((ks, kd, cap))
        call.append((src, len(data), dst, cap, hs))
    res = codec.dev_compress_many(call)
    be.sync()
    out = []
    for (nb, status), (_ks, kd, cap) in zip(res, keep):
        assert _guard_intact(be, kd, cap), "bytes behind a dst_cap were written"
        assert nb <= cap
        out.append((be.to_host(kd, nb) if status == 0 else None, status))
    return out, codec.last_many_rc


def decompress_many(be, codec, items):
    """items: [(stream bytes, dst_cap)] -> ([(bytes or None, status)], return code)"""
    keep, call = [], []
    for stream, cap in items:
        src, ks = be.to_dev(stream, 4)
        dst, kd = _guarded(be, cap)
        keep.append((ks, kd, cap))
        call.append((src, len(stream), dst, cap))
    res = codec.dev_decompress_many(call)
    be.sync()
    out = []
    for (nb, status), (_ks, kd, cap) in zip(res, keep):
        assert _guard_intact(be, kd, cap), "bytes behind a dst_cap were written"
        assert nb <= cap
        out.append((be.to_host(kd, nb) if status == 0 else None, status))
    return out, codec.last_many_rc


def single_compress(be, codec, data, hs, cap=None):
    """-> (bytes or None, status) of knz_dev_compress for this input alone"""
    src, ks = be.to_dev(data)
    cap = out_cap(len(data)) if cap is None else cap
    dst, kd = _guarded(be, cap)
    try:
        nb = codec.dev_compress(src, len(data), dst, cap, header_input_size=hs)
    except K.KnzError as e:
        assert _guard_intact(be, kd, cap)
        return None, e.code
    assert _guard_intact(be, kd, cap)
    return be.to_host(kd, nb), 0


def single_decompress(be, codec, stream, cap):
    src, ks = be.to_dev(stream, 4)
    dst, kd = _guarded(be, cap)
    try:
        nb = codec.dev_decompress(src, len(stream), dst, cap)
    except K.KnzError as e:
        return None, e.code
    return be.to_host(kd, nb), 0


def first_failure(results):
    return next((s for _b, s in results if s), 0)


def _diff(a, b):
    return len(a), len(b), [i for i in range(min(len(a), len(b))) if a[i] != b[i]][:4]


def check_against_both(be, codec, pipe, bs, items, singles=None):
    """one many call: every stream equals the single call's bytes and the reference Writer's; then the reference's streams through
    dev_decompress_many give the inputs back. singles: the places that are also run through the single call (default: all)."""
    got, rc = compress_many(be, codec, items)
    assert rc == 0 and first_failure(got) == 0, (pipe, bs, rc, [s for _b, s in got])
    refs = []
    for i, ((data, hs), (g, _s)) in enumerate(zip(items, got)):
        r = ref_stream(pipe, bs, data, hs)
        refs.append(r)
        assert g == r, (pipe, bs, i, len(data), "stream of the many call != the reference Writer's", _diff(g, r))
        if singles is None or i in singles:
            s, code = single_compress(be, codec, data, hs)
            assert code == 0 and g == s, (pipe, bs, i, len(data), "stream of the many call != the single call's", code)
    back, rc = decompress_many(be, codec, [(r, len(d) + 64) for r, (d, _h) in zip(refs, items)])
    assert rc == 0, (pipe, bs, rc, [s for _b, s in back])
    for i, ((data, _hs), (b, s)) in enumerate(zip(items, back)):
        assert s == 0 and b == data, (pipe, bs, i, len(data), s, "reference stream -> dev_decompress_many")
    return refs


def check_shapes(be, pipe, bs, monkeypatch=None):
    """cases 1 and 8: the shape list, forward and reversed; on the emulator (monkeypatch given) under both block schedules"""
    scheds = ("fwd", "rev") if (monkeypatch is not None and be.name == "emu") else (None,)
    codec = codec_for(be, pipe, bs)
    for sched in scheds:
        if sched:
            monkeypatch.setenv("KNZ_EMU_SCHED", sched)
        for reverse in (False, True):
            if sched == "rev" and reverse:
                continue                                                   # (emulator: the list under both schedules, the reversed list under one)
            check_against_both(be, codec, pipe, bs, shape_streams(bs, reverse), singles=() if (reverse or sched == "rev") else None)
    if monkeypatch is not None:
        monkeypatch.delenv("KNZ_EMU_SCHED", raising=False)
    codec.close()


# ---- coverage guard, from the reference's outputs alone ---------------------------------------------------------------------------------
def _bits(stream, pos, n):
    v = 0
    for i in range(n):
        v = (v << 1) | ((stream[(pos + i) >> 3] >> (7 - ((pos + i) & 7))) & 1)
    return v


def stream_end_bit(stream):
    """walks header and framing of a .knz stream (CompressedStream.go:1316-1460, :1816-1852) -> (number of blocks, bit behind the end marker)"""
    sz = _bits(stream, 32 + 4 + 2 + 5 + 48 + 28, 2)
    pos = 32 + 4 + 2 + 5 + 48 + 28 + 2 + 16 * sz + 15 + 24
    nblocks = 0
    while True:
        lw = _bits(stream, pos, 5) + 3
        written = _bits(stream, pos + 5, lw)
        pos += 5 + lw
        if written == 0:
            return nblocks, pos
        pos += written
        nblocks += 1


def check_coverage(block_sizes=(1024, 1 << 14)):
    for bs in block_sizes:
        pipe = PIPELINES[0]
        items = shape_streams(bs)
        ends, blocks = [], []
        for data, hs in items:
            r = ref_stream(pipe, bs, data, hs)
            nb, end = stream_end_bit(r)
            assert (end + 7) // 8 == len(r) and nb == (len(data) + bs - 1) // bs, (len(data), nb, end, len(r))
            ends.append(end)
            blocks.append(nb)
        lens = [len(d) for d, _h in items]
        assert any(n == 0 for n in lens) and any(0 < n <= 15 for n in lens) and any(n == bs for n in lens), lens
        assert any(n > bs and n % bs for n in lens), lens                  # ragged multi-block
        assert any(e % 32 for e in ends[:-1]), ends                       # a stream with a neighbour behind it ends inside a 32-bit word
        assert any(e % 8 for e in ends), ends                             # ... and one inside a byte (the zero padding of the last word)
        widths = {len(ref_stream(pipe, bs, d, h)) - (stream_end_bit(ref_stream(pipe, bs, d, h))[1] + 7) // 8 for d, h in items[:1]}
        assert widths == {0}
        hdr = {_bits(ref_stream(pipe, bs, d, h), 119, 2) for d, h in items}
        assert {0, 1, 2} <= hdr, hdr                                       # size field absent, 16 bits, 32 bits


# ---- case 2 ------------------------------------------------------------------------------------------------------------------------------
def check_k(be, pipe, bs, k):
    rng = np.random.default_rng(k)
    items = []
    for i in range(k):
        n = int(rng.integers(1, 3 * bs + 200))
        items.append((make_input(n, i + k), n if i % 3 else 0))
    codec = codec_for(be, pipe, bs)
    check_against_both(be, codec, pipe, bs, items, singles=range(0, k, 5))
    codec.close()


def check_group_limit(be, pipe=("BWT+RANK+ZRLT", "ANS0", 0, False), bs=1024, streams=40, blocks=26, singles=range(0, 40, 13)):
    """more than 1023 blocks in one call with a BWT pipeline: the suffix sort's groups of blocks"""
    assert streams * blocks > 1023
    items = [(make_input(blocks * bs - (i % 7) * 13, i), 0) for i in range(streams)]
    codec = codec_for(be, pipe, bs)
    check_against_both(be, codec, pipe, bs, items, singles=singles)
    codec.close()


# ---- case 3 ------------------------------------------------------------------------------------------------------------------------------
def check_one_batch(be, pipe=("BWT+RANK+ZRLT", "ANS1", 32, False), bs=1 << 14):
    items = [(make_input(n, i), n) for i, n in enumerate((17, bs, 2 * bs + 5, 3 * bs + 777, 900))]
    codec = codec_for(be, pipe, bs)
    total = 0
    for data, hs in items:
        assert single_compress(be, codec, data, hs)[1] == 0
        total += codec.last_counter(1)
    got, rc = compress_many(be, codec, items)
    assert rc == 0
    assert codec.last_counter(1) == total, (codec.last_counter(1), total)
    names = [n for n, _ms in codec.last_kernel_times()]
    assert names.count("knz_many_asm_plan_kernel") == 1 and names.count("knz_many_asm_copy_kernel") == 1, names
    codec.close()


# ---- case 4 ------------------------------------------------------------------------------------------------------------------------------
def check_mixed_trouble(be, pipe, bs=1 << 14):
    rng = np.random.default_rng(41)
    t, e, ck, skip = pipe
    datas = [make_input(n, 20 + i) for i, n in enumerate((3 * bs + 777, bs, 2 * bs + 1, 17, 5 * bs + 1, bs - 1, 2 * bs, 3 * bs, bs + 9, 4 * bs + 3, 1000))]
    good = [ref_stream(pipe, bs, d, len(d)) for d in datas]
    items = [(g, len(d) + 64) for g, d in zip(good, datas)]
    items[1] = (good[1][: len(good[1]) // 2], items[1][1])                 # cut in the middle
    b = bytearray(good[4])
    for i in rng.integers(30, len(b), 3):
        b[int(i)] ^= int(rng.integers(1, 256))
    items[3] = (bytes(b), len(datas[4]) + 64)                              # 3 bytes flipped behind the header (a copy of stream 4)
    datas[3] = datas[4]
    items[5] = (R.compress(datas[5], t, e, 2 * bs, ck, skip_blocks=skip), items[5][1])   # another block size in its header
    items[7] = (b"\x00" + good[7][1:], items[7][1])                        # bad magic
    items[9] = (good[9], len(datas[9]) - 1)                                # dst_cap one byte short
    bad = (1, 3, 5, 7, 9)
    codec = codec_for(be, pipe, bs)
    got, rc = decompress_many(be, codec, items)
    for i, (stream, cap) in enumerate(items):
        g, s = got[i]
        if i not in bad:
            assert s == 0 and g == datas[i], (pipe, i, s, "a good stream next to damaged ones")
            continue
        sg, ss = single_decompress(be, codec, stream, cap)
        if i == 5:
            assert s == ERR_INVALID_PARAM and g is None, (pipe, i, s)
            continue
        assert s == ss, (pipe, i, "status of the many call != the single call's", s, ss)
        assert g == sg, (pipe, i, "bytes of the many call != the single call's")
        if i == 3:
            try:
                r = R.decompress(stream, cap)
            except R.RefError:
                r = None
            if r is not None and g is not None:
                assert g == r, (pipe, i, "flipped stream: device bytes != the reference Reader's")
        else:
            assert s != 0, (pipe, i)
        if i == 9:
            assert s == ERR_WRITE_FILE, s
    assert rc == first_failure(got) and rc != 0, (rc, [s for _g, s in got])
    codec.close()


# ---- case 5 ------------------------------------------------------------------------------------------------------------------------------
def check_small_destination(be, pipe, bs=1 << 14, sweep=True):
    items = [(make_input(n, 50 + i), n) for i, n in enumerate((2 * bs + 100, 3 * bs + 777, 600, 0, bs))]
    codec = codec_for(be, pipe, bs)
    full, rc = compress_many(be, codec, items)
    assert rc == 0
    for victim in (1, 3):
        caps = [out_cap(len(d)) for d, _h in items]
        caps[victim] = len(full[victim][0]) - 8
        got, rc = compress_many(be, codec, items, caps)
        assert rc == ERR_WRITE_FILE, rc
        for i in range(len(items)):
            if i == victim:
                assert got[i] == (None, ERR_WRITE_FILE), got[i][1]
                assert single_compress(be, codec, items[i][0], items[i][1], caps[i])[1] == ERR_WRITE_FILE
            else:
                assert got[i] == full[i], (pipe, victim, i)
    # the smallest destination the single call accepts is the smallest the many call accepts
    data, hs = items[2]
    n = len(full[2][0])
    for cap in (range(n - 4, n + 12) if sweep else ()):
        s = single_compress(be, codec, data, hs, cap)
        m, _rc = compress_many(be, codec, [items[4], (data, hs)], [out_cap(bs), cap])
        assert m[1] == s, (cap, n, m[1][1], s[1])
    codec.close()


# ---- case 6 ------------------------------------------------------------------------------------------------------------------------------
def check_short_inner(be):
    """A stream whose first segment ends in a short block (two rank segments assembled by knz_dev_assemble, as parity_cases.check_short_inner_block
    builds it) between two ordinary streams: the short inner block moves every later block of ITS stream only."""
    bs = 1 << 14
    for pipe in (("NONE", "HUFFMAN", 0, False), ("BWT+RANK+ZRLT", "ANS0", 0, False)):
        a, b = P.corpus(bs + 4321, 7), P.corpus(2 * bs + 99, 8)
        c = codec_for(be, pipe, bs)
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
        gappy = be.to_host(kout, total)
        assert R.decompress(gappy, n + 64) == a + b
        d0, d2 = make_input(2 * bs + 5, 1), make_input(bs + 1, 4)
        items = [(ref_stream(pipe, bs, d0, 0), len(d0) + 64), (gappy, n + 64), (ref_stream(pipe, bs, d2, 0), len(d2))]
        got, rc = decompress_many(be, c, items)
        assert rc == 0 and [g for g, _s in got] == [d0, a + b, d2], (pipe, rc, [s for _g, s in got])
        c.close()


# ---- case 7 ------------------------------------------------------------------------------------------------------------------------------
def check_lanes(be, pipe=("LZ", "ANS0", 0, False), bs=1 << 14):
    items = shape_streams(bs)[4:10]
    c1 = codec_for(be, pipe, bs)
    want, rc = compress_many(be, c1, items)
    c1.close()
    assert rc == 0
    c3 = codec_for(be, pipe, bs, devices=[0, 0, 0])
    assert c3.L.knz_lane_count(c3.h) == 3
    got, rc = compress_many(be, c3, items)
    assert rc == 0 and got == want
    back, rc = decompress_many(be, c3, [(g, len(d) + 64) for (g, _s), (d, _h) in zip(got, items)])
    assert rc == 0 and [b for b, _s in back] == [d for d, _h in items]
    c3.close()


# ---- workspace the device refuses: the stream list in halves ------------------------------------------------------------------------------
def check_alloc_split(be, monkeypatch, pipe=("LZ", "ANS0", 0, False), bs=1 << 16):
    items = [(P.corpus(bs - 100 * i, 20 + i), 0) for i in range(12)]
    monkeypatch.delenv("KNZ_TEST_ALLOC_LIMIT", raising=False)
    c = codec_for(be, pipe, bs)
    want, rc = compress_many(be, c, items)
    c.close()
    assert rc == 0
    monkeypatch.setenv("KNZ_TEST_ALLOC_LIMIT", "1500000")                  # (the stage buffer of 12 blocks of 64 KiB does not fit, that of 3-6 does)
    c = codec_for(be, pipe, bs)
    got, rc = compress_many(be, c, items)
    assert rc == 0 and got == want, rc
    back, rc = decompress_many(be, c, [(g, len(d) + 64) for (g, _s), (d, _h) in zip(got, items)])
    assert rc == 0 and [b for b, _s in back] == [d for d, _h in items], rc
    c.close()
    monkeypatch.setenv("KNZ_TEST_ALLOC_LIMIT", "1000")                     # nothing fits: every stream comes back with an error, the call does not crash
    c = codec_for(be, pipe, bs)
    got, rc = compress_many(be, c, items[:3])
    assert rc != 0 and all(s != 0 for _g, s in got)
    c.close()
    monkeypatch.delenv("KNZ_TEST_ALLOC_LIMIT", raising=False)


def check_api(be):
    """n <= 0, the raising form, misaligned pointers"""
    c = codec_for(be, PIPELINES[0], 1024)
    assert c.dev_compress_many([]) == [] and c.last_many_rc == 0
    assert c.dev_decompress_many([]) == [] and c.last_many_rc == 0
    data = make_input(3000, 1)
    src, ks = be.to_dev(data)
    dst, kd = be.empty(out_cap(3000))
    res = c.dev_compress_many([(src, 3000, dst, out_cap(3000)), (src + 1, 2999, dst, out_cap(3000))])
    assert res[0][1] == 0 and res[1] == (0, ERR_INVALID_PARAM) and c.last_many_rc == ERR_INVALID_PARAM
    assert be.to_host(kd, res[0][0]) == ref_stream(PIPELINES[0], 1024, data, 3000)
    try:
        c.dev_compress_many([(src, 3000, dst, 8)], check=True)
        raise AssertionError("check=True did not raise")
    except K.KnzError as e:
        assert e.code == ERR_WRITE_FILE
    c.close()
