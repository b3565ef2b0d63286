"""knz_dev_splice_many / knz_dev_concat / knz_dev_slice: whole frames of .knz streams moved into new streams, nothing decoded. Cases shared by the
emulator run (tests/test_splice_emu.py) and the MI355X run (tests/test_splice_gpu.py). The sources are the reference Writer's streams (the fixtures
of range_cases). Expectations never come from the code under test: (a) where the identity with the Writer applies, many_cases.ref_stream of the
concatenated input; (b) else the bit-splicer below over range_cases.frames(): a reference-written header for the size field, the named frames' bits,
eight zero bits. Every good output is also decoded, by the device and by the reference Reader, to the concatenation of the parts' bytes.

Sources and destinations live in one arena each, filled with a known byte, guards around every destination: a failed output's arena has to be that
byte still, a good one's everything outside the stream's 32-bit words, and the source arena never changes."""
import ctypes as C
import functools

import numpy as np

import many_cases as M
import range_cases as RC
import ref_lib as R

K = RC.K
END = RC.END
KEEP = K.api.HEADER_SIZE_KEEP
assert KEEP == -1 and K.api.BLOCK_END == 0xFFFFFFFF
assert all(hasattr(K.api.Codec, f) for f in ("dev_splice_many", "dev_concat", "dev_slice"))    # (the binding of the splice calls: nothing here runs without it)
Part, Out = K.api._SplicePart, K.api._SpliceOut
GUARD, FILL = 32, 0xA5
ERR_MISSING_PARAM, ERR_WRITE_FILE, ERR_INVALID_PARAM = RC.ERR_MISSING_PARAM, RC.ERR_WRITE_FILE, RC.ERR_INVALID_PARAM
COUNTER_DECODE_BLOCKS, COUNTER_ENCODE_BLOCKS = 7, 16
HUF = RC.PIPELINES[1]                                                       # NONE&HUFFMAN/32
RAW = RC.PIPELINES[0]                                                       # NONE&NONE/0: the shortest frames
SPLIT_BLOCKS = 300
BIG48 = (1 << 33) + 5                                                       # a size field of 48 bits


# ---- what a call has to deliver: the bit-splicer --------------------------------------------------------------------------------------------------
_frames = functools.lru_cache(maxsize=None)(RC.frames)
_DATA = {}                                                                  # stream -> (data, block boundaries), for the round trips


def known(data, stream, bounds):
    _DATA[stream] = (data, bounds)
    return stream


def as_clean(hurt, clean):
    """a damaged copy: its framing and its bytes are read off the clean stream"""
    _DATA[hurt] = ("framing", clean)
    return hurt


def _clean(stream):
    e = _DATA.get(stream)
    return e[1] if e is not None and e[0] == "framing" else stream


@functools.lru_cache(maxsize=None)
def ref_header(pipe, bs, hs):
    """(header bits as an int, their count): what the reference Writer writes in front of the first frame for this size field"""
    s = M.ref_stream(pipe, bs, b"", hs)
    hb = _frames(s)[0]["header_bits"]
    return int.from_bytes(s, "big") >> (8 * len(s) - hb), hb


def keep_size(parts):
    """KNZ_HEADER_SIZE_KEEP: the sum of the sources' size fields where every part is a whole stream that has one, else no field"""
    sizes = [_frames(_clean(s))[0]["output_size"] if (f, t) == (1, END) else 0 for s, f, t in parts]
    return sum(sizes) if all(sizes) else 0


def layout(pipe, bs, parts, hs):
    """parts: [(stream, from_block, to_block)] of ONE output -> (header size field, header bits, [(source bit, bits, destination bit, blocks)] per part)"""
    hs = keep_size(parts) if hs == KEEP else hs
    at = ref_header(pipe, bs, hs)[1]
    runs = []
    for s, f, t in parts:
        fr = _frames(_clean(s))[1]
        lo, hi = RC.span((f, t), len(fr))
        a = fr[lo][0] if hi > lo else 0
        n = fr[hi - 1][1] + fr[hi - 1][2] - a if hi > lo else 0
        runs.append((a, n, at, max(hi - lo, 0)))
        at += n
    return hs, at + 8, runs


def spliced(pipe, bs, parts, hs):
    """expectation (b): header, the frames' bits, end marker"""
    hs, total, runs = layout(pipe, bs, parts, hs)
    acc, nbits = ref_header(pipe, bs, hs)
    for (s, _f, _t), (a, n, _d, _b) in zip(parts, runs):
        if n:
            acc = (acc << n) | ((int.from_bytes(s, "big") >> (8 * len(s) - a - n)) & ((1 << n) - 1))
            nbits += n
    acc, nbits = acc << 8, nbits + 8
    assert nbits == total
    pad = -nbits % 8
    return (acc << pad).to_bytes((nbits + pad) // 8, "big")


def decoded(parts):
    out = b""
    for s, f, t in parts:
        data, bounds = _DATA[_clean(s)]
        out += RC.expected(data, bounds, (f, t))
    return out


# ---- sources -----------------------------------------------------------------------------------------------------------------------------------------
def main(pipe, bs):
    return known(*RC.main_stream(pipe, bs))


def sized(pipe, bs, n, hs=None):
    data, stream, bounds = RC.sized_stream(pipe, bs, n)
    if hs is not None:
        stream = RC._ref(pipe, bs, data, hs)
    return known(data, stream, bounds)


@functools.lru_cache(maxsize=None)
def five(pipe, bs):
    return tuple(known(*t) for t in RC.many_streams(pipe, bs))


@functools.lru_cache(maxsize=None)
def tiny(pipe, bs, i):
    data = bytes((7 * i + j) & 255 for j in range(1 + i % 3))
    return known(data, RC._ref(pipe, bs, data, 0 if i % 2 else None), [0, len(data)])


def whole(streams, out=0):
    return [(s, 1, END, out) for s in streams]


# ---- the case lists (pure: the coverage guard looks at what they yield) -> {name: (parts [(stream, from, to, out)], [header size per output], identity data or None)}
def concat_cases(pipe, bs):
    s = five(pipe, bs)
    a, b, c = sized(pipe, bs, bs), sized(pipe, bs, 3 * bs), sized(pipe, bs, 2 * bs + 99)
    a0 = sized(pipe, bs, bs, 0)
    cat = _DATA[a][0] + _DATA[b][0] + _DATA[c][0]
    return {
        "five": (whole(s), [KEEP], None),
        "five reversed": (whole(s[::-1]), [sum(len(_DATA[x][0]) for x in s)], None),
        "identity, no field": (whole([a, b, c]), [0], cat),
        "identity, a value": (whole([a, b, c]), [len(cat)], cat),
        "identity, 48 bits": (whole([a, b, c]), [BIG48], cat),
        "identity, KEEP, every source has the field": (whole([a, b, c]), [KEEP], cat),
        "identity, KEEP, one source lacks it": (whole([a0, b, c]), [KEEP], cat),
    }


def slice_cases(pipe, bs):
    m = main(pipe, bs)
    n = len(_DATA[m][1]) - 1
    out = {}
    for i, (f, t) in enumerate(RC.ranges_of(n)):
        out[f"{f}..{t}"] = ([(m, f, t, 0)], [(0, KEEP, 70000 + i, 5)[i % 4]], None)
    out["the source back"] = ([(m, 1, END, 0)], [len(_DATA[m][0])], None)
    return out


def regroup_case(pipe=HUF, bs=1024):
    """one call: one output per block of a 301-block stream, one output of all its blocks backwards, blocks 3, 1, 2, the same source in several parts
    and outputs, a second source between them"""
    big = sized(pipe, bs, SPLIT_BLOCKS * bs + 5)
    m = main(pipe, bs)
    nb = SPLIT_BLOCKS + 1
    parts = [(big, b, b + 1, b - 1) for b in range(1, nb + 1)]
    hss = [(0, KEEP, 9)[b % 3] for b in range(nb)]
    parts += [(big, b, b + 1, nb) for b in range(nb, 0, -1)]
    parts += [(big, 3, 4, nb + 1), (big, 1, 2, nb + 1), (big, 2, 3, nb + 1)]
    parts += [(big, 5, 10, nb + 2), (m, 2, 5, nb + 2), (big, 2, 5, nb + 2), (big, 5, 10, nb + 2), (m, 30, END, nb + 2)]
    parts += [(m, 1, END, nb + 3), (big, nb, END, nb + 3)]
    return parts, hss + [0, KEEP, 123456, KEEP]


def tiny_case(pipe, bs=1024):
    """45 streams of 1 to 3 bytes in one output, empty streams and ranges behind the end at the first, a middle and the last position and between ; an
    output of only empty parts ; an output of no parts"""
    e = sized(pipe, bs, 0)
    ts = [tiny(pipe, bs, i) for i in range(45)]
    parts = [(e, 1, END, 0), (ts[0], 2, 3, 0)]
    for i, t in enumerate(ts):
        parts.append((t, 1, END, 0))
        if i % 6 == 1:                                                      # (three tiny frames come to 128 bits: not behind every third)
            parts += [(e, 1, END, 0), (ts[i], 4, 5, 0), (e, 2, 3, 0)]
        if i % 6 == 3:
            parts.append((ts[i], 5, 9, 0))
    parts += [(ts[1], 3, END, 0), (e, 1, 2, 0)]
    parts += [(e, 1, END, 1), (ts[3], 2, END, 1), (e, 1, END, 1)]
    return parts, [KEEP, 0, 777]                                            # (output 2 has no parts)


def by_output(parts, n_outs):
    out = [[] for _ in range(n_outs)]
    for s, f, t, o in parts:
        out[o].append((s, f, t))
    return out


def check_shifts(cases_run):
    """over all cases: (destination bit - source bit) mod 32 of the runs is all of 0 .. 31, every width of the header's size field occurs, and the
    bit-splicer agrees with the reference Writer wherever the identity applies"""
    shifts, widths = set(), set()
    for pipe, bs in cases_run:                                              # the (pipeline, block size) pairs the concat and slice tests run at
        cases = list(concat_cases(pipe, bs).values()) + list(slice_cases(pipe, bs).values())
        for parts, hss, cat in cases:
            for ps, hs in zip(by_output(parts, len(hss)), hss):
                hsz, _total, runs = layout(pipe, bs, ps, hs)
                widths.add(ref_header(pipe, bs, hsz)[1])
                shifts |= {(d - a) % 32 for a, n, d, _b in runs if n}
                if cat is not None:
                    assert spliced(pipe, bs, ps, hs) == M.ref_stream(pipe, bs, cat, hsz), (pipe, bs, hs, "the bit-splicer != the reference Writer")
    for parts, hss in (regroup_case(), tiny_case(RAW), tiny_case(HUF)):
        for ps, hs in zip(by_output(parts, len(hss)), hss):
            shifts |= {(d - a) % 32 for a, n, d, _b in layout(HUF, 1024, ps, hs)[2] if n}
    assert shifts == set(range(32)), sorted(set(range(32)) - shifts)
    assert len(widths) == 4 and max(widths) - min(widths) == 48, widths     # no size field, 16, 32 and 48 bits
    # the tiny case: a 32-bit word that five pieces share, empty pieces at the first, a middle and the last position
    for pipe in (RAW, HUF):
        parts, hss = tiny_case(pipe)
        ps = by_output(parts, len(hss))
        _h, _t, runs = layout(pipe, 1024, ps[0], hss[0])
        live = [r for r in runs if r[1]]
        assert len(live) >= 40 and runs[0][1] == 0 and runs[-1][1] == 0 and any(r[1] == 0 for r in runs[10:-10]), pipe
        assert all(r[1] == 0 for r in layout(pipe, 1024, ps[1], hss[1])[2]) and ps[2] == []
        if pipe == RAW:
            # (the reference Writer's shortest frame, a 1-byte block under NONE&NONE, has 34 bits: no more than two frames meet in a word, the
            # empty pieces between them bring the pieces of one word to five)
            per_word = {}
            for a, n, d, _b in runs:
                for w in range(d // 32, (d + max(n, 1) - 1) // 32 + 1):
                    per_word.setdefault(w, []).append(n)
            assert any(len(v) >= 5 and sum(1 for n in v if n) == 2 and v[0] and v[-1] for v in per_word.values()), "no word of two frames with empty pieces between them"
            assert min(r[1] for r in live) < 40


# ---- device calls ------------------------------------------------------------------------------------------------------------------------------
def _view(be, keep):
    return keep[1] if be.name == "emu" else keep


def _upload(be, arena):
    ptr, keep = be.empty(len(arena))
    assert ptr % 16 == 0
    if be.name == "emu":
        keep[1][: len(arena)] = arena
    else:
        keep[: len(arena)] = be.torch.from_numpy(arena).to(be.dev)
    return ptr, keep


def fit_cap(nbytes):
    """the smallest dst_cap the rule admits for a stream of nbytes: whole 32-bit words are stored, the stream plus up to 7 bytes has to fit"""
    return (nbytes + 3) // 4 * 4 + 4


def splice_call(be, codec, parts, outs, src_mods=(0,), single=None):
    """parts: [(stream, from_block, to_block, out)] ; outs: [(header size[, dst_cap or None[, d_dst mod 16[, a stream of the call to lie on]]])].
    -> ([stream or None] per output, [(out_bytes, out_blocks, status)], [(blocks, bits, status)], return code). Asserts what must not be written.
    single: "concat" / "slice": through knz_dev_concat / knz_dev_slice (one output)"""
    at, cur, order = {}, GUARD, []
    for s, _f, _t, _o in parts:
        if s not in at:
            cur += (src_mods[len(order) % len(src_mods)] - cur) % 16
            at[s] = cur
            order.append(s)
            cur += len(s) + 3 + GUARD
    arena = np.full(cur + GUARD, FILL, dtype=np.uint8)
    for s in order:
        arena[at[s]: at[s] + len(s)] = np.frombuffer(s, dtype=np.uint8)
    sptr, skeep = _upload(be, arena)
    per = by_output(parts, len(outs))
    spans, cur = [], 0
    for o, spec in enumerate(outs):
        cap = spec[1] if len(spec) > 1 and spec[1] is not None else sum(len(s) for s, _f, _t in per[o]) + 64
        mod = spec[2] if len(spec) > 2 else (0, 4, 8, 12)[o % 4]
        lead = GUARD + mod
        size = (lead + cap + GUARD + 15) // 16 * 16
        spans.append((cur, lead, cap, size))
        cur += size
    dptr, dkeep = be.empty(cur)
    assert dptr % 16 == 0
    _view(be, dkeep)[:cur] = FILL
    call_outs = []
    for (base, lead, cap, _size), spec in zip(spans, outs):
        lie = spec[3] if len(spec) > 3 else None
        call_outs.append((sptr + at[lie], len(lie), spec[0]) if lie is not None else (dptr + base + lead, cap, spec[0]))
    call_parts = [(sptr + at[s], len(s), f, t, o) for s, f, t, o in parts]
    if single == "concat":
        assert len(outs) == 1 and all((f, t) == (1, END) for _s, f, t, _o in parts)
        nb = codec.dev_concat([p[0] for p in call_parts], [p[1] for p in call_parts], call_outs[0][0], call_outs[0][1], call_outs[0][2])
        ores, pres = [(nb, None, codec.last_many_rc)], []
    elif single == "slice":
        assert len(outs) == 1 and len(parts) == 1
        p = call_parts[0]
        nb = codec.dev_slice(p[0], p[1], p[2], p[3], call_outs[0][0], call_outs[0][1], call_outs[0][2])
        ores, pres = [(nb, None, codec.last_many_rc)], []
    else:
        ores, pres = codec.dev_splice_many(call_parts, call_outs)
    rc = codec.last_many_rc
    be.sync()
    assert be.to_host(skeep, len(arena)) == arena.tobytes(), "a source was written to"
    back = be.to_host(dkeep, cur)
    got = []
    for (base, lead, cap, size), (nb, _blocks, status) in zip(spans, ores):
        mine = back[base: base + size]
        if status != 0:
            assert nb == 0 and mine == bytes([FILL]) * size, ("an output that failed wrote to its destination", status)
            got.append(None)
            continue
        words = (nb + 3) // 4 * 4
        assert words + 4 <= cap or nb == 0, (nb, cap)
        assert mine[:lead] == bytes([FILL]) * lead and mine[lead + words:] == bytes([FILL]) * (size - lead - words), "bytes outside the stream's words were written"
        got.append(mine[lead: lead + nb])
    assert rc == next((s for _n, _b, s in ores if s), 0), (rc, [s for _n, _b, s in ores])
    return got, ores, pres, rc


def round_trip(be, codec, bs, streams, wants):
    """every stream through the device's decoder and the reference Reader: the concatenation of its parts' bytes. The device decodes block b at
    b * block_size before it packs short inner blocks: its destination holds that many whole blocks"""
    for s, w in zip(streams, wants):
        assert R.decompress(s, len(w) + 64) == w, "the reference Reader on a spliced stream"
    caps = [len(RC.frames(s)[1]) * bs + 64 for s in streams]
    if len(streams) > 8:
        back, rc = M.decompress_many(be, codec, list(zip(streams, caps)))
        assert rc == 0 and [b for b, _s in back] == list(wants), rc
        return
    for s, w, cap in zip(streams, wants, caps):
        got, rc = M.single_decompress(be, codec, s, cap)
        assert rc == 0 and got == w, (rc, "knz_dev_decompress on a spliced stream")


def check_case(be, codec, pipe, bs, parts, hss, cat=None, trip=True, **kw):
    """one call: every output equals the bit-splicer's stream (and the reference Writer's where `cat` is given), the results say what was taken"""
    per = by_output(parts, len(hss))
    got, ores, pres, rc = splice_call(be, codec, parts, [(hs,) for hs in hss], **kw)
    assert rc == 0, (pipe, bs, rc, ores, pres)
    for o, (ps, hs) in enumerate(zip(per, hss)):
        want = spliced(pipe, bs, ps, hs)
        assert got[o] == want, (pipe, bs, o, hs, M._diff(got[o], want))
        if cat is not None:
            assert got[o] == M.ref_stream(pipe, bs, cat, layout(pipe, bs, ps, hs)[0]), (pipe, bs, o, "!= the reference Writer's stream of the concatenation")
        if ores[o][1] is not None:
            assert ores[o][1] == sum(r[3] for r in layout(pipe, bs, ps, hs)[2]), (o, ores[o])
    if pres:
        flat = [r for ps, hs in zip(per, hss) for r in layout(pipe, bs, ps, hs)[2]]
        assert pres == [(b, n, 0) for _a, n, _d, b in flat], "blocks / bits of the parts"
    if trip:
        round_trip(be, codec, bs, got, [decoded(ps) for ps in per])
    return got


# ---- concat, slice --------------------------------------------------------------------------------------------------------------------------------
def check_concat(be, pipe, bs, lanes=None):
    codec = M.codec_for(be, pipe, bs, **({"devices": lanes} if lanes else {}))
    out = []
    for i, (name, (parts, hss, cat)) in enumerate(concat_cases(pipe, bs).items()):
        out += check_case(be, codec, pipe, bs, parts, hss, cat, trip=not name.startswith("identity, ") or name.endswith("no field"),
                          single="concat" if i % 2 == 0 else None, src_mods=(4 * i % 16, 8, 12, 0, 4))
    codec.close()
    return out


def check_slice(be, pipe, bs):
    codec = M.codec_for(be, pipe, bs)
    cases = slice_cases(pipe, bs)
    for i, (name, (parts, hss, _c)) in enumerate(cases.items()):
        got = check_case(be, codec, pipe, bs, parts, hss, single="slice" if i % 2 == 0 else None, src_mods=((4 * i) % 16,))
        if name == "the source back":
            assert got[0] == parts[0][0]
    # ... and every range in ONE call, one output each: the source is walked once
    parts = [(p[0][0], p[0][1], p[0][2], o) for o, (p, _h, _c) in enumerate(cases.values())]
    check_case(be, codec, pipe, bs, parts, [h[0] for _p, h, _c in cases.values()], trip=False)
    names = [n for n, _ms in codec.last_kernel_times()]
    assert [names.count(k) for k in ("knz_splice_walk_kernel", "knz_splice_plan_kernel", "knz_read_scan_kernel", "knz_splice_copy_kernel")] == [1, 1, 1, 1], names
    codec.close()


# ---- split and regroup, tiny frames and empty pieces ------------------------------------------------------------------------------------------------
def check_regroup(be, pipe=HUF, bs=1024):
    parts, hss = regroup_case(pipe, bs)
    assert len(hss) > 256 and max(len(ps) for ps in by_output(parts, len(hss))) > 256
    codec = M.codec_for(be, pipe, bs)
    check_case(be, codec, pipe, bs, parts, hss)
    codec.close()


def check_tiny(be, pipe):
    parts, hss = tiny_case(pipe)
    codec = M.codec_for(be, pipe, 1024)
    got = check_case(be, codec, pipe, 1024, parts, hss)
    assert got[1] == M.ref_stream(pipe, 1024, b"", 0) and got[2] == M.ref_stream(pipe, 1024, b"", 777)       # header + end marker, as the Writer writes them
    codec.close()


# ---- alignment and capacity -----------------------------------------------------------------------------------------------------------------------
def check_alignment(be, pipe, bs):
    s = five(pipe, bs)
    parts = [(s[1], 1, END, 0), (s[3], 2, 3, 0), (s[2], 1, END, 0), (s[0], 1, 4, 0)]
    want = spliced(pipe, bs, [p[:3] for p in parts], 0)
    fit = fit_cap(len(want))
    codec = M.codec_for(be, pipe, bs)
    for i, mod in enumerate((0, 4, 8, 12)):
        mods = tuple((mod + 4 * j) % 16 for j in range(4))
        got, ores, _pres, rc = splice_call(be, codec, parts, [(0, fit, mod)], src_mods=mods)
        assert rc == 0 and got[0] == want, (pipe, bs, mod, rc, None if got[0] is None else M._diff(got[0], want))
        got, ores, _pres, rc = splice_call(be, codec, parts, [(0, fit - 1, mod)], src_mods=mods)
        assert rc == ERR_WRITE_FILE and got[0] is None and ores[0] == (0, 0, ERR_WRITE_FILE), (mod, rc, ores)
    for cap in (7, 0):
        assert splice_call(be, codec, parts, [(0, cap, 4)])[3] == ERR_WRITE_FILE
    codec.close()


# ---- trouble: many outputs in one call ------------------------------------------------------------------------------------------------------------
def check_trouble(be, pipe=HUF, bs=1024):
    assert pipe[2] == 32
    s = five(pipe, bs)
    m = s[0]
    cut = as_clean(m[:-1], m)                                               # the end marker cut off
    other = main(RC.PIPELINES[2], bs)                                       # another configuration
    codec = M.codec_for(be, pipe, bs)
    cp, _kc = be.to_dev(cut, 4)
    try:
        codec.dev_stream_index(cp, len(cut))
        raise AssertionError("the truncated stream was walked to an end marker")
    except K.KnzError as e:
        walk = e.code
    parts = [(s[1], 1, END, 0), (s[2], 1, END, 0),
             (s[1], 1, END, 1), (cut, 3, END, 1),
             (m, 4, 9, 2),
             (other, 1, 3, 3), (s[3], 1, END, 3),
             (s[3], 1, END, 4), (m, 0, 3, 4),
             (s[4], 1, END, 5),
             (s[2], 1, 3, 6), (s[4], 2, 3, 6),
             (m, 9, 12, 7), (s[1], 1, END, 7), (m, 1, 3, 7)]
    small = fit_cap(len(spliced(pipe, bs, [(s[4], 1, END)], KEEP))) - 1
    outs = [(KEEP,), (KEEP,), (0,), (KEEP,), (KEEP,), (KEEP, small), (KEEP, None, 0, s[2]), (5,)]
    codes = {1: walk, 3: ERR_INVALID_PARAM, 4: ERR_INVALID_PARAM, 5: ERR_WRITE_FILE, 6: ERR_INVALID_PARAM}
    got, ores, pres, rc = splice_call(be, codec, parts, outs)
    assert [st for _n, _b, st in ores] == [codes.get(o, 0) for o in range(8)], (ores, codes)
    assert rc == walk
    assert [st for _b, _n, st in pres] == [0, 0, 0, walk, 0, ERR_INVALID_PARAM, 0, 0, ERR_INVALID_PARAM, 0, 0, 0, 0, 0, 0], pres
    per = by_output(parts, 8)
    for o in (0, 2, 7):
        want = spliced(pipe, bs, per[o], outs[o][0])
        alone, _o, _p, arc = splice_call(be, codec, [(x, f, t, 0) for x, f, t in per[o]], [outs[o]])
        assert arc == 0 and got[o] == want == alone[0], (o, arc)
    # the finite range in front of the cut does not see it
    got, ores, _p, rc = splice_call(be, codec, [(cut, 3, 30, 0)], [(0,)], single="slice")
    assert rc == 0 and got[0] == spliced(pipe, bs, [(cut, 3, 30)], 0)
    codec.close()


# ---- damage carried, not checked ------------------------------------------------------------------------------------------------------------------
def check_damage(be, pipe=HUF, bs=1024):
    assert pipe[2] == 32
    m = main(pipe, bs)
    fr = _frames(m)[1]
    hurt = bytearray(m)
    hurt[(fr[4][1] + fr[4][2] // 2) // 8] ^= 0x10                           # the middle of block 5's payload
    hurt = as_clean(bytes(hurt), m)
    broken = bytearray(m)
    broken[(fr[10][0] + 5) // 8] ^= 0x80 >> ((fr[10][0] + 5) % 8)          # block 11's length field (its leading bit: the walk lands inside the payload)
    broken = as_clean(bytes(broken), m)
    codec = M.codec_for(be, pipe, bs)
    bp, _kb = be.to_dev(broken, 4)
    try:
        codec.dev_stream_index(bp, len(broken))
        raise AssertionError("the damaged framing was walked to an end marker")
    except K.KnzError as e:
        walk = e.code
    bad, rc = M.single_decompress(be, codec, hurt, len(_DATA[m][0]) + 64)
    assert rc != 0, "the flipped payload bit decodes"
    # one call: the flipped block inside a range, the broken field behind a finite range, the same source through KNZ_BLOCK_END
    parts = [(hurt, 3, 9, 0), (broken, 2, 8, 1), (broken, 2, END, 2), (broken, 10, 11, 3)]
    got, ores, pres, rc = splice_call(be, codec, parts, [(0,), (KEEP,), (KEEP,), (0,)])
    assert [st for _n, _b, st in ores] == [0, 0, walk, 0] and rc == walk, (ores, walk)
    assert got[0] == spliced(pipe, bs, [(hurt, 3, 9)], 0) and got[0] != spliced(pipe, bs, [(m, 3, 9)], 0)
    assert got[1] == spliced(pipe, bs, [(m, 2, 8)], 0) and got[3] == spliced(pipe, bs, [(m, 10, 11)], 0)
    round_trip(be, codec, bs, [got[1], got[3]], [decoded([(m, 2, 8)]), decoded([(m, 10, 11)])])
    codec.close()


# ---- skip / copy blocks, short inner block -----------------------------------------------------------------------------------------------------------
def check_skip(be, pipe, bs=1024):
    sk = known(*RC.skip_stream(pipe, bs))
    cp = RC.copy_blocks(sk)
    n = len(_frames(sk)[1])
    assert cp and 2 in cp
    codec = M.codec_for(be, pipe, bs)
    got = check_case(be, codec, pipe, bs, [(sk, 1, END, 0), (sk, 1, END, 0), (sk, 2, 6, 1), (sk, 2, 3, 2)], [KEEP, 0, 0])
    assert RC.copy_blocks(got[0]) == cp + [c + n for c in cp], "the mode bytes did not travel"
    assert RC.copy_blocks(got[1]) == [c - 1 for c in cp if 2 <= c < 6] and RC.copy_blocks(got[2]) == [1]
    codec.close()


def check_short_inner(be, pipe):
    bs = RC.SHORT_BS
    a, b = RC.short_parts(bs)
    sa, sb = known(a, RC._ref(pipe, bs, a), [0, bs, len(a)]), known(b, RC._ref(pipe, bs, b), [0, bs, 2 * bs, len(b)])
    codec = M.codec_for(be, pipe, bs)
    got = check_case(be, codec, pipe, bs, whole([sa, sb]), [KEEP])
    assert got[0] == RC.short_inner_stream(pipe)[1]                         # (KEEP: both have the field, the sum is the whole length)
    gp, _kg = be.to_dev(got[0], 4)
    info, pos = codec.dev_stream_index(gp, len(got[0]))
    assert info["n_blocks"] == 5 and info["output_size"] == len(a) + len(b)
    codec.close()


# ---- counters, contract --------------------------------------------------------------------------------------------------------------------------------
def check_counters(be, pipe=HUF, bs=1024):
    m = main(pipe, bs)
    codec = M.codec_for(be, pipe, bs)
    data = _DATA[m][0]
    assert M.single_decompress(be, codec, m, len(data) + 64) == (data, 0) and codec.last_counter(COUNTER_DECODE_BLOCKS) == RC.BLOCKS + 1
    check_case(be, codec, pipe, bs, [(m, 2, 9, 0), (m, 1, END, 1)], [0, KEEP], trip=False)
    assert codec.last_counter(COUNTER_DECODE_BLOCKS) == 0 and codec.last_counter(COUNTER_ENCODE_BLOCKS) == 0
    codec.close()


def check_contract(be):
    pipe, bs = HUF, 1024
    m = main(pipe, bs)
    codec = M.codec_for(be, pipe, bs)
    L = codec.L
    sp, _k = be.to_dev(m, 4)
    cap = (len(m) + 64) // 16 * 16
    back, kb = be.empty(2 * cap + 64)
    _view(be, kb)[: 2 * cap + 64] = FILL
    out = C.c_uint64(77)
    ob = C.byref(out)
    p, o = (Part * 2)(), (Out * 2)()

    def fill():
        for i in range(2):
            p[i].d_src, p[i].n_bytes, p[i].from_block, p[i].to_block, p[i].out = sp, len(m), 1 + i, 4, i
            o[i].d_dst, o[i].dst_cap, o[i].header_input_size = back + i * cap, cap, 0

    def untouched():
        be.sync()
        return be.to_host(kb, 2 * cap + 64) == bytes([FILL]) * (2 * cap + 64)

    fill()
    assert L.knz_dev_splice_many(None, p, 2, o, 2, None) == ERR_MISSING_PARAM
    assert L.knz_dev_splice_many(codec.h, p, 2, o, 0, None) == 0 and L.knz_dev_splice_many(codec.h, None, 0, None, -1, None) == 0
    assert L.knz_dev_splice_many(codec.h, p, 2, None, 2, None) == ERR_MISSING_PARAM
    assert L.knz_dev_splice_many(codec.h, None, 2, o, 2, None) == ERR_MISSING_PARAM
    for a, b in ((1, 0), (0, 2)):                                           # out decreasing, out of range: the call, nothing written
        fill()
        p[0].out, p[1].out = a, b
        assert L.knz_dev_splice_many(codec.h, p, 2, o, 2, None) == ERR_INVALID_PARAM and [o[0].status, o[1].status] == [ERR_INVALID_PARAM] * 2
        assert [o[0].out_bytes, o[1].out_bytes] == [0, 0] and untouched()
    for f, t in ((0, 3), (0, 0xFFFFFFFF), (3, 3), (4, 2), (0xFFFFFFFF, 0xFFFFFFFF)):
        fill()
        p[1].from_block, p[1].to_block = f, t
        assert L.knz_dev_splice_many(codec.h, p, 2, o, 2, None) == ERR_INVALID_PARAM and (p[0].status, p[1].status) == (0, ERR_INVALID_PARAM), (f, t)
        assert (o[0].status, o[1].status) == (0, ERR_INVALID_PARAM) and o[0].out_bytes != 0 and o[1].out_bytes == 0
    _view(be, kb)[: 2 * cap + 64] = FILL
    fill()
    p[0].d_src = None
    assert L.knz_dev_splice_many(codec.h, p, 2, o, 2, None) == ERR_MISSING_PARAM and (p[0].status, o[0].status, o[1].status) == (ERR_MISSING_PARAM, ERR_MISSING_PARAM, 0)
    fill()
    p[0].d_src, p[0].n_bytes = sp + 1, len(m) - 1
    assert L.knz_dev_splice_many(codec.h, p, 2, o, 2, None) == ERR_INVALID_PARAM and (p[0].status, o[0].status, o[1].status) == (ERR_INVALID_PARAM, ERR_INVALID_PARAM, 0)
    _view(be, kb)[: 2 * cap + 64] = FILL
    fill()
    o[1].d_dst = None
    assert L.knz_dev_splice_many(codec.h, p, 2, o, 2, None) == ERR_MISSING_PARAM and (o[0].status, o[1].status) == (0, ERR_MISSING_PARAM)
    _view(be, kb)[: 2 * cap + 64] = FILL
    for d1, c1 in ((back + cap + 2, cap - 2), (back + cap - 4, cap), (back, cap), (sp + 8, 16)):      # off 4 bytes ; on the other output ; on a source
        _view(be, kb)[: 2 * cap + 64] = FILL
        fill()
        o[1].d_dst, o[1].dst_cap = d1, c1
        rc = L.knz_dev_splice_many(codec.h, p, 2, o, 2, None)
        assert rc == ERR_INVALID_PARAM and o[1].status == ERR_INVALID_PARAM and o[1].out_bytes == 0, (d1 - back, rc)
        assert o[0].status == (ERR_INVALID_PARAM if back <= d1 < back + cap else 0)
        if o[0].status:
            assert untouched()
    _view(be, kb)[: 2 * cap + 64] = FILL
    # the single calls
    srcs, lens = (C.c_void_p * 2)(sp, sp), (C.c_uint64 * 2)(len(m), len(m))
    assert L.knz_dev_concat(None, srcs, lens, 2, 0, back, 2 * cap, ob, None) == ERR_MISSING_PARAM
    assert L.knz_dev_concat(codec.h, srcs, lens, 2, 0, back, 2 * cap, None, None) == ERR_MISSING_PARAM
    assert L.knz_dev_concat(codec.h, None, lens, 2, 0, back, 2 * cap, ob, None) == ERR_MISSING_PARAM and out.value == 0
    assert L.knz_dev_concat(codec.h, srcs, lens, 2, 0, None, 2 * cap, ob, None) == ERR_MISSING_PARAM
    assert L.knz_dev_slice(codec.h, sp, len(m), 2, 4, 0, back, cap, None, None) == ERR_MISSING_PARAM
    assert L.knz_dev_slice(codec.h, None, len(m), 2, 4, 0, back, cap, ob, None) == ERR_MISSING_PARAM
    assert L.knz_dev_slice(codec.h, sp, len(m), 0, 4, 0, back, cap, ob, None) == ERR_INVALID_PARAM and out.value == 0
    assert untouched()
    assert L.knz_dev_concat(codec.h, None, None, 0, 0, back, cap, ob, None) == 0                    # no sources: header + end marker
    be.sync()
    assert be.to_host(kb, out.value) == M.ref_stream(pipe, bs, b"", 0)
    assert L.knz_dev_slice(codec.h, sp, len(m), 2, 4, 0, back, cap, ob, None) == 0                  # ... and the handle still works
    be.sync()
    assert be.to_host(kb, out.value) == spliced(pipe, bs, [(m, 2, 4)], 0)
    # a handle whose configuration differs from the source's header, in each of the four fields
    for other, obs in ((("LZ", "HUFFMAN", 32, False), bs), (("NONE", "ANS0", 32, False), bs), (pipe, 2 * bs), (("NONE", "HUFFMAN", 64, False), bs)):
        c2 = M.codec_for(be, other, obs)
        got, ores, pres, rc = splice_call(be, c2, [(m, 1, END, 0)], [(KEEP,)])
        assert rc == ERR_INVALID_PARAM and pres == [(0, 0, ERR_INVALID_PARAM)], (other, obs, rc)
        c2.close()
    try:
        codec.dev_slice(sp, len(m), 0, 3, back, cap, check=True)
        raise AssertionError("check=True did not raise")
    except K.KnzError as e:
        assert e.code == ERR_INVALID_PARAM
    codec.close()
