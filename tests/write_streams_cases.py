"""knz_dev_write_streams: byte writes into many .knz streams in one device batch. Cases shared by the emulator run (tests/test_write_streams_emu.py) and
the MI355X run (tests/test_write_streams_gpu.py). A target is what tests/write_cases.py calls a case: a source stream of the reference Writer, writes, a
header size. What a target has to deliver is said twice: by the existing single call for that target alone (write_cases.write_call: bytes, out_bytes,
status, write statuses) and by the reference Writer's stream for the edited input (write_cases.expected_stream).

All outputs of a call are packed into ONE arena filled with a known byte, guards on both sides: target k's d_dst starts at the first 4-byte boundary
behind target k - 1's dst_cap. After the call every byte outside the 32-bit words of the good streams has to be that byte still: the gap between a
stream's last word and its dst_cap, the gaps between the targets, the whole range of a failed target."""
import ctypes as C
import functools

import numpy as np

import many_cases as M
import range_cases as RC
import write_cases as WR

K = RC.K
END, KEEP = WR.END, WR.KEEP
GUARD, FILL = WR.GUARD, WR.FILL
GRID_PIPE, XF_PIPE = WR.GRID_PIPE, WR.XF_PIPE
ERR_MISSING_PARAM, ERR_WRITE_FILE, ERR_INVALID_PARAM = WR.ERR_MISSING_PARAM, WR.ERR_WRITE_FILE, WR.ERR_INVALID_PARAM
assert hasattr(K.api, "_WriteTarget") and hasattr(K.api, "_WriteTo")       # (the binding of the call: nothing here runs without it)


class Target:
    """one target of a call: source stream (and its data), writes [(offset, data)], header size ; cap None: write_cases.out_cap ; share: targets with
    the same key name one d_src ; dst: "arena" (packed), "null", or "source" (d_dst = its own d_src: an overlap)"""

    def __init__(self, name, data, stream, writes, header_size=KEEP, cap=None, share=None, dst="arena"):
        self.name, self.data, self.stream, self.writes, self.header_size, self.cap, self.share, self.dst = name, data, stream, writes, header_size, cap, share, dst


# ---- the case lists (pure) ---------------------------------------------------------------------------------------------------------------------
EQUIV_BOUNDARY = ("several boundaries", "inside the ragged block", "one whole block", "three blocks and five bytes past L", "END, full blocks",
                  "END, empty stream", "append of nothing")
EQUIV_ORDER = ("overlap, same range, nested", "an offset inside an earlier write's growth")
EQUIV_HEADER = ("none -> true size", "KEEP, field, growth (16 -> 32 bits at 1024)", "none -> 32 bits", "KEEP, a block grows or shrinks")


def equivalence_targets(pipe, bs):
    """about a dozen targets of write_cases' lists, and two streams of a few words: header sizes KEEP, 0 and explicit values inside one call"""
    out = []
    bc, oc, hc = WR.boundary_cases(bs), WR.order_cases(bs), WR.header_cases(bs)
    for name in EQUIV_BOUNDARY:
        n, writes = bc[name]
        data, stream = WR.source(pipe, bs, n)
        hs = 0 if name == "append of nothing" else KEEP
        out.append(Target(name, data, stream, writes, hs, share="main" if name in ("several boundaries", "inside the ragged block") else None))
    for name in EQUIV_ORDER:
        n, writes = oc[name]
        data, stream = WR.source(pipe, bs, n)
        out.append(Target(name, data, stream, writes))
    for name in EQUIV_HEADER:
        n, hs, writes, hsz = hc[name]
        data, stream = WR.source(pipe, bs, n, hs)
        out.append(Target(name, data, stream, writes, hsz))
    n, p = RC.BLOCKS * bs + RC.TAIL, WR.payload
    data, stream = WR.source(pipe, bs, n)                                   # blocks that change their size: every run behind one moves by some number of bits
    out.append(Target("text and zeros over three blocks", data, stream, [(bs, p(bs, 46, text=True)), (19 * bs + 50, bytes(700)), (30 * bs, p(bs, 47, text=True))], n + 1))
    out.append(Target("text and random bytes over three blocks", data, stream, [(6 * bs, p(bs, 48, text=True)), (11 * bs + 3, p(500, 49)), (25 * bs, p(bs, 51, text=True))]))
    empty, estream = WR.source(pipe, bs, 0)
    out.append(Target("one byte into an empty stream", empty, estream, [(END, WR.payload(1, 50))], 0))
    out.append(Target("nothing into an empty stream", empty, estream, [(END, b"")], 0))
    return out


def new_blocks(t, bs):
    edited = WR.apply(t.data, t.writes)
    return max(0, (len(edited) + bs - 1) // bs - (len(t.data) + bs - 1) // bs)


def check_coverage(pipes=(GRID_PIPE, XF_PIPE), bs=1024):
    """what one call of the equivalence case meets, from the reference streams alone"""
    for pipe in pipes:
        ts = equivalence_targets(pipe, bs)
        shifts, sizes = set(), []
        for t in ts:
            _e, new = WR.expected_stream(pipe, bs, t.data, t.stream, t.writes, t.header_size)
            shifts |= WR.run_shifts(t.stream, new, WR.touched_blocks(len(t.data), bs, t.writes))
            sizes.append(len(new))
        assert len(shifts) >= 8 and 0 in shifts and any(s for s in shifts), (pipe, sorted(shifts))
        assert any(s <= 32 for s in sizes), (pipe, min(sizes))                                    # a new stream of at most 8 words
        assert any(new_blocks(t, bs) >= 3 for t in ts)
        assert any(WR.touched_blocks(len(t.data), bs, t.writes) == {(len(t.data) + bs - 1) // bs - 1} and len(t.data) > bs for t in ts)
        assert {t.header_size for t in ts} >= {KEEP, 0} and any(t.header_size > 0 for t in ts)
        assert sum(1 for t in ts if t.share == "main") == 2


# ---- the call -----------------------------------------------------------------------------------------------------------------------------------
def _view(be, keep):
    return keep[1] if be.name == "emu" else keep


def _fill(be, keep, arena):
    if be.name == "emu":
        keep[1][: len(arena)] = arena
    else:
        keep[: len(arena)] = be.torch.from_numpy(arena).to(be.dev)


def interleaved(targets):
    """[(target, index of its write)]: the writes of the targets taken in turns, every target's own in index order"""
    rows, j = [], 0
    while any(j < len(t.writes) for t in targets):
        rows += [(k, j) for k, t in enumerate(targets) if j < len(t.writes)]
        j += 1
    return rows


def streams_call(be, codec, targets, dst_mod=4, rows=None):
    """-> ([(new stream or None, status, [write status])] per target, return code, [d_dst]). Asserts what must not be written."""
    keep, shared, srcs = [], {}, []
    for t in targets:
        if t.share is None or t.share not in shared:
            shared[t.share if t.share is not None else len(keep)] = be.to_dev(t.stream, 4)
        sp, ks = shared[t.share if t.share is not None else len(keep)]
        keep.append(ks)
        srcs.append(sp)
    rows = interleaved(targets) if rows is None else rows
    at, cur = {}, GUARD
    for i, (k, j) in enumerate(rows):
        cur += GUARD
        cur += ((5 * i + 1) % 16 - cur) % 16
        at[(k, j)] = cur
        cur += len(targets[k].writes[j][1])
    dsize = cur + 2 * GUARD
    dptr, dkeep = be.empty(dsize)
    arena = np.full(dsize, FILL, dtype=np.uint8)
    for (k, j), a in at.items():
        d = targets[k].writes[j][1]
        arena[a: a + len(d)] = np.frombuffer(d, dtype=np.uint8)
    _fill(be, dkeep, arena)
    caps = [WR.out_cap(t.stream, t.writes) if t.cap is None else t.cap for t in targets]
    place, cur = [], GUARD + dst_mod
    for t, cap in zip(targets, caps):
        if t.dst != "arena":
            place.append(None)
            continue
        cur = (cur + 3) // 4 * 4
        place.append(cur)
        cur += cap
    size = cur + 16 + GUARD
    optr, okeep = be.empty(size)
    assert optr % 16 == 0
    _view(be, okeep)[:size] = FILL
    call, dsts = [], []
    for k, t in enumerate(targets):
        dst = {"arena": None, "null": None, "source": srcs[k]}[t.dst] if t.dst != "arena" else optr + place[k]
        cap = len(t.stream) // 4 * 4 if t.dst == "source" else caps[k]
        call.append((srcs[k], len(t.stream), dst, cap, t.header_size))
        dsts.append(dst)
    res, wst = codec.dev_write_streams(call, [(k, targets[k].writes[j][0], len(targets[k].writes[j][1]), dptr + at[(k, j)]) for k, j in rows])
    rc = codec.last_many_rc
    be.sync()
    got = bytearray(be.to_host(okeep, size))
    out = []
    for k, t in enumerate(targets):
        nb, status = res[k]
        st = [wst[i] for i, (kk, _j) in enumerate(rows) if kk == k]
        if status != 0 or not t.writes:
            assert nb == 0, (t.name, nb, status)
            out.append((None, status, st))
            continue
        assert t.dst == "arena" and nb <= caps[k], (t.name, nb, caps[k])
        words = (nb + 3) // 4 * 4
        out.append((bytes(got[place[k]: place[k] + nb]), 0, st))
        got[place[k]: place[k] + words] = bytes([FILL]) * words
    assert bytes(got) == bytes([FILL]) * size, "bytes outside the good streams' own words were written"
    for k, t in enumerate(targets):
        if t.dst == "source":
            assert be.to_host(keep[k], len(t.stream)) == t.stream, "a source was written"
    assert be.to_host(dkeep, dsize) == arena.tobytes()
    failed = [s for _g, s, _st in out if s]
    assert rc == (failed[0] if failed else 0), (rc, failed)
    return out, rc, dsts


_SINGLE = {}


def single(be, codec, pipe, bs, t, tag=""):
    """write_cases.write_call for this target alone (once per backend, pipeline, block size and target)"""
    key = (be.name, pipe, bs, t.name, t.cap, t.header_size, tag)
    if key not in _SINGLE:
        _SINGLE[key] = WR.write_call(be, codec, t.stream, t.writes, t.header_size, cap=t.cap)
    return _SINGLE[key]


def compare(be, codec, pipe, bs, targets, results, decode=False):
    """every target against its single call, the healthy ones against the reference Writer's stream as well ; returns how many were compared"""
    done = 0
    for t, (got, status, st) in zip(targets, results):
        want, wst, wrc = single(be, codec, pipe, bs, t)
        assert (got, status, st) == (want, wrc, wst), (t.name, status, wrc, st, wst, None if got is None or want is None else M._diff(got, want))
        if wrc == 0:
            edited, ref = WR.expected_stream(pipe, bs, t.data, t.stream, t.writes, t.header_size)
            assert got == ref, (t.name, M._diff(got, ref))
            if decode:
                sp, _k = be.to_dev(got, 4)
                dst, kd = be.empty(len(edited) + 64)
                assert codec.dev_decompress(sp, len(got), dst, len(edited) + 64) == len(edited)
                be.sync()
                assert be.to_host(kd, len(edited)) == edited, t.name
        done += 1
    return done


# ---- 1. equivalence, 9. schedules ---------------------------------------------------------------------------------------------------------------
def check_equivalence(be, pipe, bs, lanes=None, decode=True):
    targets = equivalence_targets(pipe, bs)
    codec = M.codec_for(be, pipe, bs, **({"devices": lanes} if lanes else {}))
    res, rc, _d = streams_call(be, codec, targets)
    assert rc == 0
    assert compare(be, codec, pipe, bs, targets, res, decode) == len(targets)
    codec.close()
    return [g for g, _s, _st in res]


# ---- 3. placement ---------------------------------------------------------------------------------------------------------------------------------
def placement_targets(pipe=GRID_PIPE, bs=1024):
    """eight targets whose dst_cap lets the next d_dst fall on 4 k mod 16: the stream's words, the spare word of the dst_cap rule, 0 .. 15 bytes more"""
    names = ("several boundaries", "END, empty stream", "one whole block", "append of one byte", "END, ragged", "inside the ragged block", "one boundary", "ending at L")
    bc = WR.boundary_cases(bs)
    out, cur = [], GUARD
    for k, name in enumerate(names):
        n, writes = bc[name]
        data, stream = WR.source(pipe, bs, n)
        _e, new = WR.expected_stream(pipe, bs, data, stream, writes)
        fit = (len(new) + 3) // 4 * 4 + 4
        cap = fit + (4 * (k + 1) - (cur + fit)) % 16 - (1 if k % 3 == 2 else 0)                # (k % 3 == 2: a dst_cap off 4 bytes, the next d_dst behind it)
        out.append(Target(name, data, stream, writes, cap=cap))
        cur = (cur + cap + 3) // 4 * 4
    return out


def check_placement(be, pipe=GRID_PIPE, bs=1024):
    targets = placement_targets(pipe, bs)
    codec = M.codec_for(be, pipe, bs)
    res, rc, dsts = streams_call(be, codec, targets, dst_mod=0)
    assert rc == 0 and {d % 16 for d in dsts} == {0, 4, 8, 12}, (rc, [d % 16 for d in dsts])
    ends = [d + (len(g) + 3) // 4 * 4 for d, (g, _s, _st) in zip(dsts, res)]
    assert any((e - 4) // 16 == d // 16 for e, d in zip(ends, dsts[1:])), "no output's last word shares a 16-byte line with the next output's first"
    for t, (got, status, _st) in zip(targets, res):
        _e, ref = WR.expected_stream(pipe, bs, t.data, t.stream, t.writes, t.header_size)
        assert status == 0 and got == ref, (t.name, status)
    codec.close()


# ---- 4. isolation ---------------------------------------------------------------------------------------------------------------------------------
def short_inner(pipe, bs):
    """range_cases.short_inner_stream at this block size: the frames of two reference streams behind one header, block 2 is short"""
    a, b = RC.P.corpus(bs + 321, 7), RC.P.corpus(2 * bs + 99, 8)
    return a + b, RC.splice_streams(RC._ref(pipe, bs, a + b, len(a) + len(b)), [RC._ref(pipe, bs, a), RC._ref(pipe, bs, b)])


def isolation_targets(pipe=GRID_PIPE, bs=1024):
    """-> [(target, expected (status, write statuses) or None: the single call says)], failing ones first, in the middle and last"""
    assert pipe[2] == 32
    p = WR.payload
    n = RC.BLOCKS * bs + RC.TAIL
    data, stream = WR.source(pipe, bs, n)
    _info, fr, _end = RC.frames(stream)
    hurt = bytearray(stream)
    hurt[(fr[4][1] + fr[4][2] // 2) // 8] ^= 0x10                           # write_cases.check_damage's fixture: the middle of block 5's payload
    hurt = bytes(hurt)
    bc = WR.boundary_cases(bs)
    healthy = [Target(name, *WR.source(pipe, bs, bc[name][0]), bc[name][1]) for name in ("one boundary", "END, ragged", "one whole block", "one byte past L")]
    small = [(3 * bs + 5, p(40, 2))]
    _e, want = WR.expected_stream(pipe, bs, data, stream, small)
    odata, ostream = WR.source(RC.PIPELINES[2], bs, n)
    sdata, sstream = short_inner(pipe, bs)
    two = [(2 * bs, p(10, 2)), (4 * bs + 10, p(20, 1)), (9 * bs, p(5, 4))]
    return [(Target("damaged touched block", data, hurt, two), None),
            (healthy[0], None),
            (Target("hole", data, stream, [(10, p(10, 61)), (END, p(5, 62)), (n + 6, p(3, 63)), (0, p(1, 64))]), None),
            (Target("dst_cap one word short", data, stream, small, cap=(len(want) + 3) // 4 * 4), None),
            (healthy[1], None),
            (Target("source of another pipeline", odata, ostream, small), None),
            (Target("NULL d_dst", data, stream, small, dst="null"), (ERR_MISSING_PARAM, [0])),
            (healthy[2], None),
            (Target("d_dst overlaps a source", data, stream, small, dst="source"), (ERR_INVALID_PARAM, [ERR_INVALID_PARAM])),
            (healthy[3], None),
            (Target("short inner block", sdata, sstream, [(bs + 10, p(20, 1))]), None)]


def check_isolation(be, pipe=GRID_PIPE, bs=1024):
    cases = isolation_targets(pipe, bs)
    targets = [t for t, _w in cases]
    codec = M.codec_for(be, pipe, bs)
    res, rc, _d = streams_call(be, codec, targets)
    done, failed = 0, 0
    for (t, fixed), (got, status, st) in zip(cases, res):
        if t.name == "NULL d_dst":                                          # (the single call with the same arguments: it does not look at the writes)
            sp, _k = be.to_dev(t.stream, 4)
            dp, _kd = be.to_dev(t.writes[0][1])
            nb, sst = codec.dev_write_many(sp, len(t.stream), [(t.writes[0][0], len(t.writes[0][1]), dp)], None, 1 << 20)
            assert (nb, codec.last_many_rc, sst) == (0,) + fixed
        if fixed is not None:
            assert (got, status, st) == (None,) + fixed, (t.name, status, st)
            done += 1
        else:
            done += compare(be, codec, pipe, bs, [t], [(got, status, st)])
        failed += status != 0
    assert done == len(targets) == 11 and failed == 7, (done, failed)
    assert rc == res[0][1] != 0
    codec.close()


# ---- 5. counters ------------------------------------------------------------------------------------------------------------------------------------
def check_counters(be, pipe=GRID_PIPE, bs=1024):
    bc = WR.boundary_cases(bs)
    names = ("several boundaries", "one boundary", "END, empty stream", "three blocks and five bytes past L", "one whole block")
    targets = [Target(name, *WR.source(pipe, bs, bc[name][0]), bc[name][1]) for name in names]
    touched = [len(WR.touched_blocks(len(t.data), bs, t.writes)) for t in targets]
    assert len(set(touched)) >= 3, touched
    codec = M.codec_for(be, pipe, bs)
    res, rc, _d = streams_call(be, codec, targets)
    assert rc == 0 and all(s == 0 for _g, s, _st in res)
    got = codec.last_counter(WR.COUNTER_DECODE_BLOCKS), codec.last_counter(WR.COUNTER_ENCODE_BLOCKS)
    assert got == (sum(touched), sum(touched) + sum(new_blocks(t, bs) for t in targets)), (got, touched)
    codec.close()


# ---- 6. contract ------------------------------------------------------------------------------------------------------------------------------------
def check_contract(be, pipe=GRID_PIPE, bs=1024):
    n = RC.BLOCKS * bs + RC.TAIL
    data, stream = WR.source(pipe, bs, n)
    codec = M.codec_for(be, pipe, bs)
    L = codec.L
    WT, WTo = K.api._WriteTarget, K.api._WriteTo
    sp, _k = be.to_dev(stream, 4)
    dp, _kd = be.to_dev(WR.payload(64, 1))
    cap = WR.out_cap(stream, [])
    back, kb = be.empty(3 * cap)
    _view(be, kb)[: 3 * cap] = FILL

    def fresh(m=3):
        ts, ws = (WT * 3)(), (WTo * 3)()
        for k in range(3):
            ts[k].d_src, ts[k].n_bytes, ts[k].d_dst, ts[k].dst_cap, ts[k].header_input_size = sp, len(stream), back + k * cap, cap, KEEP
            ts[k].out_bytes, ts[k].status = 77, 77
        for i in range(m):
            ws[i].target, ws[i].offset, ws[i].length, ws[i].d_data, ws[i].status = i, 10 + i, 20, dp, 77
        return ts, ws

    def untouched():
        be.sync()
        return be.to_host(kb, 3 * cap) == bytes([FILL]) * (3 * cap)

    ts, ws = fresh()
    assert L.knz_dev_write_streams(None, ts, 3, ws, 3, None) == ERR_MISSING_PARAM
    assert L.knz_dev_write_streams(codec.h, ts, 0, ws, 3, None) == 0 and L.knz_dev_write_streams(codec.h, ts, -1, ws, 3, None) == 0
    assert L.knz_dev_write_streams(codec.h, None, 3, ws, 3, None) == ERR_MISSING_PARAM
    assert L.knz_dev_write_streams(codec.h, ts, 3, None, 3, None) == ERR_MISSING_PARAM
    assert untouched()
    # n_writes 0: every target is the single call's n_writes <= 0
    assert L.knz_dev_write_streams(codec.h, ts, 3, None, 0, None) == 0
    assert [(t.status, t.out_bytes) for t in ts] == [(0, 0)] * 3 and untouched()
    # a target index out of range: the call is malformed
    ts, ws = fresh()
    ws[1].target = 3
    assert L.knz_dev_write_streams(codec.h, ts, 3, ws, 3, None) == ERR_INVALID_PARAM
    assert [t.status for t in ts] == [ERR_INVALID_PARAM] * 3 and [w.status for w in ws] == [ERR_INVALID_PARAM] * 3 and [t.out_bytes for t in ts] == [0] * 3
    assert untouched()
    # a target no write names, between two that are named
    ts, ws = fresh(2)
    ws[1].target = 2
    assert L.knz_dev_write_streams(codec.h, ts, 3, ws, 2, None) == 0
    assert [t.status for t in ts] == [0] * 3 and ts[1].out_bytes == 0 and ts[0].out_bytes != 0 and ts[2].out_bytes != 0 and [w.status for w in ws][:2] == [0, 0]
    be.sync()
    got = be.to_host(kb, 3 * cap)
    assert got[cap: 2 * cap] == bytes([FILL]) * cap
    for k, (o, d) in ((0, (10, 20)), (2, (11, 20))):
        _e, want = WR.expected_stream(pipe, bs, data, stream, [(o, WR.payload(64, 1)[:d])])
        assert got[k * cap: k * cap + ts[k].out_bytes] == want
    _view(be, kb)[: 3 * cap] = FILL
    # overlapping destinations: both fail, the third completes
    ts, ws = fresh()
    ts[1].d_dst = back + cap - 4
    assert L.knz_dev_write_streams(codec.h, ts, 3, ws, 3, None) == ERR_INVALID_PARAM
    assert [t.status for t in ts] == [ERR_INVALID_PARAM, ERR_INVALID_PARAM, 0] and [w.status for w in ws] == [ERR_INVALID_PARAM, ERR_INVALID_PARAM, 0]
    assert ts[2].out_bytes != 0 and ts[0].out_bytes == 0 and ts[1].out_bytes == 0
    be.sync()
    assert be.to_host(kb, 2 * cap) == bytes([FILL]) * (2 * cap)
    _view(be, kb)[: 3 * cap] = FILL
    # a NULL d_data with length > 0 fails only its target ; d_src off 4 bytes: the single call's code on target and writes
    ts, ws = fresh()
    ws[1].d_data = None
    ts[2].d_src, ts[2].n_bytes = sp + 1, len(stream) - 1
    assert L.knz_dev_write_streams(codec.h, ts, 3, ws, 3, None) == ERR_MISSING_PARAM
    assert [t.status for t in ts] == [0, ERR_MISSING_PARAM, ERR_INVALID_PARAM] and [w.status for w in ws] == [0, ERR_MISSING_PARAM, ERR_INVALID_PARAM]
    assert ts[0].out_bytes != 0 and ts[1].out_bytes == 0
    be.sync()
    assert be.to_host(kb, 3 * cap)[cap:] == bytes([FILL]) * (2 * cap)
    try:
        codec.dev_write_streams([(sp, len(stream), back, cap)], [(0, n + 5, 1, dp)], check=True)
        raise AssertionError("check=True did not raise")
    except K.KnzError as e:
        assert e.code == ERR_INVALID_PARAM
    codec.close()


# ---- 7. many targets --------------------------------------------------------------------------------------------------------------------------------
def many_targets(count, pipe=GRID_PIPE, bs=1024):
    lens = (bs, 2 * bs, bs - 24, bs + 500)
    out = []
    for k in range(count):
        n = lens[k % 4]
        data, stream = WR.source(pipe, bs, n)
        off = END if k % 2 else (k * 13) % (n - 7)
        out.append(Target(f"target {k}", data, stream, [(off, WR.payload(7, k))]))
    return out


def check_many(be, count, pipe=GRID_PIPE, bs=1024):
    targets = many_targets(count, pipe, bs)
    codec = M.codec_for(be, pipe, bs)
    res, rc, _d = streams_call(be, codec, targets)
    assert rc == 0
    for t, (got, status, st) in zip(targets, res):
        _e, ref = WR.expected_stream(pipe, bs, t.data, t.stream, t.writes)
        assert status == 0 and st == [0] and got == ref, (t.name, status, st)
    sample = [(count - 1) * i // 15 for i in range(16)]
    assert compare(be, codec, pipe, bs, [targets[i] for i in sample], [res[i] for i in sample]) == 16
    codec.close()


# ---- 8. workspace (emulator) --------------------------------------------------------------------------------------------------------------------------
def check_workspace(be, monkeypatch, pipe=RC.PIPELINES[2], bs=16400):
    n = RC.BLOCKS * bs + RC.TAIL
    data, stream = WR.source(pipe, bs, n)
    p = WR.payload
    targets = [Target("long", data, stream, [(3 * bs + 5, p(12 * bs, 1, text=True)), (END, p(2 * bs, 2))]),
               Target("short", data, stream, [(5 * bs + 5, p(100, 3))]),
               Target("two", data, stream, [(7 * bs - 5, p(10, 4))]),
               Target("tail", data, stream, [(END, p(bs, 5))])]
    wants = [WR.expected_stream(pipe, bs, t.data, t.stream, t.writes)[1] for t in targets]
    codec = M.codec_for(be, pipe, bs)
    seen = set()
    for limit in ("100000", "300000", "600000", None):
        if limit is None:
            monkeypatch.delenv("KNZ_TEST_ALLOC_LIMIT", raising=False)
        else:
            monkeypatch.setenv("KNZ_TEST_ALLOC_LIMIT", limit)
            try:
                codec.dev_decompress(*WR._whole(be, stream, n))             # (where it fits, another call's workspace is in place when the limit bites)
            except K.KnzError as e:
                assert e.code in (4, 5)
        res, rc, _d = streams_call(be, codec, targets)
        for t, want, (got, status, st) in zip(targets, wants, res):
            assert (status == 0 and got == want) or (status in (4, 5) and st == [status] * len(t.writes)), (limit, t.name, status, st)
            seen.add(status == 0)
    assert rc == 0 and all(s == 0 for _g, s, _st in res) and seen == {True, False}
    codec.close()


# ---- 10. large blocks, lanes (MI355X only) ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _large_source(pipe, seed, bs):
    n = 2 * bs + bs - 1000
    data = RC.G.make_input(pipe[0], n, seed)
    return data, M.ref_stream(pipe, bs, data, n)


def large_targets(pipe, other, bs=4 << 20):
    """two sources of this pipeline and one of another (it fails alone: the handle's configuration), three blocks each, the first one untouched"""
    writes = [(bs + 12345, WR.payload(100, 1)), (END, WR.payload(3000, 2, text=True))]
    return [Target(name, *_large_source(pp, seed, bs), writes) for name, pp, seed in (("first", pipe, 3), ("foreign", other, 3), ("second", pipe, 4))]


def check_large(be, targets, pipe, lanes=None, bs=4 << 20):
    codec = M.codec_for(be, pipe, bs, **({"devices": lanes} if lanes else {}))
    res, rc, _d = streams_call(be, codec, targets)
    assert rc == ERR_INVALID_PARAM and [s for _g, s, _st in res] == [0, ERR_INVALID_PARAM, 0] and res[1][2] == [ERR_INVALID_PARAM] * 2, (rc, [r[1:] for r in res])
    for t, (got, _s, _st) in zip(targets, res):
        if t.name != "foreign":
            _e, want = WR.expected_stream(pipe, bs, t.data, t.stream, t.writes)
            assert got == want, (t.name, M._diff(got, want))
    if not lanes:
        good = [t for t in targets if t.name != "foreign"]
        touched = sum(len(WR.touched_blocks(len(t.data), bs, t.writes)) for t in good)
        assert codec.last_counter(WR.COUNTER_DECODE_BLOCKS) == touched == 4
        assert codec.last_counter(WR.COUNTER_ENCODE_BLOCKS) == touched + sum(new_blocks(t, bs) for t in good)
    codec.close()
    return [g for g, _s, _st in res]
