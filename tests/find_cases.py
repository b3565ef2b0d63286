"""knz_dev_find_many / knz_dev_find: where a byte string occurs in the decoded bytes of .knz streams. Cases shared by the emulator run
(tests/test_find_emu.py) and the MI355X run (tests/test_find_gpu.py). The streams are written by the reference's own Writer (oracle/_ref through
tests/ref_lib.py) from data built here, so the decoded bytes are known; the checker is oracle() below: bytes.find over the bytes the extended read
(offset, length + pattern_len - 1) delivers (read_cases.expected, the rule of include/knz_gpu.h), restarted at hit + 1.

Every case is a JOB: sources, queries and the oracle's expected (hits, scanned) for each, built without a device (the *_job functions are pure).
check_honesty() looks at the jobs alone: the boundary and dense cases expect at least 100 hits a query, every j of the boundary case is hit, the
small tile cuts every dense query into three tiles and more, and at most one query in ten of a module expects no hit. run_job() runs a job: every
d_hits array lies in one arena of a known 64-bit word with guard words on both sides; after the call everything but the words [0, min(n_hits, hits_cap))
of each query has to be that word still."""
import collections
import ctypes as C
import functools
import os

import numpy as np

import many_cases as M
import range_cases as RC
import read_cases as RD
import ref_lib as R

K = RC.K
ERR_MISSING_PARAM, ERR_INVALID_PARAM = RC.ERR_MISSING_PARAM, RC.ERR_INVALID_PARAM
PIPES = RC.PIPELINES[:4]                                                    # NONE&NONE, NONE&HUFFMAN/32, LZ&ANS0, BWT+RANK+ZRLT&ANS1/64
BLOCK_SIZES = (1024, 16384)
BLOCKS = {"gpu": {1024: 40, 16384: 20}, "emu": {1024: 10, 16384: 5}}        # the emulator runs a quarter of the lengths
TAIL = 777
LENS = (1, 2, 3, 4, 5, 8, 15, 16, 17, 64, 255, 256)
SMALL_TILE, DEFAULT_TILE = 256, 4096
GUARD_WORDS, FILL = 8, 0xA5
FILL_WORD = int.from_bytes(bytes([FILL]) * 8, "little")
FAR = 1 << 62                                                               # "a length past any stream" for the oracle's read

Q = collections.namedtuple("Q", "s pat off length cap hits scanned status")  # length None: KNZ_LENGTH_END ; cap None: NULL d_hits ; status: 0, a code, or "block"
Job = collections.namedtuple("Job", "case pipe bs sources queries tile")    # sources: [(data, stream, block boundaries)]


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------------------
def oracle(data, bounds, bs, off, length, pat):
    """-> (absolute offsets of the matches, scanned)"""
    pl = len(pat)
    ext = RD.expected(data, bounds, bs, off, (FAR if length is None else length) + pl - 1) if (length is None or length) else b""
    scanned = min(FAR if length is None else length, len(ext))
    hits, p = [], ext.find(pat)
    while p != -1 and p < scanned:
        hits.append(off + p)
        p = ext.find(pat, p + 1)
    return hits, scanned


def query(sources, bs, s, pat, off, length, cap="fit"):
    data, _stream, bounds = sources[s]
    hits, scanned = oracle(data, bounds, bs, off, length, pat)
    return Q(s, pat, off, length, len(hits) + 3 if cap == "fit" else cap, hits, scanned, 0)


def refused(s, pat, off, length, status, cap=4):
    return Q(s, pat, off, length, cap, [], 0, status)


# ---- data, streams ------------------------------------------------------------------------------------------------------------------------------------
def _filler(n, seed):
    return bytearray(np.random.default_rng(seed).integers(97, 123, n, dtype=np.uint8).tobytes())


def len_patterns():
    return [bytes(np.random.default_rng(100 + pl).integers(200, 256, pl, dtype=np.uint8)) for pl in LENS]


EDGE = b"\xc8EDGE\xc9\xca!"
HANG = EDGE + b"TAIL"
PERIOD = b"QRS"


@functools.lru_cache(maxsize=None)
def data_of(kind, bs, blocks):
    n = blocks * bs + TAIL
    buf = _filler(n, 7 + blocks)
    if kind == "lens":                                                      # every pattern of len_patterns() in slots of 300 bytes, taken in turn
        pats = len_patterns()
        for i in range(n // 300):
            pat, pos = pats[i % len(pats)], i * 300 + (i * 37) % 40
            if pos + len(pat) <= n:
                buf[pos: pos + len(pat)] = pat
    elif kind == "period":                                                  # runs of period 3 over every inner block boundary, the phase moving with the boundary
        for k in range(1, blocks + 1):
            for x in range(k * bs - 300, min(k * bs + 520, n)):
                buf[x] = PERIOD[(x + k) % 3]
    elif kind == "dense":                                                   # runs of a, of ab, a little filler between them ; no run length is a multiple of 64
        unit = b"a" * 777 + b"xyz" * 5 + b"ab" * 389 + b"q" + b"a" * 61 + b"b" + b"ab" * 33 + b"zz"
        buf = bytearray((unit * (n // len(unit) + 1))[:n])
    elif kind == "edge":
        for pos in edge_positions(bs):
            buf[pos: pos + len(EDGE)] = EDGE
        for pos in (bs // 2 + 1, 4 * bs - 6):
            buf[pos: pos + len(HANG)] = HANG
        buf[n - len(EDGE):] = EDGE                                          # a match that ends with the stream ; HANG hangs over the end here
    else:
        raise KeyError(kind)
    return bytes(buf)


def edge_positions(bs):
    return [bs - 3, 2 * bs + 5, 3 * bs + 517, 3 * bs + 900]


@functools.lru_cache(maxsize=None)
def stream_of(pipe, kind, bs, blocks):
    """(data, the reference Writer's stream, block boundaries)"""
    data = data_of(kind, bs, blocks)
    stream = RC._ref(pipe, bs, data)
    assert R.decompress(stream, len(data) + 64) == data
    return data, stream, RC._bounds(len(data), bs)


def _job(case, pipe, bs, sources, specs, tile=None):
    return Job(case, pipe, bs, sources, [sp if isinstance(sp, Q) else query(sources, bs, *sp) for sp in specs], tile)


# ---- the jobs (pure) ----------------------------------------------------------------------------------------------------------------------------------
def lengths_job(pipe, bs, scale):
    """1. every pattern length over the whole stream ; lengths 0 and 257 are refused (in one of the jobs: they are queries without a hit)"""
    refusals = pipe == PIPES[1] and bs == 1024
    src = [stream_of(pipe, "lens", bs, BLOCKS[scale][bs])]
    specs = [(0, pat, 0, None) for pat in len_patterns()]
    if refusals:
        specs += [refused(0, b"", 0, None, ERR_INVALID_PARAM), refused(0, b"x" * 257, 0, None, ERR_INVALID_PARAM)]
    return _job("lengths", pipe, bs, src, specs)


def boundary_job(pipe, bs, scale):
    """2. a 17-byte and a 256-byte pattern that start at k * bs - j for every j in 1 .. pattern_len - 1, over the boundaries k"""
    src = [stream_of(pipe, "period", bs, BLOCKS[scale][bs])]
    return _job("boundary", pipe, bs, src, [(0, (PERIOD * 86)[:pl], 0, None) for pl in (17, 256)])


def dense_job(pipe, bs, scale, tile):
    """3. hits at every position, overlapping ones: across every tile and wave edge"""
    src = [stream_of(pipe, "dense", bs, BLOCKS[scale][bs])]
    return _job("dense", pipe, bs, src, [(0, b"a", 5, None), (0, b"aaaa", 0, len(src[0][0]) - 9), (0, b"abab", 777, None)], tile)


def edges_job(pipe, bs, scale):
    """4. window edges"""
    src = [stream_of(pipe, "edge", bs, BLOCKS[scale][bs])]
    n = len(src[0][0])
    p = edge_positions(bs)
    specs = [(0, EDGE, p[1], p[2] - p[1] + 1),                              # matches that start at offset and at offset + length - 1 (that one ends behind the window)
             (0, EDGE, p[0] + 1, p[2] - p[0]),                              # a match starting at offset - 1 is none ; unaligned offset
             (0, EDGE, n - 100, None),                                      # a match ending exactly at the stream's end ; KNZ_LENGTH_END
             (0, HANG, 0, None),                                            # a pattern hanging over the end is none
             (0, EDGE, 3, 1 << 40),                                         # a window far past the end
             (0, EDGE, p[3] - 13, 14),                                      # the last start position of a short window
             (0, EDGE, n + 5, 10), (0, EDGE, 10, 0)]                        # an offset behind the end ; length == 0
    return _job("edges", pipe, bs, src, specs)


def caps_job(pipe, bs, scale):
    """5. hits_cap of 0 with NULL d_hits, 1, n_hits - 1, n_hits, n_hits + 5"""
    src = [stream_of(pipe, "lens", bs, BLOCKS[scale][bs])]
    pat = len_patterns()[LENS.index(5)]
    n = len(query(src, bs, 0, pat, 0, None).hits)
    assert n >= 2
    return _job("caps", pipe, bs, src, [(0, pat, 0, None, cap) for cap in (None, 1, n - 1, n, n + 5)])


def many_job(pipe, bs, scale):
    """6. three sources, twelve queries, several patterns over overlapping windows of one source"""
    blocks = BLOCKS[scale][bs]
    src = [stream_of(pipe, "lens", bs, blocks), stream_of(pipe, "edge", bs, blocks), stream_of(pipe, "dense", bs, blocks)]
    pats = len_patterns()
    n = len(src[0][0])
    specs = [(0, pats[3], 0, None), (0, pats[5], bs + 7, 3 * bs), (0, pats[8], 2 * bs - 40, 2 * bs + 100), (0, pats[10], 2 * bs + 1, 2 * bs),
             (0, pats[0], 0, 2 * bs), (0, pats[11], 0, 5 * bs), (1, EDGE, 0, None), (1, HANG, 100, 4 * bs), (1, EDGE, 2 * bs, 2 * bs),
             (2, b"ab", bs - 1, 700), (2, b"aaaa", 3 * bs + 9, bs), (0, pats[9], n - 5000, None)]
    return _job("many", pipe, bs, src, specs)


def distinct_pairs(job):
    """(source, block) pairs the queries' extended reads touch, blocks that do not exist left out"""
    pairs = set()
    for q in job.queries:
        nb = len(job.sources[q.s][2]) - 1
        if q.status != 0 or q.length == 0 or q.off >= nb * job.bs:
            continue
        last = nb - 1 if q.length is None else min((q.off + q.length + len(q.pat) - 2) // job.bs, nb - 1)
        pairs |= {(q.s, b) for b in range(q.off // job.bs, last + 1)}
    return pairs


DAMAGED = 5                                                                 # the block (ids from 1) whose payload gets a bit flipped


def damage_job(pipe, bs, scale):
    """7. queries whose extended window holds block 5 fail, the others complete ; source 1 is the undamaged stream"""
    case = stream_of(pipe, "lens", bs, BLOCKS[scale][bs])
    pats = len_patterns()
    lo, hi = (DAMAGED - 1) * bs, DAMAGED * bs
    specs = [(0, pats[3], 0, lo - 4), (0, pats[4], hi, None), (0, pats[11], hi + 10, None), (1, pats[4], lo - 100, bs + 200), (1, pats[9], 0, None),
             (0, pats[5], 100, lo - 108), (0, pats[8], hi + 3, None)]
    job = _job("damage", pipe, bs, [case, case], specs)
    hurt = [(0, pats[3], lo + 10, 100), (0, pats[9], 0, None), (0, pats[5], lo - 50, 60),
            (0, pats[11], lo - 400, 400)]                                   # ... the window ends in front of the block, the last start's 256 bytes reach into it
    assert all(q.hits for q in job.queries)
    return job._replace(queries=job.queries + [Q(s, pat, off, ln, 6, [], 0, "block") for s, pat, off, ln in hurt])


def short_parts(bs, scale):
    """two inputs: the first ends in a short block, a pattern lies across the joint, others on both sides of it"""
    blocks = max(BLOCKS[scale][bs] // 4, 2)
    a, b = _filler(blocks * bs + 333, 21), _filler(blocks * bs + 90, 22)
    a[-5:], b[:3] = EDGE[:5], EDGE[5:]                                      # in the decoded stream EDGE lies across the joint: in the addressing of the find call it does not
    for pos in (17, bs + 3, len(a) - 40):
        a[pos: pos + 8] = EDGE
    for pos in (60, bs - 4, len(b) - 8):
        b[pos: pos + 8] = EDGE
    return bytes(a), bytes(b)


def short_job(pipe, bs, scale):
    """8. a stream with a short inner block (the concatenation of two streams): a query across the joint stops at the short block's end"""
    a, b = short_parts(bs, scale)
    sa, sb = RC._ref(pipe, bs, a), RC._ref(pipe, bs, b)
    assert R.decompress(sa, len(a) + 64) == a and R.decompress(sb, len(b) + 64) == b
    ba, bb = RC._bounds(len(a), bs), RC._bounds(len(b), bs)
    bounds = ba + [len(a) + x for x in bb[1:]]
    na = len(ba) - 1                                                        # blocks of a: b's first block is addressed at na * bs
    src = [(a + b, (sa, sb), bounds)]
    specs = [(0, EDGE, len(a) - 100, 2 * bs), (0, EDGE, 0, None), (0, EDGE, na * bs, None), (0, EDGE, na * bs + 50, bs), (0, EDGE, len(a) - 6, 50)]
    job = _job("short", pipe, bs, src, specs)
    q = job.queries
    assert q[0].scanned == 100 and q[0].hits == [len(a) - 40] and q[1].scanned == len(a) and len(q[1].hits) == 3        # ... it stops there, no match reaches over it
    assert q[2].hits == [na * bs + p for p in (60, bs - 4, len(b) - 8)] and q[4].hits == [] and q[4].scanned == 6
    return job


def all_jobs(scale):
    """every job a module of this scale runs (the damage, short and contract jobs included)"""
    out = []
    for bs in BLOCK_SIZES:
        for i, pipe in enumerate(PIPES):
            out += [lengths_job(pipe, bs, scale), boundary_job(pipe, bs, scale), dense_job(pipe, bs, scale, SMALL_TILE)]
        out += [dense_job(PIPES[1], bs, scale, None)] if bs == 16384 else []
        out += [edges_job(PIPES[1], bs, scale), edges_job(PIPES[2], bs, scale), caps_job(PIPES[3], bs, scale),
                many_job(PIPES[1], bs, scale), short_job(PIPES[1], bs, scale), short_job(PIPES[3], bs, scale)]
    out += [damage_job(PIPES[1], 1024, scale), contract_job(scale)]
    return out


def check_honesty(scale):
    jobs = all_jobs(scale)
    for job in jobs:
        for q in job.queries:
            if job.case in ("boundary", "dense"):
                assert len(q.hits) >= 100, (job.case, job.bs, len(q.pat), len(q.hits))
            if job.case == "boundary":
                pl = len(q.pat)
                starts = set(q.hits)
                nb = len(job.sources[0][2]) - 1
                for j in range(1, pl):
                    assert any(k * job.bs - j in starts for k in range(1, nb)), (job.bs, pl, j, "no match starts j bytes in front of a boundary")
                assert len(starts) == len(q.hits)
            if job.case == "dense":
                tile = job.tile or DEFAULT_TILE
                assert q.scanned >= 3 * tile and (job.tile is None or job.bs % tile == 0 and job.bs > tile), (job.bs, tile, q.scanned)
                assert any(b - a == 1 for a, b in zip(q.hits, q.hits[1:])) or len(q.pat) == 4 and q.pat == b"abab"       # hits at neighbouring positions
                assert any((a - q.off) // tile != (b - q.off) // tile and b - a <= max(len(q.pat) - 1, 1) for a, b in zip(q.hits, q.hits[1:])), \
                    "no overlapping (for one byte: neighbouring) matches across a tile edge"
    assert any(job.case == "dense" and job.tile is None and len(job.sources[0][0]) >= 3 * DEFAULT_TILE for job in jobs)
    qs = [q for job in jobs for q in job.queries]
    empty = [q for q in qs if not q.hits]
    assert 10 * len(empty) <= len(qs), (len(empty), len(qs), "more than one query in ten expects no hit")
    for case in ("lengths", "boundary", "dense", "edges", "caps", "many", "damage", "short", "contract"):
        assert any(job.case == case for job in jobs), case
    lens = {len(q.pat) for job in jobs if job.case == "lengths" for q in job.queries}
    assert lens == set(LENS) | {0, 257}
    e = [job for job in jobs if job.case == "edges"][0]
    p, n = edge_positions(e.bs), len(e.sources[0][0])
    h = [q.hits for q in e.queries]
    assert h[0][0] == p[1] and h[0][-1] == p[2] and p[0] not in h[1] and h[1][-1] == p[2] and h[2] == [n - 8]
    assert h[3] and n - 8 not in h[3] and h[4][0] == e.bs // 2 + 1 and h[4][-1] == n - 8 and h[5] == [p[3]] and h[6] == h[7] == [] and e.queries[6].scanned == e.queries[7].scanned == 0
    assert any(q.off % 16 for q in e.queries)
    return len(qs), len(empty)


# ---- device calls -------------------------------------------------------------------------------------------------------------------------------------
def _view(be, keep):
    return keep[1] if be.name == "emu" else keep


def to_dev(be, case):
    """a job's source on the device -> (pointer, bytes, what keeps it alive)"""
    stream = case[1]
    sp, keep = be.to_dev(stream, 4)
    return sp, len(stream), keep


def concat_dev(be, codec, streams):
    """a source of several streams: their knz_dev_concat, made on the device (a part that ends in a short block leaves a short inner block)"""
    keep = [be.to_dev(s, 4) for s in streams]
    cap = sum(len(s) for s in streams) + 64
    dst, kd = be.empty(cap)
    nb = codec.dev_concat([k[0] for k in keep], [len(s) for s in streams], dst, cap, check=True)
    be.sync()
    return dst, nb, (keep, kd)


def find_call(be, codec, src, queries, tile=None):
    """src: [(device pointer, bytes[, index rows])] ; queries: [Q]. -> ([(n_hits, scanned, status, [offsets])], return code). Asserts that nothing but the
    words [0, min(n_hits, hits_cap)) of every query has changed."""
    at, cur = [], GUARD_WORDS
    for q in queries:
        at.append(cur)
        cur += (q.cap or 0) + GUARD_WORDS
    size = 8 * cur
    ptr, keep = be.empty(size)
    assert ptr % 16 == 0
    _view(be, keep)[:size] = FILL
    finds = [(q.s, q.pat, q.off, q.length, None if q.cap is None else ptr + 8 * a, q.cap or 0) for q, a in zip(queries, at)]
    if tile:
        os.environ["KNZ_FIND_TILE"] = str(tile)
    try:
        res = codec.dev_find_many(src, finds)
    finally:
        os.environ.pop("KNZ_FIND_TILE", None)
    be.sync()
    words = np.frombuffer(be.to_host(keep, size), dtype="<u8").copy()
    out = []
    for (n, scanned, status), q, a in zip(res, queries, at):
        w = min(n, q.cap or 0)
        out.append((n, scanned, status, [int(x) for x in words[a: a + w]]))
        words[a: a + w] = FILL_WORD
    bad = [int(i) for i in np.flatnonzero(words != FILL_WORD)[:4]]
    assert not bad, ("words outside [0, min(n_hits, hits_cap)) of the queries were written", bad, at[:4])
    return out, codec.last_many_rc


def want_of(q, code=None):
    status = code if q.status == "block" else q.status
    return (len(q.hits), q.scanned, status, q.hits[: q.cap or 0])


def run_job(be, job, codec=None):
    """the job on the device: every query's count, scanned and offsets are the oracle's"""
    own = codec is None
    codec = codec or M.codec_for(be, job.pipe, job.bs)
    keep, src = [], []
    for case in job.sources:
        d = concat_dev(be, codec, case[1]) if isinstance(case[1], tuple) else to_dev(be, case)
        keep.append(d)
        src.append((d[0], d[1]))
    got, rc = find_call(be, codec, src, job.queries, job.tile)
    for q, g in zip(job.queries, got):
        assert g == want_of(q), (job.case, job.pipe, job.bs, job.tile, len(q.pat), q.off, q.length, q.cap, g[:3], len(q.hits), q.scanned, M._diff(g[3], q.hits))
    assert rc == next((q.status for q in job.queries if q.status), 0)
    if own:
        codec.close()
    return got, src, keep


# ---- 5. hits_cap, 6. many ---------------------------------------------------------------------------------------------------------------------------------
def check_many(be, pipe, bs, scale):
    job = many_job(pipe, bs, scale)
    assert len(job.sources) == 3 and len(job.queries) == 12
    codec = M.codec_for(be, pipe, bs)
    got, src, _keep = run_job(be, job, codec)
    pairs = distinct_pairs(job)
    assert codec.last_counter(7) == len(pairs) and len(pairs) < sum(len(distinct_pairs(job._replace(queries=[q]))) for q in job.queries), codec.last_counter(7)
    for q, g in zip(job.queries, got):                                      # each query issued alone: identical
        alone, rc = find_call(be, codec, [src[q.s]], [q._replace(s=0)])
        assert rc == 0 and alone == [g], (q.s, q.off, q.length)
        assert codec.last_counter(7) == len(distinct_pairs(job._replace(queries=[q])))
    back, rc = find_call(be, codec, src, job.queries[::-1])
    assert rc == 0 and back[::-1] == got, "the reversed query list gives other results"
    hinted = []
    for i, (sp, nbytes) in enumerate(src):                                  # index hints: all rows, the first three, none
        _info, pos = codec.dev_stream_index(sp, nbytes)
        hinted.append((sp, nbytes, (pos, pos[:3], None)[i]))
    again, rc = find_call(be, codec, hinted, job.queries)
    assert rc == 0 and again == got and codec.last_counter(7) == len(pairs)
    single = job.queries[0]                                                 # the single form: one source, its whole stream
    ptr, kd = be.empty(8 * (len(single.hits) + 4))
    n = codec.dev_find(src[0][0], src[0][1], single.pat, ptr, len(single.hits) + 4)
    be.sync()
    assert n == len(single.hits) and [int(x) for x in np.frombuffer(be.to_host(kd, 8 * n), dtype="<u8")] == single.hits
    assert codec.dev_find(src[0][0], src[0][1], single.pat) == n
    codec.close()


# ---- 7. damage ------------------------------------------------------------------------------------------------------------------------------------------
def check_damage(be, scale, pipe=PIPES[1], bs=1024):
    assert pipe[2] == 32
    job = damage_job(pipe, bs, scale)
    data, stream, _bounds = job.sources[0]
    _info, fr, _end = RC.frames(stream)
    hurt = bytearray(stream)
    hurt[(fr[DAMAGED - 1][1] + fr[DAMAGED - 1][2] // 2) // 8] ^= 0x10       # the middle of the block's payload
    codec = M.codec_for(be, pipe, bs)
    hp, _kh = be.to_dev(bytes(hurt), 4)
    sp, _ks = be.to_dev(stream, 4)
    _g, code = RC.range_call(be, codec, hp, len(hurt), bs, (DAMAGED, DAMAGED + 1))
    assert code != 0
    src = [(hp, len(hurt)), (sp, len(stream))]
    for qs in (job.queries, job.queries[4:] + job.queries[:4]):
        got, rc = find_call(be, codec, src, qs)
        assert got == [want_of(q, code) for q in qs], [(g[:3], want_of(q, code)[:3]) for g, q in zip(got, qs)]
        assert rc == code
    # a source with a bad header, a NULL and a misaligned pointer: their own queries fail, the others complete
    tp, _kt = be.to_dev(stream[:10], 4)
    src = [(sp, len(stream)), (tp, 10), (None, len(stream)), (sp + 1, len(stream) - 1)]
    good = [q._replace(s=0) for q in job.queries if q.status == 0][:6]
    qs = good[:2] + [good[2]._replace(s=1), good[3]._replace(s=2), good[4]._replace(s=3)] + good[5:]
    got, rc = find_call(be, codec, src, qs)
    short = codec.last_source_status[1]
    assert short != 0 and codec.last_source_status == [0, short, ERR_MISSING_PARAM, ERR_INVALID_PARAM]
    want = [want_of(q) for q in qs]
    for i, st in ((2, short), (3, ERR_MISSING_PARAM), (4, ERR_INVALID_PARAM)):
        want[i] = (0, 0, st, [])
    assert got == want and rc == short, [g[:3] for g in got]
    codec.close()


# ---- arguments -------------------------------------------------------------------------------------------------------------------------------------------
def contract_job(scale, pipe=PIPES[1], bs=1024):
    src = [stream_of(pipe, "lens", bs, BLOCKS[scale][bs])]
    pats = len_patterns()
    specs = [(0, pats[4], 5, 3 * bs), refused(1, pats[4], 0, 10, ERR_INVALID_PARAM), refused(0, pats[4], 2 ** 64 - 5, 10, ERR_INVALID_PARAM),
             (0, pats[6], bs - 1, None), (0, pats[7], 2 ** 64 - 11, 10), (0, pats[2], 0, 2 ** 64 - 1)]
    return _job("contract", pipe, bs, src, specs)


def check_contract(be, scale):
    job = contract_job(scale)
    pipe, bs = job.pipe, job.bs
    codec = M.codec_for(be, pipe, bs)
    got, src, _keep = run_job(be, job, codec)
    assert got[4][:3] == (0, 0, 0)                                          # an offset far behind the end whose window does not overflow: nothing, no error
    L = codec.L
    Source, Find = K.api._Source, K.api._Find
    sp, nbytes = src[0]
    pat = C.create_string_buffer(job.queries[0].pat, 5)
    hits, _kh = be.empty(64)
    s, f = (Source * 1)(), (Find * 1)()
    s[0].d_src, s[0].n = sp, nbytes

    def one(**kw):
        f[0].source, f[0].pattern_len, f[0].pattern, f[0].offset, f[0].length, f[0].d_hits, f[0].hits_cap = 0, 5, C.addressof(pat), 5, 3 * bs, hits, 4
        for k, v in kw.items():
            setattr(f[0], k, v)
        return L.knz_dev_find_many(codec.h, s, 1, f, 1, None), f[0].status, f[0].n_hits

    want = len(job.queries[0].hits)
    assert one() == (0, 0, want) and want > 0
    assert one(d_hits=hits + 4) == (ERR_INVALID_PARAM, ERR_INVALID_PARAM, 0)
    assert one(pattern=None) == (ERR_MISSING_PARAM, ERR_MISSING_PARAM, 0)
    assert one(d_hits=None) == (ERR_MISSING_PARAM, ERR_MISSING_PARAM, 0)
    assert one(d_hits=None, hits_cap=0) == (0, 0, want)
    assert L.knz_dev_find_many(None, s, 1, f, 1, None) == ERR_MISSING_PARAM
    assert L.knz_dev_find_many(codec.h, s, 1, f, 0, None) == 0 and L.knz_dev_find_many(codec.h, None, 0, None, -1, None) == 0
    assert L.knz_dev_find_many(codec.h, None, 1, f, 1, None) == ERR_MISSING_PARAM and L.knz_dev_find_many(codec.h, s, 1, None, 1, None) == ERR_MISSING_PARAM
    out = C.c_uint64()
    assert L.knz_dev_find(codec.h, sp, nbytes, C.addressof(pat), 5, hits, 4, None, None) == ERR_MISSING_PARAM
    assert L.knz_dev_find(codec.h, None, nbytes, C.addressof(pat), 5, hits, 4, C.byref(out), None) == ERR_MISSING_PARAM
    assert L.knz_dev_find(codec.h, sp + 1, nbytes - 1, C.addressof(pat), 5, hits, 4, C.byref(out), None) == ERR_INVALID_PARAM
    assert L.knz_dev_find(codec.h, sp, nbytes, C.addressof(pat), 0, hits, 4, C.byref(out), None) == ERR_INVALID_PARAM
    assert codec.dev_find_many([], []) == [] and codec.last_many_rc == 0
    try:
        codec.dev_find_many(src, [(0, b"", 0, None, None, 0)], check=True)
        raise AssertionError("check=True did not raise")
    except K.KnzError as e:
        assert e.code == ERR_INVALID_PARAM
    # an empty stream (header + end marker): no block, no entry, no hit
    _d0, empty, _b0 = RC.sized_stream(pipe, bs, 0)
    ep, _ke = be.to_dev(empty, 4)
    assert codec.dev_find_many([(ep, len(empty))], [(0, b"ab", 0, None, None, 0), (0, b"ab", 5, 100, None, 0)]) == [(0, 0, 0)] * 2 and codec.last_counter(7) == 0
    dst, kd = be.empty(len(job.sources[0][0]) + 64)                        # the handle still works
    assert codec.dev_decompress(sp, nbytes, dst, len(job.sources[0][0]) + 64) == len(job.sources[0][0])
    be.sync()
    assert be.to_host(kd, len(job.sources[0][0])) == job.sources[0][0]
    codec.close()


# ---- no phantom entries ------------------------------------------------------------------------------------------------------------------------------------
def check_no_phantom(be, scale, pipe=PIPES[1], bs=1024):
    """a whole block multiple (no ragged last block) and windows far past the end: the batch holds the stream's blocks and no more ; framing damaged in
    front of a block fails the queries that reach it with the walk's code, the others complete"""
    blocks = BLOCKS[scale][bs] // 2
    data = data_of("lens", bs, BLOCKS[scale][bs])[: blocks * bs]
    stream = RC._ref(pipe, bs, data)
    assert R.decompress(stream, len(data) + 64) == data
    case = (data, stream, RC._bounds(len(data), bs))
    pats = len_patterns()
    last = next(p for p in pats[2:] if oracle(data, case[2], bs, (blocks - 1) * bs + 7, None, p)[0])
    job = _job("phantom", pipe, bs, [case], [(0, pats[3], 0, None), (0, last, (blocks - 1) * bs + 7, 1 << 50), (0, pats[8], 3, 1 << 62)])
    codec = M.codec_for(be, pipe, bs)
    _got, src, _keep = run_job(be, job, codec)
    assert codec.last_counter(7) == blocks and all(q.scanned == len(data) - q.off for q in job.queries)
    _info, fr, _end = RC.frames(stream)
    cut = bytearray(stream)
    cut[(fr[2][0] + 5) // 8] ^= 0x80 >> ((fr[2][0] + 5) % 8)                # block 3's length field: the walk lands inside its payload
    cp, _kc = be.to_dev(bytes(cut), 4)
    _g, walk = RC.range_call(be, codec, cp, len(cut), bs, (4, 5))
    assert walk != 0
    qs = [query([case], bs, 0, pats[3], 0, 2 * bs - 300), Q(0, pats[3], 0, None, 4, [], 0, walk), Q(0, pats[5], 5 * bs, bs, 4, [], 0, walk)]
    got, rc = find_call(be, codec, [(cp, len(cut))], qs)
    assert got[0] == want_of(qs[0]) and got[0][0] > 0 and [g[2] != 0 for g in got] == [False, True, True] and got[2][2] == walk and rc == got[1][2], got
    _i, pos = codec.dev_stream_index(src[0][0], src[0][1])                  # with the index of the undamaged stream they complete
    got, rc = find_call(be, codec, [(cp, len(cut), pos)], [qs[0], query([case], bs, 0, pats[5], 5 * bs, bs)])
    assert rc == 0 and got[1][0] == len(oracle(data, case[2], bs, 5 * bs, bs, pats[5])[0])
    codec.close()


# ---- 9. symbols -----------------------------------------------------------------------------------------------------------------------------------------
def check_symbols(be):
    lib = C.CDLL(be.lib)
    for name in ("knz_dev_find_many", "knz_dev_find"):
        assert hasattr(lib, name), name
    assert C.sizeof(K.api._Find) == 72 and K.api.LENGTH_END == 2 ** 64 - 1 and K.api.FIND_MAX_PATTERN == 256
