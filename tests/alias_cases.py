"""PACK / DNA (the reference's AliasCodec, transform ids 18 and 19) cases shared by the emulator run and the MI355X run. The checker is
oracle/_ref (tests/ref_lib.py: the reference's own sources, translated and compiled); the hand-written oracle does not know these ids.
Every input comes from a seeded generator below; `row` names the line of the coverage guard the input is meant for."""
import base64

import numpy as np

import parity_cases as P
import ref_lib as R

K = P.K
PACK, DNA, LZ = 18, 19, 3
DT = {"UNDEFINED": 0, "TEXT": 1, "MULTIMEDIA": 2, "EXE": 3, "NUMERIC": 4, "BASE64": 5, "DNA": 6, "BIN": 7, "UTF8": 8, "SMALL_ALPHABET": 9}


def _pick(rng, values, n, p=None):
    return rng.choice(np.frombuffer(bytes(values), dtype=np.uint8), n, p=p).tobytes()


def _dna_lines(rng, n, letters=b"ACGT"):
    a = bytearray(_pick(rng, letters, n))
    for i in rng.integers(0, n, max(1, n // 500)):
        a[int(i)] = ord("N")
    for i in range(60, n, 61):
        a[i] = 10
    return bytes(a)


def _motif(rng, base=3000, reps=40, muts=15):
    m = np.frombuffer(_pick(rng, b"ACGT", base), dtype=np.uint8)
    out = []
    for _ in range(reps):
        c = m.copy()
        c[rng.integers(0, base, muts)] = np.frombuffer(_pick(rng, b"ACGT", muts), dtype=np.uint8)
        out.append(c.tobytes())
    return b"".join(out)


def _runs(rng, n):
    """long runs abababab... broken at random points by a third letter: alias runs of every length and parity"""
    alpha = bytes(range(ord("A"), ord("A") + 26)) + bytes(range(ord("c"), ord("c") + 14))
    out, total = [], 0
    while total < n:
        k = int(rng.integers(1, 40)) if rng.random() < 0.7 else int(rng.integers(40, 20000))
        piece = (b"ab" * (k // 2 + 1))[:k] + bytes([alpha[int(rng.integers(0, 40))]])
        out.append(piece)
        total += len(piece)
    return b"".join(out)[:n]


def inputs(big=True):
    """(name, row, data). big: the lengths of the GPU run; the emulator run takes the shorter ones."""
    rng = np.random.default_rng(0x414C4941)
    s = 1 if big else 4                                                    # emulator: a quarter of the length
    yield "one-value", "one", bytes([0x41]) * (100_003 // s)
    for k, n in ((2, 40_002), (3, 30_001), (4, 299_999)):
        yield "small-%d" % k, "small", _pick(rng, (0x01, 0x02, 0xF0, 0xFE)[:k], n // s)
    for k, n in ((2, 4_099), (3, 20_002), (4, 50_001)):
        yield "letters-%d" % k, "letters", _pick(rng, b"xyzw"[:k], n)
    yield "dna-ACGT", "dna", _pick(rng, b"ACGT", 200_003 // s)
    yield "dna-acgu", "dna", _pick(rng, b"acgu", 30_002)
    yield "dna-lines", "dna", _dna_lines(rng, 120_001 // s)
    yield "dna-motif", "dna", _motif(rng, 3000, 40 // s, 15)
    for k, n in ((5, 10_001), (15, 70_000), (16, 33_333)):
        yield "values-%d" % k, "nibble", _pick(rng, range(40, 40 + k), n)
    yield "values-17", "digram", _pick(rng, range(40, 57), 90_001 // s)
    w = np.array([2.0 ** -min(i, 12) for i in range(17)])
    yield "values-17-skewed", "digram", _pick(rng, range(40, 57), 65_536, p=w / w.sum())
    yield "corpus-even", "digram", P.corpus(150_000 // s)
    yield "corpus-odd", "digram", P.corpus(131_073 // s, 5)
    yield "utf-text", "digram", P.utf_text(60_001, 21)
    for name, data in P.text_inputs(50_000):
        if name in ("plain", "crlf", "markup", "capitals"):
            yield "text-" + name, "digram", data
    yield "cycle-20", "cycle", bytes(range(100, 120)) * (30_000 // 20 // s) + bytes(range(100, 107))
    yield "ab-runs", "runs", _runs(rng, 300_000 // s)
    yield "ab-runs-odd", "runs", _runs(rng, 70_001)
    yield "uniform-100", "savings", _pick(rng, range(20, 120), 100_000 // s)
    for k in (241, 250, 256):
        yield "uniform-%d" % k, "slots", _pick(rng, range(k), 60_000 // s)
    yield "numeric", "numeric", _pick(rng, b"0123456789+-*/=,.:; ", 40_001)
    yield "base64", "base64", base64.b64encode(rng.integers(0, 256, 45_000, dtype=np.uint8).tobytes())
    yield "len-1023", "floor", P.corpus(1023, 7)
    yield "len-1024", "floor", _pick(rng, b"ACGT", 1024)


def ref_forward(tid, data):
    """the reference's Forward of one object with a fresh ctx -> (bytes or None, ctx["dataType"] afterwards)"""
    R.set_ctx(1 << 16, R.entropy_type("NONE"), 0)
    out = R.transform_forward(tid, data)
    return out, R.data_type()


def path_of(out):
    """what the first bytes of a PACK output say: the mode, and the tail byte of the digram mode"""
    if out is None:
        return "declined", None
    n = out[0]
    if n == 255:
        return "one", None
    if n >= 252:
        return "2bit", None
    if n >= 240:
        return "4bit", None
    return "digram", out[1]


def check_objects(be, monkeypatch=None, big=True):
    """check 1: PACK and DNA objects against the reference's, both directions crossed"""
    c = K.Codec("NONE", "NONE", 1 << 20, lib=be.lib)
    scheds = ("fwd", "rev") if (monkeypatch is not None and be.name == "emu") else (None,)
    applied = {PACK: 0, DNA: 0}
    total = 0
    for name, _row, data in inputs(big):
        total += 1
        for tid in (PACK, DNA):
            r, _dt = ref_forward(tid, data)
            t = K.ByteTransform(c, tid)
            for sched in scheds:
                if sched:
                    monkeypatch.setenv("KNZ_EMU_SCHED", sched)
                g = t.forward(data)
                assert (g is None) == (r is None), (tid, name, sched, "one declines, the other does not")
                if r is None:
                    continue
                assert g == r, (tid, name, sched, "device forward != reference forward", len(g), len(r), [i for i in range(min(len(g), len(r))) if g[i] != r[i]][:4])
                assert t.inverse(r, len(data) + max(512, len(data) >> 4)) == data, (tid, name, sched, "reference-forward -> device-inverse")
                assert t.inverse(r, len(data)) == data, (tid, name, sched, "device-inverse into a buffer of exactly the block's size")
            if r is not None:
                applied[tid] += 1
                assert R.transform_inverse(tid, g, len(data) + 1024) == data, (tid, name, "device-forward -> reference-inverse")
    if monkeypatch is not None:
        monkeypatch.delenv("KNZ_EMU_SCHED", raising=False)
    R.set_ctx()
    c.close()
    assert total - applied[PACK] <= total // 3, ("PACK declined too often", applied, total)
    assert applied[DNA] >= 4, applied


def check_coverage():
    """check 5: with the reference alone, every row of the table takes the path it names"""
    seen = {}
    for name, row, data in inputs(True):
        out, dt = ref_forward(PACK, data)
        dout, ddt = ref_forward(DNA, data)
        seen.setdefault(row, []).append((name, path_of(out), dt, path_of(dout)[0], len(data)))
    R.set_ctx()

    def some(row, pred):
        assert any(pred(e) for e in seen[row]), (row, seen[row])

    some("one", lambda e: e[1][0] == "one")
    some("small", lambda e: e[1][0] == "2bit" and e[2] == DT["SMALL_ALPHABET"] and e[3] == "declined")
    some("letters", lambda e: e[1][0] == "2bit" and e[2] == DT["BASE64"] and e[3] == "declined")
    some("dna", lambda e: e[1][0] == "2bit" and e[2] == DT["DNA"] and e[3] == "2bit")
    some("dna", lambda e: e[1][0] == "4bit" and e[2] == DT["DNA"] and e[3] == "4bit")
    some("nibble", lambda e: e[1][0] == "4bit")
    some("digram", lambda e: e[1] == ("digram", 0))
    some("digram", lambda e: e[1] == ("digram", 1))
    some("cycle", lambda e: e[1][0] == "digram")
    some("runs", lambda e: e[1][0] == "digram")
    some("savings", lambda e: e[1][0] == "declined")
    some("slots", lambda e: e[1][0] == "declined")
    some("numeric", lambda e: e[2] == DT["NUMERIC"])
    some("base64", lambda e: e[2] == DT["BASE64"])
    some("floor", lambda e: e[1][0] == "declined" and e[4] == 1023)
    some("floor", lambda e: e[1][0] != "declined" and e[4] == 1024)
    # the n0 > n1 branch: the cycle has 20 values and 20 (+ 1: the first byte's pair with 0) pairs
    cyc = [d for n, r, d in inputs(True) if r == "cycle"][0]
    assert ref_forward(PACK, cyc)[0][0] == 21
    # lengths that are and are not multiples of 2 and 4, between 1024 and 300 000
    lens = [e[4] for es in seen.values() for e in es]
    assert any(l % 2 for l in lens) and any(l % 4 == 2 for l in lens) and any(l % 4 == 0 for l in lens) and max(lens) <= 300_000


def _stream_both_ways(be, codec, data, transform, entropy, bs, ck, what):
    src, ks = be.to_dev(data)
    cap = 2 * len(data) + (1 << 18) + 4096 * (len(data) // bs + 2)
    dst, kd = be.empty(cap)
    nb = codec.dev_compress(src, len(data), dst, cap)
    got = be.to_host(kd, nb)
    exp = R.compress(data, transform, entropy, bs, ck)
    assert got == exp, (transform, entropy, bs, what, "device stream != the reference Writer's stream", len(got), len(exp),
                        [i for i in range(min(len(got), len(exp))) if got[i] != exp[i]][:4])
    assert R.decompress(got, len(data) + 64) == data, (transform, entropy, bs, what, "device stream -> reference Reader")
    s2, k2 = be.to_dev(exp)
    out, ko = be.empty(len(data) + 64)
    assert codec.dev_decompress(s2, len(exp), out, len(data) + 64) == len(data)
    assert be.to_host(ko, len(data)) == data, (transform, entropy, bs, what, "reference stream -> device reader")
    return exp


STREAMS = (("PACK", "NONE", 0), ("DNA", "HUFFMAN", 32), ("DNA+LZ", "HUFFMAN", 0), ("PACK+LZ", "ANS0", 64), ("TEXT+UTF+PACK+LZX", "HUFFMAN", 0),
           ("PACK+BWT+RANK+ZRLT", "ANS1", 32))


def mixed_input(big=True):
    """the kinds side by side: neighbouring blocks take different paths"""
    parts = []
    for name, row, data in inputs(big):
        if row in ("one", "small", "dna", "nibble", "digram", "runs", "savings", "slots", "numeric"):
            parts.append(data[: 40_000 if big else 9_000])
    return b"".join(parts)


def magic_inputs():
    rng = np.random.default_rng(77)
    body = _pick(rng, b"ACGT", 30_000)
    for magic in (b"BM", b"\x1f\x8b", b"\x7fELF"):
        yield magic, magic + body[len(magic):]
    yield b"", body


def check_streams(be, big=True, block_sizes=(1024, 1 << 14, 1 << 16), streams=STREAMS, named_from=1 << 14):
    """check 2: sequences and streams against the reference's Writer and Reader, both directions crossed"""
    mixed = mixed_input(big)
    named = {n: d for n, _r, d in inputs(big)}
    for transform, entropy, ck in streams:
        for bs in block_sizes:
            codec = K.Codec(transform, entropy, bs, ck, lib=be.lib)
            _stream_both_ways(be, codec, mixed[: (60 if big else 12) * bs], transform, entropy, bs, ck, "mixed")
            if bs >= named_from:
                for name in ("dna-motif", "small-3", "letters-4", "ab-runs-odd", "corpus-odd", "text-plain"):
                    _stream_both_ways(be, codec, named[name][: 8 * bs], transform, entropy, bs, ck, name)
                for magic, data in magic_inputs():
                    _stream_both_ways(be, codec, data, transform, entropy, bs, ck, ("magic", magic))
            codec.close()


def check_dt_handover(be, big=True):
    """check 2, the blk_dt hand-over pinned on the blocks themselves: DNA text reaches LZ with min match 6 (dst[12] of the LZ output), small non-DNA
    alphabets make LZ decline, a magic number makes PACK / DNA decline and LZ run with min match 4; the skip-flag byte matches the reference's"""
    named = {n: d for n, _r, d in inputs(big)}
    bs = 1 << 17
    tt = K.transform_type("DNA+LZ")
    R.set_ctx(bs, R.entropy_type("NONE"), 0)
    c = K.Codec("DNA+LZ", "NONE", bs, lib=be.lib)
    bb = K.BlockBatch(c)
    cases = [("dna-motif", named["dna-motif"][:bs], 0x3F, 6), ("small-3", named["small-3"][:bs], 0xFF, None)]
    for magic, data in magic_inputs():
        cases.append((("magic", magic), data, 0xBF if magic else None, 4 if magic else None))
    res = [bb.encode([d])[0] for _n, d, _s, _m in cases]                 # (one call per block: only the last block of a batch may be short)
    for (name, data, skip, mm), (bits, written, mode, post, got_skip) in zip(cases, res):
        R.set_ctx(bs, R.entropy_type("NONE"), {b"BM": DT["MULTIMEDIA"], b"\x1f\x8b": DT["BIN"], b"\x7fELF": DT["EXE"]}.get(name[1], 0) if isinstance(name, tuple) else 0)
        ref_bytes, ref_skip = R.sequence_forward(tt, data)
        assert got_skip == ref_skip, (name, hex(got_skip), hex(ref_skip))
        assert post == len(ref_bytes), (name, post, len(ref_bytes))
        if skip is not None:
            assert ref_skip == skip, (name, hex(ref_skip), hex(skip))
        if mm is not None and not (ref_skip & 0x40):                      # LZ applied last: byte 12 of its output carries the min match it used
            assert ((ref_bytes[12] >> 1) & 7) + 2 == mm, (name, ref_bytes[12], mm)   # dst[12] = 0000MMMD (LZCodec.go:313-314)
    R.set_ctx()
    for (name, data, _s, _m), r in zip(cases, res):
        assert bb.decode([r[0]]) == [data], name
    c.close()


def check_batch_hooks(be, big=True):
    """check 3: knz_encode_blocks / knz_decode_blocks with the -l 2 sequence, then one handle with 3 lanes"""
    bs = 1 << 16
    mixed = mixed_input(big)
    blocks = [mixed[i: i + bs] for i in range(0, min(len(mixed), 14 * bs), bs)]
    blocks[-1] = blocks[-1][: max(1500, len(blocks[-1]) // 3)]
    for lanes in (None, 3):
        c = K.Codec("DNA+LZ", "HUFFMAN", bs, lib=be.lib, **({} if lanes is None else {"devices": [0] * lanes}))
        if lanes:
            assert c.L.knz_lane_count(c.h) == lanes
        bb = K.BlockBatch(c)
        res = bb.encode(blocks)
        assert bb.decode([r[0] for r in res]) == blocks
        # the stream the reference's Writer makes of the same blocks carries the same skip flags and block payloads: compare through a whole stream
        whole = b"".join(blocks)
        cs = K.Codec("DNA+LZ", "HUFFMAN", bs, lib=be.lib)
        exp = _stream_both_ways(be, cs, whole, "DNA+LZ", "HUFFMAN", bs, 0, "hook blocks as one stream")
        cs.close()
        tt = K.transform_type("DNA+LZ")
        for blk, (bits, written, mode, post, skip) in zip(blocks, res):
            magic = R.magic_type(blk)
            R.set_ctx(bs, R.entropy_type("HUFFMAN"), 0)
            ref_bytes, ref_skip = R.sequence_forward(tt, blk)
            assert (skip, post) == (ref_skip, len(ref_bytes)), (lanes, hex(skip), hex(ref_skip), post, len(ref_bytes), magic)
        R.set_ctx()
        c.close()


def _pack_none_stream(data, bs):
    return R.compress(data, "PACK", "NONE", bs)


def check_damaged(be, big=True, guard=False):
    """check 4: damaged PACK blocks. The transformed block is damaged as an object (the inverse transform object against the reference's:
    both fail or both give the same bytes) and inside a reference-written PACK&NONE stream (the call comes back; where the reference's
    Reader errors the device errors, where it succeeds the device gives the same bytes or rejects a block that passes the block size)."""
    rng = np.random.default_rng(4)
    named = {n: d for n, _r, d in inputs(big)}
    c = K.Codec("NONE", "NONE", 1 << 20, lib=be.lib)
    t = K.ByteTransform(c, PACK)
    for name in ("one-value", "small-3", "dna-lines", "values-16", "corpus-odd", "ab-runs-odd"):
        data = named[name][:20_000]
        good, _dt = ref_forward(PACK, data)
        assert good is not None, name
        cap = len(data)
        variants = [good[: len(good) - k] for k in (1, 2, 3, len(good) // 2, len(good) - 1, len(good) - 3)]
        variants += [bytes([v]) + good[1:] for v in range(16)]
        variants += [bytes([v]) + good[1:] for v in (16, 17, 100, 239, 240, 251, 252, 254, 255)]
        mode = path_of(good)[0]
        if mode in ("2bit", "4bit"):
            at = 1 + 256 - good[0]
            variants += [good[:at] + bytes([v]) + good[at + 1:] for v in (1, 2, 3, 4, 5, 128, 255)]
        if mode == "one":
            variants += [good[:2] + int(v).to_bytes(4, "little") for v in (cap + 1, cap * 2, 0xFFFFFFFF, 0, cap - 1)]
        if mode == "digram":
            variants += [good[:1] + bytes([v]) + good[2:] for v in (1, 2, 255)]
        for _ in range(12):
            b = bytearray(good)
            for i in rng.integers(0, len(b), int(rng.integers(1, 6))):
                b[int(i)] = int(rng.integers(0, 256))
            variants.append(bytes(b))
        for vi, bad in enumerate(variants):
            if len(bad) == 0:
                continue
            try:
                r = R.transform_inverse(PACK, bad, cap)
            except R.RefError:
                r = None
            try:
                g = t.inverse(bad, cap)
            except K.KnzError as e:
                assert e.code == 13, (name, vi, e.code)
                g = None
            if r is None:
                assert g is None, (name, vi, "the reference fails, the device does not")
            elif g is not None:
                assert g == r, (name, vi, "damaged block: device bytes != reference bytes")
            else:                                                          # the device may only reject what does not fit the buffer it was given
                assert len(r) >= cap - 1, (name, vi, "the device rejects what the reference decodes", len(r), cap)
    c.close()
    # inside streams: PACK&NONE streams of the reference, bytes of the transformed blocks flipped / the stream cut
    bs = 1 << 14
    cs = K.Codec("PACK", "NONE", bs, lib=be.lib)
    for name in ("one-value", "small-3", "dna-lines", "corpus-odd"):
        data = named[name][: 3 * bs + 777]
        good = _pack_none_stream(data, bs)
        trials = [good[: len(good) - k] for k in (5, 40, len(good) // 2)]
        for _ in range(10):
            b = bytearray(good)
            for i in rng.integers(14, len(b), int(rng.integers(1, 4))):
                b[int(i)] = int(rng.integers(0, 256))
            trials.append(bytes(b))
        for ti, bad in enumerate(trials):
            try:
                r = R.decompress(bad, len(data) + 64)
            except R.RefError:
                r = None
            sp, ks = be.to_dev(bad, 4)
            out, ko = be.empty(len(data) + 64 + 256)
            if guard:
                ko[1][len(data) + 64: len(data) + 64 + 256] = 0xA5
            try:
                nd = cs.dev_decompress(sp, len(bad), out, len(data) + 64)
                g = be.to_host(ko, nd)
            except K.KnzError:
                g = None
            if guard:
                assert bytes(ko[1][len(data) + 64: len(data) + 64 + 256]) == b"\xa5" * 256, (name, ti, "bytes behind the output buffer were written")
            if r is None:
                assert g is None, (name, ti, "the reference's Reader fails, the device does not")
            elif g is not None:
                assert g == r, (name, ti, "damaged stream: device bytes != reference bytes")
    cs.close()
