"""Block sizes that are multiples of 16 only, pointers at the minimum alignment include/knz_gpu.h asks for, and destinations of the smallest
capacity it allows. Cases shared by the emulator run (tests/test_geometry_emu.py) and the MI355X run (tests/test_geometry_gpu.py).
Every comparison is bit for bit. The checker is the hand-written oracle (oracle_lib); the stream cases are also compared with the
reference's own Writer (oracle/_ref through tests/ref_lib.py) where it is built. PACK / DNA are known to oracle/_ref only.

Everywhere else in tests/ a block size is a power of two and every device pointer is 256-byte aligned: block b starts at a multiple of
1024 bytes, every block is a whole number of entropy chunks and transform segments, and a ragged chunk is the last thing in a stream.
Here every block ends in a 16-byte chunk, block starts are 16-byte aligned only, and check_coverage() keeps the tables that way."""
import ctypes as C
import functools

import numpy as np

import alias_cases as A
import many_cases as M
import parity_cases as P
import ref_lib as R
import text_corpus

K, O = P.K, P.O
FILL = 0xA5
ERR_WRITE_FILE = 12

# chunk sizes of the entropy codecs (KNZ_ANS1_CHUNK, KNZ_FPAQ_CHUNK; Huffman / ANS0: 16 KiB)
CHUNK = {"HUFFMAN": 1 << 14, "ANS0": 1 << 14, "ANS1": 4 << 20, "FPAQ": 4 << 20}
# 1040: the smallest step above the minimum ; 5008: no multiple of 64 ; 16 400: a 16 KiB chunk and two 8 KiB transform segments plus 16 bytes in
# EVERY block ; 49 136: three chunks, the last 16 bytes short ; 65 552: just above the inverse BWT's list-ranking threshold
BLOCK_SIZES = (1040, 5008, 16400, 49136, 65552)
BIG_BLOCK = (4 << 20) + 16                                                  # a 16-byte second ANS1 / FPAQ chunk in every block
TAIL, BIG_TAIL = 777, 12345                                                 # ragged last blocks, no multiple of 16

NONE_PIPES = (("NONE", "HUFFMAN"), ("NONE", "ANS0"), ("NONE", "ANS1"), ("NONE", "FPAQ"), ("NONE", "NONE"))
XF_PIPES = (("BWT+RANK+ZRLT", "ANS1"), ("BWT+RANK+ZRLT", "ANS0"), ("BWT+MTFT+ZRLT", "FPAQ"), ("LZ", "ANS0"), ("LZX", "NONE"), ("LZP+SRT", "HUFFMAN"),
            ("TEXT+UTF+BWT+RANK+ZRLT", "ANS0"), ("DNA+LZ", "HUFFMAN"), ("PACK", "ANS0"))


def stream_cases(gpu, block_sizes=BLOCK_SIZES, big=BIG_BLOCK):
    """[(transform, entropy, block size, n, seed)] of check_stream_geometry. The MI355X runs every pipeline at every block size with four blocks
    and a tail, and the 4 MiB + 16 size for NONE / ANS1 and NONE / FPAQ. The emulator runs every pipeline at the first size, the NONE pipelines
    at all of them, and the transform pipelines at the second and third size with two blocks and a tail."""
    cases = []
    for i, bs in enumerate(block_sizes):
        for t, e in NONE_PIPES:
            cases.append((t, e, bs, 4 * bs + TAIL, 3))
        for t, e in XF_PIPES:
            if gpu or i == 0:
                cases.append((t, e, bs, 4 * bs + TAIL, 3))
            elif i in (1, 2):
                cases.append((t, e, bs, 2 * bs + TAIL, 3))
    if gpu:
        cases += [("NONE", "ANS1", big, 2 * big + BIG_TAIL, 3), ("NONE", "FPAQ", big, 2 * big + BIG_TAIL, 3)]
    return cases


def case_id(case):
    return "-".join(str(x) for x in case[:3])


# (compress source, compress destination, stream handed to the decoder, decode destination): bytes past a 256-byte boundary
PLACEMENTS = ((16, 4, 4, 1), (48, 12, 8, 2), (240, 252, 12, 3), (0, 8, 4, 15), (16, 4, 12, 7))

# (transform, entropy, a power-of-two block size, n, a block size of the table, n)
ALIGN_CASES = (("NONE", "HUFFMAN", 1 << 14, 49999, 16400, 40001), ("NONE", "ANS0", 1 << 14, 49999, 16400, 40001), ("NONE", "ANS1", 4096, 20001, 5008, 30003),
               ("NONE", "FPAQ", 4096, 20001, 1040, 10007), ("NONE", "NONE", 1 << 14, 49999, 16400, 40001), ("BWT+RANK+ZRLT", "ANS1", 4096, 9001, 5008, 12001),
               ("LZ", "ANS0", 4096, 9001, 5008, 12001), ("TEXT+UTF+BWT+RANK+ZRLT", "ANS0", 4096, 9001, 5008, 12001), ("LZP+SRT", "HUFFMAN", 4096, 9001, 1040, 3001),
               ("BWT+MTFT+ZRLT", "ANS0", 1024, 3001, 5008, 7001), ("LZX", "NONE", 4096, 9001, 16400, 40001))

# (transform, entropy, block size, n): n odd
TIGHT_CASES = (("NONE", "HUFFMAN", 16400, 3 * 16400 + 777), ("NONE", "NONE", 1040, 5 * 1040 + 33), ("BWT+RANK+ZRLT", "ANS1", 5008, 2 * 5008 + 1001),
               ("LZ", "ANS0", 1 << 14, 40001))


# ---- inputs and expected streams, computed once -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_input(transform, n, seed):
    names = transform.split("+")
    if "DNA" in names:
        return A._dna_lines(np.random.default_rng(seed), n)
    if "PACK" in names:                                                     # 15 values: the 4-bit form
        return A._pick(np.random.default_rng(seed), range(40, 55), n)
    if "TEXT" in names:
        return text_corpus.make_text(n, seed=seed, utf8=0.02)
    if "UTF" in names:
        return P.utf_text(n, seed)
    return P.corpus(n, seed)


def _ref_only(transform):
    return bool({"PACK", "DNA"} & set(transform.split("+")))


@functools.lru_cache(maxsize=None)
def expected(transform, entropy, bs, n, seed):
    """the stream the oracle writes for make_input(transform, n, seed); compared with the reference Writer's where oracle/_ref is built"""
    data = make_input(transform, n, seed)
    if _ref_only(transform):
        return R.compress(data, transform, entropy, bs)
    exp = O.compress(data, transform, entropy, bs)
    if R.available():
        ref = R.compress(data, transform, entropy, bs)
        assert exp == ref, (transform, entropy, bs, n, "the oracle's stream != the reference Writer's", M._diff(exp, ref))
    return exp


# ---- 1. placement --------------------------------------------------------------------------------------------------------------------------
def place(be, data_or_n, offset, guard=64):
    """-> (ptr, keep, n): n bytes that start `offset` bytes past a 256-byte boundary, inside one allocation filled with 0xA5 (the n bytes
    too, unless data is given: a destination starts out stale, not cleared). At least `guard` bytes lie on either side."""
    data = None if isinstance(data_or_n, (int, np.integer)) else data_or_n
    n = int(data_or_n) if data is None else len(data)
    assert 0 <= offset < 256
    total = 256 + offset + n + 2 * guard + 16
    if be.name == "gpu":
        buf = be.torch.full((total,), FILL, dtype=be.torch.uint8, device=be.dev)
        base = buf.data_ptr()
    else:
        buf = np.full(total, FILL, dtype=np.uint8)
        base = buf.ctypes.data
    start = (-base) % 256 + offset
    if start < guard:
        start += 256
    assert start + n + guard <= total
    if data is not None and n:
        a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        if be.name == "gpu":
            buf[start:start + n] = be.torch.from_numpy(np.ascontiguousarray(a)).to(be.dev)
        else:
            buf[start:start + n] = a
    ptr = base + start
    assert ptr % 256 == offset, (ptr % 256, offset)                         # (a wrong slice must not test the aligned case again)
    return ptr, (buf, start), n


def _host(be, keep):
    buf, start = keep
    if be.name == "gpu":
        be.sync()
        return buf.cpu().numpy(), start
    return buf, start


def fetch(be, keep, n):
    a, start = _host(be, keep)
    return a[start:start + n].tobytes()


def guards_intact(be, keep, n, slack=0):
    """every byte before the placed range and every byte from its byte n + slack on is as place() left it"""
    a, start = _host(be, keep)
    assert bool((a[:start] == FILL).all()), ("bytes in front of the pointer were written", np.nonzero(a[:start] != FILL)[0][:4] - start)
    assert bool((a[start + n + slack:] == FILL).all()), ("bytes behind the capacity were written", n, np.nonzero(a[start + n + slack:] != FILL)[0][:4] + n + slack)


def place_stream(be, stream, offset):
    """a stream for the decoder: readable to the next multiple of 4, as the header asks"""
    return place(be, stream + bytes(-len(stream) % 4), offset)[:2]


# ---- 2. whole streams at block sizes that are multiples of 16 only ---------------------------------------------------------------------------
def check_stream_geometry(be, transform, entropy, bs, n, seed=3):
    assert bs % 16 == 0 and n >= 2 * bs and (n % bs) % 16
    data = make_input(transform, n, seed)
    exp = expected(transform, entropy, bs, n, seed)
    tag = (transform, entropy, bs, n)
    c = K.Codec(transform, entropy, bs, lib=be.lib)
    src, ksrc = be.to_dev(data)
    cap = 2 * n + 262144 * (n // bs + 2)
    dst, kdst = be.empty(cap)
    nb = c.dev_compress(src, n, dst, cap)
    got = be.to_host(kdst, nb)
    assert got == exp, (tag, "device stream != oracle stream", M._diff(got, exp))
    sp, ks = be.to_dev(exp, 4)
    out, kout = be.empty(n + 64)
    nd = c.dev_decompress(sp, len(exp), out, n + 64)
    assert nd == n, (tag, nd)
    back = be.to_host(kout, nd)
    assert back == data, (tag, "oracle stream -> device decoder", M._diff(back, data))
    if entropy == "HUFFMAN":                                                # an encoder-written stream never needs the serial Huffman decoder
        assert c.last_counter(0) == 0, tag
    if (transform, entropy) == ("BWT+RANK+ZRLT", "ANS1"):                   # the two inverses ran as one chain under the rANS decoder
        assert c.last_counter(6) >= 1, (tag, "no block took the fused chain")
    c.close()


# ---- 3. the other entry points ------------------------------------------------------------------------------------------------------------
def check_short_inner_block(be, bs=16400):
    """parity_cases.check_short_inner_block with blocks of 16 400 bytes: the gaps are closed between block starts that are 16-byte aligned only"""
    for transform, entropy in (("NONE", "HUFFMAN"), ("BWT+RANK+ZRLT", "ANS0")):
        a, b = P.corpus(bs + 4321, 7), P.corpus(2 * bs + 99, 8)
        c = K.Codec(transform, entropy, bs, lib=be.lib)
        segs, bits, keep = [], [], []
        for part in (a, b):
            src, ks = be.to_dev(part)
            cap = 2 * len(part) + 65536
            dst, kd = be.empty(cap)
            bits.append(c.dev_compress_blocks(src, len(part), dst, cap))
            segs.append(dst)
            keep += [ks, kd]
        n = len(a) + len(b)
        cap = 2 * n + 65536
        out, kout = be.empty(cap)
        total = c.dev_assemble(n, segs, bits, out, cap)
        stream = be.to_host(kout, total)
        assert O.decompress(stream, n + 64) == a + b
        sp, ksp = be.to_dev(stream, 4)
        back, kb = be.empty(5 * bs + 64)                                    # (blocks are placed at multiples of the block size first)
        assert c.dev_decompress(sp, len(stream), back, 5 * bs + 64) == n
        assert be.to_host(kb, n) == a + b
        c.close()


FUZZ_BLOCK_SIZES = (1040, 3088, 5008, 16400, 20016, 65552)


def check_fuzz(be, cases, seed, max_n, heavy_max_n=None, block_sizes=FUZZ_BLOCK_SIZES, oracle_only=False):
    """parity_cases.check_fuzz's loop with its block sizes replaced (the data generators are that module's). oracle_only: no device, counts
    the cases the oracle takes (what the three-quarters bound below needs of a seed)."""
    r = np.random.default_rng(seed)
    tnames = ["NONE", "BWT", "RANK", "MTFT", "ZRLT", "LZ", "LZX", "LZP", "SRT", "UTF", "TEXT"]
    enames = ["NONE", "HUFFMAN", "ANS0", "ANS1", "FPAQ"]
    heavy = {"BWT", "RANK", "MTFT", "SRT"}
    done = 0
    for case in range(cases):
        nt = int(r.integers(1, 4))
        seq = [tnames[int(i)] for i in r.integers(0, len(tnames), nt)]
        transform = "+".join(seq)
        entropy = enames[int(r.integers(0, len(enames)))]
        bs = int(r.choice(block_sizes))
        lim = heavy_max_n if (heavy_max_n and heavy & set(seq)) else max_n
        n = int(r.integers(1, lim))
        if r.random() < 0.2:
            n = int(r.choice([1, 2, 15, 16, 31, 32, 33, bs - 1, bs, bs + 1, 2 * bs + 16]))
            n = max(1, min(n, lim))
        ck = int(r.choice([0, 0, 32, 64]))
        sk = bool(r.random() < 0.25)
        data = P._fuzz_data(r, n)
        tag = (case, transform, entropy, bs, n, ck, sk)
        cap = 2 * n + 262144 * (n // bs + 2)
        try:
            exp = O.compress(data, transform, entropy, bs, ck, skip_blocks=sk)
        except O.OracleError as e:                                          # inputs the reference itself fails on
            if not oracle_only:
                c = K.Codec(transform, entropy, bs, checksum_bits=ck, lib=be.lib, skip_blocks=sk)
                src, ks = be.to_dev(data)
                dst, kd = be.empty(cap)
                with P.pytest_raises_knz(e.code):
                    c.dev_compress(src, n, dst, cap)
                c.close()
            continue
        done += 1
        if oracle_only:
            continue
        c = K.Codec(transform, entropy, bs, checksum_bits=ck, lib=be.lib, skip_blocks=sk)
        src, ks = be.to_dev(data)
        dst, kd = be.empty(cap)
        nb = c.dev_compress(src, n, dst, cap)
        assert be.to_host(kd, nb) == exp, tag
        sp, ksp = be.to_dev(exp, 4)
        out, ko = be.empty(n + 64)
        assert c.dev_decompress(sp, len(exp), out, n + 64) == n, tag
        assert be.to_host(ko, n) == data, tag
        if case % 5 == 0 and ck == 0 and not sk:                            # the same input through the host-pointer batch hook
            bb = K.BlockBatch(c)
            blocks = [data[i:i + bs] for i in range(0, n, bs)]
            res = bb.encode(blocks)
            tt, et = O.transform_type(transform), O.entropy_type(entropy)
            for blk, (bits, written, mode, post, skip) in zip(blocks, res):
                o = O.encode_block(blk, tt, et)
                assert (written, bits, mode, post, skip) == (o["written"], o["bits"], o["mode"], o["post_len"], o["skip_flags"]), tag
            assert bb.decode([x[0] for x in res]) == blocks, tag
        c.close()
    assert done >= cases * 3 // 4, (done, cases)
    return done


# ---- 4. pointers at the contract's minimum alignment ---------------------------------------------------------------------------------------
def check_alignment(be, transform, entropy, bs, n, placements=PLACEMENTS, seed=4):
    """knz_dev_compress with d_src 16-byte and d_dst 4-byte aligned, knz_dev_decompress with the stream 4-byte aligned and d_dst anywhere:
    the oracle's bytes both ways, and every byte around both destinations untouched"""
    data = make_input(transform, n, seed)
    exp = expected(transform, entropy, bs, n, seed)
    c = K.Codec(transform, entropy, bs, lib=be.lib)
    for pl in placements:
        o_src, o_dst, o_str, o_out = pl
        tag = (transform, entropy, bs, n, pl)
        src, ksrc, _ = place(be, data, o_src)
        cap = len(exp) + 999
        dst, kdst, _ = place(be, cap, o_dst)
        nb = c.dev_compress(src, n, dst, cap)
        got = fetch(be, kdst, nb)
        assert got == exp, (tag, "device stream != oracle stream", M._diff(got, exp))
        guards_intact(be, kdst, cap)
        assert fetch(be, ksrc, n) == data, (tag, "the source was written")
        sp, ksp = place_stream(be, exp, o_str)
        ocap = n + 37
        out, kout, _ = place(be, ocap, o_out)
        nd = c.dev_decompress(sp, len(exp), out, ocap)
        assert nd == n, (tag, nd)
        back = fetch(be, kout, n)
        assert back == data, (tag, "oracle stream -> device decoder", M._diff(back, data))
        guards_intact(be, kout, ocap)
    c.close()


def check_sharded_alignment(be, entropy, bs, n, ranks=3):
    """knz_dev_compress_blocks into a destination at 4 mod 16, knz_dev_decompress_blocks from a segment at 12 mod 16 into an odd address,
    knz_dev_assemble from segments at 4, 8 and 12 mod 16 into a destination at 4 mod 16"""
    data = make_input("NONE", n, 5)
    exp = expected("NONE", entropy, bs, n, 5)
    nblocks = (n + bs - 1) // bs
    per = (nblocks + ranks - 1) // ranks
    assert per * (ranks - 1) < nblocks                                      # every rank has blocks
    c = K.Codec("NONE", entropy, bs, lib=be.lib)
    segs, bits, keep = [], [], []
    for r in range(ranks):
        part = data[r * per * bs: min((r + 1) * per * bs, n)]
        src, ksrc, _ = place(be, part, 16 * (2 * r + 1))
        cap = len(part) + len(part) // 2 + 4099
        dst, kdst, _ = place(be, cap, 4 + 16 * r)
        nbits = c.dev_compress_blocks(src, len(part), dst, cap)
        guards_intact(be, kdst, cap)
        seg = fetch(be, kdst, (nbits + 7) // 8)
        sp, ksp = place_stream(be, seg, 12 + 32 * r)
        ocap = len(part) + 1
        back, kback, _ = place(be, ocap, 2 * r + 1)
        assert c.dev_decompress_blocks(sp, nbits, back, ocap) == len(part), (entropy, bs, r)
        assert fetch(be, kback, len(part)) == part, (entropy, bs, r, "a rank decodes its own segment")
        guards_intact(be, kback, ocap)
        sp2, ksp2 = place_stream(be, seg, (4, 8, 12)[r % 3] + 16 * r)
        segs.append(sp2)
        bits.append(nbits)
        keep += [ksrc, kdst, ksp, ksp2]
    cap = len(exp) + 999
    out, kout, _ = place(be, cap, 244)
    total = c.dev_assemble(n, segs, bits, out, cap)
    got = fetch(be, kout, total)
    assert got == exp, (entropy, bs, "assembled stream != oracle stream", M._diff(got, exp))
    guards_intact(be, kout, cap)
    c.close()


def check_many_alignment(be, transform, entropy, bs, placements=PLACEMENTS):
    """one knz_dev_compress_many and one knz_dev_decompress_many call of five streams, every stream's pointers at another placement
    (knz_stream asks for a 4-byte aligned d_dst in both directions, so the decode destinations sit at 4, 8 and 12 mod 16)"""
    lens = (3 * bs + 777, 17, bs, 2 * bs + 1, bs + 16 + 5)
    c = K.Codec(transform, entropy, bs, lib=be.lib)
    datas = [make_input(transform, n, 6) for n in lens]
    exps = [expected(transform, entropy, bs, n, 6) for n in lens]
    call, keep = [], []
    for data, exp, pl in zip(datas, exps, placements):
        src, ksrc, _ = place(be, data, pl[0])
        cap = len(exp) + 999
        dst, kdst, _ = place(be, cap, pl[1])
        call.append((src, len(data), dst, cap))
        keep.append((ksrc, kdst, cap))
    res = c.dev_compress_many(call)
    assert c.last_many_rc == 0, (c.last_many_rc, res)
    for i, ((nb, status), (_ks, kd, cap), exp) in enumerate(zip(res, keep, exps)):
        assert status == 0 and fetch(be, kd, nb) == exp, (transform, entropy, bs, i, status, "stream of the many call != oracle stream")
        guards_intact(be, kd, cap)
    call, keep = [], []
    for data, exp, pl in zip(datas, exps, placements):
        sp, ksp = place_stream(be, exp, pl[2])
        cap = len(data) + 37
        dst, kdst, _ = place(be, cap, 4 * pl[3])                            # (knz_stream.d_dst is 4-byte aligned in both directions: the minimum here is 4, not 1)
        call.append((sp, len(exp), dst, cap))
        keep.append((ksp, kdst, cap))
    res = c.dev_decompress_many(call)
    assert c.last_many_rc == 0, (c.last_many_rc, res)
    for i, ((nb, status), (_ks, kd, cap), data) in enumerate(zip(res, keep, datas)):
        assert status == 0 and nb == len(data) and fetch(be, kd, nb) == data, (transform, entropy, bs, i, status, "oracle stream -> dev_decompress_many")
        guards_intact(be, kd, cap)
    c.close()


# ---- 5. capacities -------------------------------------------------------------------------------------------------------------------------
def check_tight_capacity(be, transform, entropy, bs, n, seed=7):
    """the header's rule at its edge: the stream plus 7 bytes is enough for the compress calls (whole big-endian words are stored), the
    stream's own length is not; the decoder needs the bytes it gives back and no more; nothing is written at or behind dst_cap either way"""
    assert n % 2 == 1
    data = make_input(transform, n, seed)
    exp = expected(transform, entropy, bs, n, seed)
    tag = (transform, entropy, bs, n)
    c = K.Codec(transform, entropy, bs, lib=be.lib)
    src, ksrc, _ = place(be, data, 16)
    cap = len(exp) + 7
    dst, kdst, _ = place(be, cap, 4)
    nb = c.dev_compress(src, n, dst, cap)
    assert fetch(be, kdst, nb) == exp, (tag, "dst_cap = stream + 7")
    guards_intact(be, kdst, cap)
    cap = len(exp)
    dst, kdst, _ = place(be, cap, 12)
    with P.pytest_raises_knz(ERR_WRITE_FILE):
        c.dev_compress(src, n, dst, cap)
    guards_intact(be, kdst, cap)
    sp, ksp = place_stream(be, exp, 4)
    out, kout, _ = place(be, n, 3)
    assert c.dev_decompress(sp, len(exp), out, n) == n, tag
    assert fetch(be, kout, n) == data, (tag, "dst_cap = n")
    guards_intact(be, kout, n)
    out, kout, _ = place(be, n - 1, 1)
    with P.pytest_raises_knz(ERR_WRITE_FILE):                               # (decode_batch: "destination buffer too small", as knz_decode_blocks answers per block)
        c.dev_decompress(sp, len(exp), out, n - 1)
    guards_intact(be, kout, n - 1)
    c.close()


# ---- 6. single objects through host pointers at odd addresses -------------------------------------------------------------------------------
class _Host:
    """place() for host memory whatever the backend: the single-object calls take host pointers"""
    name = "emu"


_HOST = _Host()
_u8p = C.POINTER(C.c_uint8)
OBJECT_LENGTHS = (1040, 16400, 16401)


def _hp(ptr):
    return C.cast(C.c_void_p(ptr), _u8p)


def check_entropy_objects_unaligned(be, ename):
    c = K.Codec("NONE", ename, 1 << 16, lib=be.lib)
    L, et = c.L, O.entropy_type(ename)
    for i, n in enumerate(OBJECT_LENGTHS):
        data = P.corpus(n, 20 + i)
        ob, obits = O.entropy_encode(et, data)
        src, ksrc, _ = place(_HOST, data, 1 + 2 * i)
        cap = len(ob) + 8 + i
        dst, kdst, _ = place(_HOST, cap, 3 + 4 * i)
        bits = C.c_uint64()
        c._chk(L.knz_entropy_encode(c.h, et, _hp(src), n, _hp(dst), cap, C.byref(bits)))
        assert bits.value == obits and fetch(_HOST, kdst, (obits + 7) // 8) == ob, (ename, n, bits.value, obits)
        guards_intact(_HOST, kdst, cap)
        sp, ksp, _ = place(_HOST, ob, 5 + 2 * i)
        out, kout, _ = place(_HOST, n, 7 + 8 * i)
        used = C.c_uint64()
        c._chk(L.knz_entropy_decode(c.h, et, _hp(sp), len(ob), _hp(out), n, C.byref(used)))
        assert fetch(_HOST, kout, n) == data and used.value == obits, (ename, n, used.value, obits)
        guards_intact(_HOST, kout, n)
    c.close()


def _object_input(tname, n, seed):
    if tname == "UTF":
        return P.utf_text(n, seed, (1,))
    if tname == "TEXT":
        return text_corpus.make_text(n, seed=seed)
    if tname == "LZP":                                                      # records that repeat: predictions that hold (LZP declines the plain corpus)
        return (P.corpus(300, seed) * (n // 300 + 1))[:n]
    return P.corpus(n, seed)


def check_transform_objects_unaligned(be, tname):
    bs = 1 << 20
    c = K.Codec("NONE", "NONE", bs, lib=be.lib)
    L, tid = c.L, P._TID[tname]
    applied = 0
    for i, n in enumerate(OBJECT_LENGTHS):
        data = _object_input(tname, n, 30 + i)
        O.set_ctx(bs, O.E_NONE)                                             # (TEXT reads ctx: the handle's block size and entropy stage)
        o = O.transform_forward(tid, data)
        src, ksrc, _ = place(_HOST, data, 1 + 2 * i)
        cap = int(L.knz_max_encoded_len(tid << 42, n)) + 61
        dst, kdst, _ = place(_HOST, cap, 3 + 4 * i)
        m = C.c_uint32()
        rc = L.knz_transform_forward(c.h, tid, _hp(src), n, _hp(dst), cap, C.byref(m))
        assert (rc == -1) == (o is None), (tname, n, rc, "one declines, the other does not")
        guards_intact(_HOST, kdst, cap)
        if o is None:
            continue
        c._chk(rc)
        assert fetch(_HOST, kdst, m.value) == o, (tname, n, m.value, len(o))
        applied += 1
        sp, ksp, _ = place(_HOST, o, 5 + 2 * i)
        ocap = n + 513
        out, kout, _ = place(_HOST, ocap, 7 + 8 * i)
        c._chk(L.knz_transform_inverse(c.h, tid, _hp(sp), len(o), _hp(out), ocap, C.byref(m)))
        assert m.value == n and fetch(_HOST, kout, n) == data, (tname, n, m.value)
        guards_intact(_HOST, kout, ocap)
    O.set_ctx()
    c.close()
    assert applied >= 2, (tname, applied, "the transform declined these inputs: nothing was compared")


# ---- 7. coverage guard, from the tables alone -----------------------------------------------------------------------------------------------
def check_coverage(gpu_cases=None, emu_cases=None, placements=PLACEMENTS):
    """what keeps a later edit of the tables from turning this file back into the aligned case"""
    gpu_cases = stream_cases(True) if gpu_cases is None else gpu_cases
    emu_cases = stream_cases(False) if emu_cases is None else emu_cases
    for name, cases in (("gpu", gpu_cases), ("emu", emu_cases)):
        for ename, chunk in CHUNK.items():
            if name == "emu" and chunk > (1 << 20):                          # the 4 MiB + 16 size runs on the device only
                continue
            assert any(e == ename and bs % chunk == 16 for _t, e, bs, _n, _s in cases), (name, ename, "no block size that leaves a 16-byte chunk")
        sizes = {bs for _t, _e, bs, _n, _s in cases}
        assert any(bs % 64 == 16 for bs in sizes) and any(bs % 64 == 48 for bs in sizes), (name, sorted(sizes))
        assert all(bs % 16 == 0 and bs & (bs - 1) for bs in sizes), (name, sorted(sizes), "a power of two among the block sizes")
        for t, e, bs, n, _s in cases:
            assert (n + bs - 1) // bs >= 3 and (n % bs) % 16 != 0, (name, t, e, bs, n)
        for pipe in NONE_PIPES + XF_PIPES:
            assert any((t, e) == pipe for t, e, _bs, _n, _s in cases), (name, pipe)
    srcs, dsts, strs, outs = zip(*placements)
    assert any(s % 32 == 16 for s in srcs) and all(s % 16 == 0 for s in srcs), srcs
    assert all(d % 4 == 0 for d in dsts) and any(d % 16 for d in dsts), dsts
    assert {4, 8, 12} <= {s % 16 for s in strs} and all(s % 4 == 0 for s in strs), strs
    assert {1, 2, 3} <= {o % 4 for o in outs}, outs
    assert len(placements) >= 5 and len(set(placements)) == len(placements)
    for _t, _e, bs_a, _n, bs_b, _m in ALIGN_CASES:
        assert bs_a & (bs_a - 1) == 0 and bs_b in BLOCK_SIZES, (bs_a, bs_b)
    assert all(n % 2 for _t, _e, _bs, n in TIGHT_CASES)
