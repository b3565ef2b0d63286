// Remaining C-ABI entry points (included by knz_gpu.hip): stream decode, host-pointer batch calls,
// multi-GPU segment assembly, single-codec objects.

// ---- stream header parse (host side of Reader.readHeader, v2/io/CompressedStream.go:1316-1460) ------------------------
static uint64_t hdr_get(const uint8_t* p, uint32_t& pos, uint32_t count) {
    uint64_t v = 0;
    for (uint32_t i = 0; i < count; i++, pos++) v = (v << 1) | ((p[pos >> 3] >> (7 - (pos & 7))) & 1);
    return v;
}

static int parse_stream_header(Handle* h, const uint8_t* hdr, uint64_t avail, knz_cfg& out, int64_t& outputSize, uint32_t& bits) {
    if (avail < 20) return knz_set_error(h, KNZ_ERR_INVALID_FILE, "stream too short");
    uint32_t pos = 0;
    if (hdr_get(hdr, pos, 32) != 0x4B414E5Au) return knz_set_error(h, KNZ_ERR_INVALID_FILE, "Invalid stream type");
    uint32_t ver = (uint32_t)hdr_get(hdr, pos, 4);
    if (ver > 6) return knz_set_error(h, KNZ_ERR_STREAM_VERSION, "Invalid bitstream, cannot read this version of the stream");
    if (ver != 6) return knz_set_error(h, KNZ_ERR_STREAM_VERSION, "only bitstream version 6 is decoded on the device");
    uint32_t ck = (uint32_t)hdr_get(hdr, pos, 2);
    if (ck == 3) return knz_set_error(h, KNZ_ERR_INVALID_CODEC, "Invalid bitstream, incorrect checksum size");
    out.checksum_bits = ck == 1 ? 32 : (ck == 2 ? 64 : 0);
    out.entropy = (uint32_t)hdr_get(hdr, pos, 5);
    out.transform = hdr_get(hdr, pos, 48);
    out.block_size = (uint32_t)(hdr_get(hdr, pos, 28) << 4);
    if (out.block_size < 1024 || out.block_size > (1u << 30)) return knz_set_error(h, KNZ_ERR_BLOCK_SIZE, "Invalid bitstream, incorrect block size");
    uint32_t szMask = (uint32_t)hdr_get(hdr, pos, 2);
    if (avail * 8 < pos + 16 * szMask + 39) return knz_set_error(h, KNZ_ERR_INVALID_FILE, "stream too short");
    outputSize = szMask ? (int64_t)hdr_get(hdr, pos, 16 * szMask) : 0;
    hdr_get(hdr, pos, 15);
    uint32_t ck1 = (uint32_t)hdr_get(hdr, pos, 24);
    uint32_t words[8];
    knz_cfg tmp = out;
    uint32_t hb = knz_build_stream_header(tmp, szMask ? outputSize : 0, words);
    // szMask 0 with a non-zero size cannot be rebuilt; compare the checksum field only
    uint32_t cpos = hb - 24, ck2 = 0;
    for (uint32_t i = 0; i < 24; i++, cpos++) ck2 = (ck2 << 1) | ((words[cpos >> 5] >> (31 - (cpos & 31))) & 1);
    if (hb != pos || ck1 != ck2) return knz_set_error(h, KNZ_ERR_CRC_CHECK, "Invalid bitstream: checksum mismatch");
    bits = pos;
    return KNZ_OK;
}

// the head of a stream at d_src, brought over and parsed: its codec parameters, size field and first block's bit
static int read_stream_header(Handle* h, const void* d_src, uint64_t n_bytes, hipStream_t st, knz_cfg& sc, int64_t& outputSize, uint32_t& hbits) {
    uint8_t hdr[32] = {0};
    HIP_OK(hipMemcpyAsync(hdr, d_src, std::min<uint64_t>(32, n_bytes), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return parse_stream_header(h, hdr, n_bytes, sc, outputSize, hbits);
}

// what a range asks for that can be refused before the device is asked (hbits: the first block's bit, from the stream's header)
static int check_block_range(Handle* h, const knz_block_range& r, uint64_t n_bytes, uint32_t hbits) {
    if (r.from_block == 0 || r.to_block <= r.from_block) return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "invalid block range");
    if (r.from_bit != 0 && (r.from_bit >= 8 * n_bytes || r.from_bit < hbits)) return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "from_bit lies outside the stream's blocks");
    return KNZ_OK;
}

// knz_dev_decompress and knz_dev_decompress_range: the whole stream (range == nullptr) or the blocks of a range, packed from d_dst on
static int dev_decompress_stream(void* handle, const void* d_src, uint64_t n_bytes, const knz_block_range* range, void* d_dst, uint64_t dst_cap,
                                 uint64_t* out_bytes, void* hip_stream) {
    Handle* h = lane_of_pointer((Handle*)handle, d_dst);
    if (!h || !d_src || !d_dst || !out_bytes) return KNZ_ERR_MISSING_PARAM;
    DeviceGuard dg(h);
    if ((uintptr_t)d_src & 3) return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "d_src must be 4-byte aligned");
    hipStream_t st = dev_call_stream(h, hip_stream);
    knz_cfg sc = h->cfg;
    int64_t outputSize = 0;
    uint32_t hbits = 0;
    int rc = read_stream_header(h, d_src, n_bytes, st, sc, outputSize, hbits);
    if (rc) return rc;
    DecodeBatch db(sc, (const uint8_t*)d_src, n_bytes, (uint8_t*)d_dst, dst_cap);   // (what the stream's header says, whatever the handle was opened with)
    db.first_bit = hbits;
    if (range) {
        if ((rc = check_block_range(h, *range, n_bytes, hbits)) != KNZ_OK) return rc;
        const uint64_t to = range->to_block == KNZ_BLOCK_END ? ~(uint64_t)0 : range->to_block;
        if (range->from_bit) db.range(range->from_bit, range->from_block, range->from_block, to, true);
        else db.range(hbits, 1, range->from_block, to, false);
    }
    rc = decode_batch(h, db, st);
    if (rc) return rc;
    // A kanzi Writer fills every block but the last (:536-560), and the batch placed block b at b * block_size. The Reader accepts
    // short blocks anywhere (concatenated streams, other writers): close the gaps, front to back, through a staging buffer (rare).
    bool gaps = false;
    for (uint32_t b = 0; b + 1 < db.nblocks; b++) gaps = gaps || db.pre_len[b] != sc.block_size;
    if (gaps) {
        if (h->stage_out.reserve((uint64_t)sc.block_size + 64)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
        uint64_t at = 0;
        for (uint32_t b = 0; b < db.nblocks; b++) {
            const uint64_t from = (uint64_t)b * sc.block_size;
            if (from != at && db.pre_len[b]) {
                HIP_OK(hipMemcpyAsync(h->stage_out.p, (uint8_t*)d_dst + from, db.pre_len[b], hipMemcpyDeviceToDevice, st));
                HIP_OK(hipMemcpyAsync((uint8_t*)d_dst + at, h->stage_out.p, db.pre_len[b], hipMemcpyDeviceToDevice, st));
            }
            at += db.pre_len[b];
        }
        HIP_OK(hipStreamSynchronize(st));
    }
    *out_bytes = db.total_out;
    return KNZ_OK;
}

extern "C" int knz_dev_decompress(void* handle, const void* d_src, uint64_t n_bytes, void* d_dst, uint64_t dst_cap,
                                  uint64_t* out_bytes, void* hip_stream) {
    return dev_decompress_stream(handle, d_src, n_bytes, nullptr, d_dst, dst_cap, out_bytes, hip_stream);
}

extern "C" int knz_dev_decompress_range(void* handle, const void* d_src, uint64_t n_bytes, const knz_block_range* range, void* d_dst, uint64_t dst_cap,
                                        uint64_t* out_bytes, void* hip_stream) {
    if (!range) return KNZ_ERR_MISSING_PARAM;
    return dev_decompress_stream(handle, d_src, n_bytes, range, d_dst, dst_cap, out_bytes, hip_stream);
}

// The index of a stream: its header's fields, and the walk of knz_dev_decompress_range over every frame, recording where each starts. The count, the end
// bit and the first pos_cap rows come back in one pinned copy.
extern "C" int knz_dev_stream_index(void* handle, const void* d_src, uint64_t n_bytes, knz_stream_info* info, knz_block_pos* pos, uint32_t pos_cap,
                                    void* hip_stream) {
    Handle* h = lane_of_pointer((Handle*)handle, d_src);
    if (!h || !d_src || !info) return KNZ_ERR_MISSING_PARAM;
    DeviceGuard dg(h);
    if ((uintptr_t)d_src & 3) return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "d_src must be 4-byte aligned");
    hipStream_t st = dev_call_stream(h, hip_stream);
    knz_cfg sc = h->cfg;
    int64_t outputSize = 0;
    uint32_t hbits = 0;
    int rc = read_stream_header(h, d_src, n_bytes, st, sc, outputSize, hbits);
    if (rc) return rc;
    const uint32_t bound = (uint32_t)std::min<uint64_t>(n_bytes / 3 + 1, 1u << 24);       // (dec_walk_framing's: 8 framing + 16 payload bits a block at least)
    const uint32_t cap = pos ? std::min(pos_cap, bound) : 0;
    const size_t bytes = 8 * (4 + 2 * (size_t)cap);
    if (h->blk_dst_bit.reserve(bytes)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
    if (h->pinned_rows.reserve(bytes)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "pinned host allocation failed");
    WalkRangeArgs wr;
    wr.stream = (const uint8_t*)d_src; wr.nbytes = n_bytes; wr.first_bit = hbits; wr.first_id = 1; wr.from = 1; wr.to = ~(uint64_t)0;
    wr.max_blocks = bound; wr.cap = cap; wr.frames = 1; wr.stride = 2; wr.hinted = 0;
    wr.result = h->blk_dst_bit.as<uint64_t>(); wr.blk_bit = wr.result + 4; wr.blk_bits = wr.result + 5;
    hipLaunchKernelGGL(knz_dec_walk_range_kernel, dim3(1), dim3(1), 0, st, wr);
    const uint64_t* res = h->pinned_rows.as<uint64_t>();
    HIP_OK(hipMemcpyAsync(h->pinned_rows.p, h->blk_dst_bit.p, bytes, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    if (res[1]) return knz_set_error(h, (int)res[1], "invalid block framing in stream");
    info->transform = sc.transform; info->entropy = sc.entropy; info->block_size = sc.block_size; info->checksum_bits = sc.checksum_bits; info->bs_version = 6;
    info->output_size = outputSize; info->header_bits = hbits; info->n_blocks = (uint32_t)res[0]; info->end_bit = res[2];
    if (pos) memcpy(pos, res + 4, sizeof(knz_block_pos) * (size_t)std::min<uint64_t>(res[0], cap));
    return KNZ_OK;
}

extern "C" int knz_dev_decompress_blocks(void* handle, const void* d_src, uint64_t n_bits, void* d_dst, uint64_t dst_cap,
                                         uint64_t* out_bytes, void* hip_stream) {
    Handle* h = lane_of_pointer((Handle*)handle, d_dst);
    if (!h || !d_src || !d_dst || !out_bytes) return KNZ_ERR_MISSING_PARAM;
    DeviceGuard dg(h);
    if ((uintptr_t)d_src & 3) return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "d_src must be 4-byte aligned");
    *out_bytes = 0;
    if (n_bits == 0) return KNZ_OK;
    hipStream_t st = dev_call_stream(h, hip_stream);
    DecodeBatch db(h->cfg, (const uint8_t*)d_src, (n_bits + 7) >> 3, (uint8_t*)d_dst, dst_cap);
    db.seg_bits = n_bits;
    int rc = decode_batch(h, db, st);
    if (rc) return rc;
    *out_bytes = db.total_out;
    return KNZ_OK;
}

// ---- host-pointer batch entry points ------------------------------------------------------------------------------------
static int encode_blocks_once(Handle* h, knz_block* blocks, int n);
static int decode_blocks_once(Handle* h, knz_block* blocks, int n);
// A range [lo, lo + cnt) of blocks or streams whose workspace the device cannot hold any more (other handles, other tenants) is taken in halves after the
// handle's own workspace has been given back: blocks are independent (Definitions.go:73-77), so the result is the same, with fewer of them side by side.
// failed(lo, cnt, rc) hears of every range that failed for good ; both_halves: a first half that did still lets the second run ; callers: the caller's
// stream or null, synchronised before the workspace goes (the handle's own ones always are).
template <typename Once, typename Failed>
static int split_retry(Handle* h, int lo, int cnt, bool both_halves, const hipStream_t* callers, Once once, Failed failed) {
    g_alloc_refused = false;
    int rc = once(lo, cnt);
    if (rc != KNZ_OK && g_alloc_refused) {
        if (callers) hipStreamSynchronize(*callers);
        knz_release_workspace(h);
        g_alloc_refused = false;
        if (cnt > 1) {
            const int half = cnt / 2;
            rc = split_retry(h, lo, half, both_halves, callers, once, failed);
            if (rc && !both_halves) return rc;
            const int rc2 = split_retry(h, lo + half, cnt - half, both_halves, callers, once, failed);
            return rc ? rc : rc2;
        }
        rc = once(lo, cnt);                                       // (once more with nothing else of this handle resident)
    }
    if (rc != KNZ_OK) failed(lo, cnt, rc);
    return rc;
}
// the blocks form: the first half that fails for good ends the batch with its code (knz_multi.inc's lanes call it for their ranges)
static int blocks_split_retry(Handle* h, knz_block* blocks, int n, int (*once)(Handle*, knz_block*, int)) {
    return split_retry(h, 0, n, false, nullptr, [&](int lo, int cnt) { return once(h, blocks + lo, cnt); }, [](int, int, int) {});
}

// What the block-local stream of a block of len bytes can take, rounded up to 64 (the stride of such streams in stage_out): the longest the transform
// sequence can make the block, coded at 12 bits a byte at the worst (the longest Huffman code), 1 KiB for the block header and the coders' chunk
// headers, and for rANS order 1 its context headers: up to 128 KiB per 4 MiB chunk, two chunks to spare.
static uint64_t block_stream_bound(uint64_t transform, uint32_t entropy, uint64_t len) {
    const uint64_t ans1 = entropy == KNZ_E_ANS1 ? 131072ull * (len / (4u << 20) + 2) : 0;
    return ((uint64_t)knz_max_encoded_len(transform, (uint32_t)std::max<uint64_t>(len, 1)) * 12 / 8 + 1024 + ans1 + 63) & ~(uint64_t)63;
}
extern "C" int knz_encode_blocks(void* handle, knz_block* blocks, int n) {
    Handle* h = (Handle*)handle;
    if (!h || (!blocks && n)) return KNZ_ERR_MISSING_PARAM;
    if (n <= 0) return KNZ_OK;
    if (h->multi) return multi_blocks(h, blocks, n, 1);
    DeviceGuard dg(h);
    return blocks_split_retry(h, blocks, n, encode_blocks_once);
}
static int encode_blocks_once(Handle* h, knz_block* blocks, int n) {
    hipStream_t st = host_call_stream(h);
    const uint64_t bs = h->cfg.block_size;
    // stage the blocks at block_size stride; all but the last must be full for the shared block table
    for (int i = 0; i < n; i++) {
        blocks[i].status = 0;
        if (!blocks[i].src || !blocks[i].dst || blocks[i].src_len == 0 || blocks[i].src_len > bs) return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "invalid block descriptor");
        if (i + 1 < n && blocks[i].src_len != bs) return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "only the last block of a batch may be short");
    }
    const uint64_t total = (uint64_t)(n - 1) * bs + blocks[n - 1].src_len;
    const uint64_t ostride = block_stream_bound(h->cfg.transform, h->cfg.entropy, bs);
    if (h->stage_in.reserve(total + 64) || h->stage_out.reserve(ostride * n + 64)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
    for (int i = 0; i < n; i++)
        HIP_OK(hipMemcpyAsync(h->stage_in.as<uint8_t>() + (uint64_t)i * bs, blocks[i].src, blocks[i].src_len, hipMemcpyHostToDevice, st));
    EncodeBatch eb = EncodeBatch::block_streams(h->stage_in.as<uint8_t>(), total, h->stage_out.as<uint8_t>(), ostride, (uint64_t)n);
    int rc = encode_batch(h, eb, st);
    if (rc) { for (int i = 0; i < n; i++) blocks[i].status = rc; return rc; }
    const Handle::ResultRow* rows = h->pinned_rows.as<Handle::ResultRow>();   // (filled by encode_batch: nothing more to bring over but the streams themselves)
    int worst = KNZ_OK;
    for (int i = 0; i < n; i++) {
        const uint64_t nb = (rows[i].written + 7) >> 3;
        blocks[i].out_bits = rows[i].written;
        blocks[i].post_len = rows[i].post_len;
        blocks[i].mode = (uint8_t)rows[i].mode;
        blocks[i].skip_flags = (uint8_t)rows[i].skip;     // bit 7-k set = transform k of the sequence was skipped (Sequence.go:86-91)
        blocks[i].checksum = h->cfg.checksum_bits ? rows[i].cksum : 0;
        if (nb > blocks[i].dst_cap) { blocks[i].status = KNZ_ERR_WRITE_FILE; worst = KNZ_ERR_WRITE_FILE; continue; }
        HIP_OK(hipMemcpyAsync(blocks[i].dst, h->stage_out.as<uint8_t>() + (uint64_t)i * ostride, nb, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    if (worst) return knz_set_error(h, worst, "destination buffer too small");
    return KNZ_OK;
}

extern "C" int knz_decode_blocks(void* handle, knz_block* blocks, int n) {
    Handle* h = (Handle*)handle;
    if (!h || (!blocks && n)) return KNZ_ERR_MISSING_PARAM;
    if (n <= 0) return KNZ_OK;
    if (h->multi) return multi_blocks(h, blocks, n, 2);
    DeviceGuard dg(h);
    return blocks_split_retry(h, blocks, n, decode_blocks_once);
}
// Staging for an unframed decode: the payloads side by side in stage_in, each at a multiple of 8 bytes with zeros between and behind them, their bit
// positions in blk_dst_bit and bit counts in blk_written, out_bytes of room in stage_out. `total`: the staged bytes.
struct Payload { const uint8_t* p; uint64_t len; };
static int dec_stage_payloads(Handle* h, const std::vector<Payload>& pl, uint64_t out_bytes, uint64_t& total, hipStream_t st) {
    const size_t n = pl.size();
    std::vector<uint64_t> bit(n), bits(n);
    total = 0;
    for (size_t i = 0; i < n; i++) { bit[i] = total * 8; bits[i] = pl[i].len * 8; total += (pl[i].len + 7) & ~(uint64_t)7; }
    if (h->stage_in.reserve(total + 64) || h->stage_out.reserve(out_bytes + 64) || h->blk_dst_bit.reserve(8 * n + 8) || h->blk_written.reserve(8 * n + 8))
        return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
    HIP_OK(hipMemsetAsync(h->stage_in.p, 0, total + 64, st));
    for (size_t i = 0; i < n; i++)
        HIP_OK(hipMemcpyAsync(h->stage_in.as<uint8_t>() + (bit[i] >> 3), pl[i].p, pl[i].len, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(h->blk_dst_bit.p, bit.data(), 8 * n, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(h->blk_written.p, bits.data(), 8 * n, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
    return KNZ_OK;
}

static int decode_blocks_once(Handle* h, knz_block* blocks, int n) {
    hipStream_t st = host_call_stream(h);
    const uint64_t bs = h->cfg.block_size;
    std::vector<Payload> pl(n);
    for (int i = 0; i < n; i++) {
        blocks[i].status = 0;
        if (!blocks[i].src || !blocks[i].dst || blocks[i].src_len == 0) return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "invalid block descriptor");
        pl[i] = {blocks[i].src, blocks[i].src_len};
    }
    const uint64_t ostride = (bs + 63) & ~(uint64_t)63;
    uint64_t total = 0;
    int rc = dec_stage_payloads(h, pl, ostride * n, total, st);
    if (rc) return rc;
    DecodeBatch db(h->cfg, h->stage_in.as<uint8_t>(), total, h->stage_out.as<uint8_t>(), ostride * n);
    db.unframed((uint32_t)n, ostride);
    rc = decode_batch(h, db, st);
    if (rc) {
        for (int i = 0; i < n; i++) blocks[i].status = (i < (int)db.status.size() && db.status[i]) ? db.status[i] : rc;
        return rc;
    }
    int worst = KNZ_OK;
    for (int i = 0; i < n; i++) {
        blocks[i].out_bits = db.pre_len[i];
        blocks[i].post_len = db.pre_len[i];
        if (db.pre_len[i] > blocks[i].dst_cap) { blocks[i].status = KNZ_ERR_WRITE_FILE; worst = KNZ_ERR_WRITE_FILE; continue; }
        HIP_OK(hipMemcpyAsync(blocks[i].dst, h->stage_out.as<uint8_t>() + (uint64_t)i * ostride, db.pre_len[i], hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    if (worst) return knz_set_error(h, worst, "destination buffer too small");
    return KNZ_OK;
}

// ---- multi-GPU assembly: header | segment bit strings in rank order | end marker -----------------------------------------
struct ConcatArgs { const uint8_t* src; uint64_t nbits; uint32_t* dst_words; uint64_t dst_bit; };

__global__ __launch_bounds__(256) void knz_concat_segment_kernel(ConcatArgs a) {
    if (a.nbits == 0) return;
    const uint64_t w0 = a.dst_bit >> 5, w1 = (a.dst_bit + a.nbits - 1) >> 5;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t w = w0 + (uint64_t)blockIdx.x * 256 + threadIdx.x; w <= w1; w += stride) {
        const uint32_t v = knz_fetch32(a.src, (int64_t)(w << 5) - (int64_t)a.dst_bit, (int64_t)a.nbits);
        const uint32_t sw = knz_bswap32(v);
        if (w == w0 || w == w1) atomicOr(&a.dst_words[w], sw);
        else a.dst_words[w] = sw;
    }
}

// The concat kernels store interior words and OR the two boundary words of a segment: only those need zeroing first.
#define KNZ_ASM_ZERO_MAX 160
struct ZeroWordsArgs { uint32_t* dst; uint32_t n; uint64_t w[KNZ_ASM_ZERO_MAX]; };

__global__ __launch_bounds__(256) void knz_zero_words_kernel(ZeroWordsArgs a) {
    if (threadIdx.x < a.n) a.dst[a.w[threadIdx.x]] = 0;
}

extern "C" int knz_dev_assemble(void* handle, int64_t header_input_size, const void* const* d_segments,
                                const uint64_t* segment_bits, int n_segments, void* d_dst, uint64_t dst_cap,
                                uint64_t* out_bytes, void* hip_stream) {
    Handle* h = lane_of_pointer((Handle*)handle, d_dst);
    if (!h || !d_dst || !out_bytes || (n_segments && (!d_segments || !segment_bits))) return KNZ_ERR_MISSING_PARAM;
    DeviceGuard dg(h);
    if ((uintptr_t)d_dst & 3) return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "d_dst must be 4-byte aligned");
    hipStream_t st = dev_call_stream(h, hip_stream);
    uint32_t words[8];
    const uint32_t hbits = knz_build_stream_header(h->cfg, header_input_size, words);
    uint64_t total = hbits;
    for (int i = 0; i < n_segments; i++) total += segment_bits[i];
    total += 8; // end marker (:593-594)
    const uint64_t nbytes = (total + 7) >> 3;
    if (((nbytes + 3) & ~(uint64_t)3) + 4 > dst_cap) return knz_set_error(h, KNZ_ERR_WRITE_FILE, "destination buffer too small");
    const uint64_t nwords = (nbytes + 3) >> 2;
    if (2 * (uint64_t)n_segments + 12 <= KNZ_ASM_ZERO_MAX) {
        ZeroWordsArgs za;
        za.dst = (uint32_t*)d_dst; za.n = 0;
        for (uint64_t w = 0; w < 8 && w < nwords; w++) za.w[za.n++] = w;                     // header words (<= 26 bytes) + the first segment's first word
        uint64_t q = hbits;
        for (int i = 0; i < n_segments; i++) {
            if (segment_bits[i]) { za.w[za.n++] = q >> 5; za.w[za.n++] = (q + segment_bits[i] - 1) >> 5; }
            q += segment_bits[i];
        }
        za.w[za.n++] = q >> 5;                                                                // end marker byte and the padding of the last word
        za.w[za.n++] = std::min(nwords - 1, (q + 7) >> 5);
        za.w[za.n++] = nwords - 1;
        hipLaunchKernelGGL(knz_zero_words_kernel, dim3(1), dim3(256), 0, st, za);
    } else {
        HIP_OK(hipMemsetAsync(d_dst, 0, nwords * 4, st));
    }
    uint8_t hb[32];
    for (int i = 0; i < 8; i++) { hb[4 * i] = (uint8_t)(words[i] >> 24); hb[4 * i + 1] = (uint8_t)(words[i] >> 16); hb[4 * i + 2] = (uint8_t)(words[i] >> 8); hb[4 * i + 3] = (uint8_t)words[i]; }
    memcpy(h->pinned, hb, 32);
    HIP_OK(hipMemcpyAsync(d_dst, h->pinned, (hbits + 7) >> 3, hipMemcpyHostToDevice, st)); // header is a whole number of bytes (160+16k bits)
    uint64_t pos = hbits;
    for (int i = 0; i < n_segments; i++) {
        if ((uintptr_t)d_segments[i] & 3) return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "segments must be 4-byte aligned");
        ConcatArgs ca{(const uint8_t*)d_segments[i], segment_bits[i], (uint32_t*)d_dst, pos};
        const uint64_t nw = (segment_bits[i] + 31) / 32 + 1;
        const unsigned grid = (unsigned)std::min<uint64_t>((nw + 255) / 256, 4096);
        if (segment_bits[i]) hipLaunchKernelGGL(knz_concat_segment_kernel, dim3(grid), dim3(256), 0, st, ca);
        pos += segment_bits[i];
    }
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    *out_bytes = nbytes;
    return KNZ_OK;
}

// ---- single kanzi.ByteTransform / EntropyEncoder / EntropyDecoder objects ------------------------------------------------
// One ByteTransform object on one buffer: a batch of one block through the same stage kernels.
static int transform_single(void* handle, uint64_t type1, bool forward, const uint8_t* src, uint32_t n, uint8_t* dst, uint32_t cap, uint32_t* out_n) {
    Handle* h = lane0((Handle*)handle);
    if (!h || !src || !dst || !out_n) return KNZ_ERR_MISSING_PARAM;
    DeviceGuard dg(h);
    if (!xf_codec((uint32_t)type1)) return knz_set_error(h, KNZ_ERR_INVALID_CODEC, "transform has no device implementation in this build");
    *out_n = 0;
    if (n == 0 || cap == 0) return KNZ_OK;                                  // every Forward/Inverse returns (0,0,nil) on empty input
    if (type1 == KNZ_T_NONE) {
        if (cap < n) return forward ? KNZ_SKIP : knz_set_error(h, KNZ_ERR_PROCESS_BLOCK, "Destination buffer too small");
        memcpy(dst, src, n);                                                // NullTransform: nothing for the device to do
        *out_n = n;
        return KNZ_OK;
    }
    hipStream_t st = host_call_stream(h);
    XfBatch x;
    const uint64_t stride = ((uint64_t)cap + 15) & ~(uint64_t)15;
    if (xf_alloc(h, x, 1, stride) || h->stage_in.reserve((uint64_t)n + 64) || h->blk_off.reserve(16) || h->blk_len.reserve(16) ||
        h->blk_skip.reserve(32) || h->blk_status.reserve(16))
        return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
    x.cur_ptr = h->blk_off.as<uint64_t>(); x.cur_len = h->blk_len.as<uint32_t>(); x.skip = h->blk_skip.as<uint8_t>(); x.blk_status = h->blk_status.as<int32_t>();
    const uint64_t p = (uint64_t)h->stage_in.p;
    const uint8_t one = 1, zero = 0, ff = 0xFF;
    const int32_t z32 = 0;
    HIP_OK(hipMemcpyAsync(h->stage_in.p, src, n, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(x.cur_ptr, &p, 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(x.cur_len, &n, 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(x.skip, &ff, 1, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(x.active, &one, 1, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(x.side, &zero, 1, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(x.blk_status, &z32, 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
    CommitArgs c = xf_commit_args(h, x, 0);
    hipLaunchKernelGGL(knz_xf_prepare_kernel, dim3(1), dim3(64), 0, st, c, x.out_ptr, x.ok);
    // the stage kernels take the capacity from the stride: make it the caller's dst length exactly
    x.stride = cap;
    int rc = run_stage(h, x, (uint32_t)type1, forward, st);
    if (rc) return rc;
    int32_t ok = 0; uint32_t olen = 0;
    HIP_OK(hipMemcpyAsync(&ok, x.ok, 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(&olen, x.out_len, 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    if (ok == 0) return forward ? KNZ_SKIP : knz_set_error(h, KNZ_ERR_PROCESS_BLOCK, "inverse transform failed");
    if (ok < 0) return forward ? KNZ_SKIP : knz_set_error(h, -ok, "inverse transform failed");
    if (olen > cap) return knz_set_error(h, KNZ_ERR_WRITE_FILE, "destination buffer too small");
    uint64_t optr = 0;
    // (on the handle's own stream: a copy on the NULL stream would be ordered against the blocking streams of every other handle of the process)
    HIP_OK(hipMemcpyAsync(&optr, x.out_ptr, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipMemcpyAsync(dst, (const void*)optr, olen, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    *out_n = olen;
    return KNZ_OK;
}

extern "C" int knz_transform_forward(void* handle, uint64_t type1, const uint8_t* src, uint32_t n, uint8_t* dst, uint32_t cap, uint32_t* out_n) {
    return transform_single(handle, type1, true, src, n, dst, cap, out_n);
}

extern "C" int knz_transform_inverse(void* handle, uint64_t type1, const uint8_t* src, uint32_t n, uint8_t* dst, uint32_t cap, uint32_t* out_n) {
    return transform_single(handle, type1, false, src, n, dst, cap, out_n);
}

extern "C" int knz_entropy_encode(void* handle, uint32_t type, const uint8_t* src, uint32_t n, uint8_t* bits, uint64_t cap_bytes, uint64_t* out_bits) {
    Handle* h = lane0((Handle*)handle);
    if (!h || (!src && n) || !bits || !out_bits) return KNZ_ERR_MISSING_PARAM;
    DeviceGuard dg(h);
    if (!entropy_on_device(type)) return knz_set_error(h, KNZ_ERR_INVALID_CODEC, "entropy codec has no device implementation in this build");
    *out_bits = 0;
    if (n == 0) return KNZ_OK;                 // HuffmanEncoder.Write(len 0) writes nothing (:395-397)
    if (n > (1u << 30)) return knz_set_error(h, KNZ_ERR_BLOCK_SIZE, "Invalid block size parameter (max is 1<<30)");   // FPAQCodec.go:128-130 and friends
    hipStream_t st = host_call_stream(h);
    knz_cfg saved = h->cfg;
    h->cfg.entropy = type; h->cfg.transform = 0; h->cfg.checksum_bits = 0;
    h->cfg.block_size = std::max<uint32_t>(1024, (n + 15) & ~15u);
    const uint64_t ocap = (uint64_t)n * 2 + 262144;       // rANS order 1 spends up to 110 KB of headers per 4 MiB chunk
    int rc = KNZ_OK;
    if (h->stage_in.reserve((uint64_t)n + 64) || h->stage_out.reserve(ocap + 64)) rc = knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
    uint64_t written = 0;
    if (!rc) {
        hipMemcpyAsync(h->stage_in.p, src, n, hipMemcpyHostToDevice, st);
        EncodeBatch eb = EncodeBatch::payload(h->stage_in.as<uint8_t>(), n, h->stage_out.as<uint8_t>(), ocap);
        rc = encode_batch(h, eb, st);
        if (!rc) written = h->pinned_rows.as<Handle::ResultRow>()[0].written;       // (the batch's result rows are on the host already)
    }
    h->cfg = saved;
    if (rc) return rc;
    const uint64_t nb = (written + 7) >> 3;
    if (nb > cap_bytes) return knz_set_error(h, KNZ_ERR_WRITE_FILE, "destination buffer too small");
    HIP_OK(hipMemcpyAsync(bits, h->stage_out.p, nb, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    *out_bits = written;
    return KNZ_OK;
}

extern "C" int knz_entropy_decode(void* handle, uint32_t type, const uint8_t* bits, uint64_t n_bytes, uint8_t* dst, uint32_t n, uint64_t* used_bits) {
    Handle* h = lane0((Handle*)handle);
    if (!h || (!bits && n_bytes) || (!dst && n)) return KNZ_ERR_MISSING_PARAM;
    DeviceGuard dg(h);
    if (!entropy_on_device(type)) return knz_set_error(h, KNZ_ERR_INVALID_CODEC, "entropy codec has no device implementation in this build");
    if (used_bits) *used_bits = 0;
    if (n == 0) return KNZ_OK;
    hipStream_t st = host_call_stream(h);
    uint64_t padded = 0;
    int rc = dec_stage_payloads(h, {Payload{bits, n_bytes}}, n, padded, st);
    if (rc) return rc;
    knz_cfg oc = h->cfg;                                   // a bare EntropyDecoder: one payload of n bytes, no block header, no transform, no checksum
    oc.entropy = type; oc.transform = 0; oc.checksum_bits = 0; oc.block_size = std::max<uint32_t>(1024, n);
    DecodeBatch db(oc, h->stage_in.as<uint8_t>(), padded, h->stage_out.as<uint8_t>(), n);
    db.unframed(1, n); db.payload_only = 1; db.given_len = n;
    rc = decode_batch(h, db, st);
    if (rc) return rc;
    HIP_OK(hipMemcpyAsync(dst, h->stage_out.p, n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (used_bits) *used_bits = db.end_bit[0];
    return KNZ_OK;
}
