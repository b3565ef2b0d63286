// knz_dev_compress_many / knz_dev_decompress_many (included by knz_gpu.hip): K independent .knz streams per call, all their blocks in ONE
// encode_batch / decode_batch. The batch runs unframed (block-local streams / decoded blocks at a fixed stride in the handle's staging buffers)
// over a block table the device derives from the table of streams; many.hip assembles the K streams (encode) or places the decoded blocks
// (decode). Launches and copies do not grow with K: the table of streams goes up and comes back as one pinned copy each.

// split_retry's streams form: once(lo, cnt) returns 0 with every stream's result set, or a code with none of them touched. Both halves of a range run,
// what fails for good marks its range, and the caller's stream has run dry before the workspace goes.
template <typename F>
static void many_split_retry(Handle* h, knz_stream* s, int n, hipStream_t st, F once) {
    split_retry(h, 0, n, true, &st, once, [&](int lo, int cnt, int rc) { for (int k = lo; k < lo + cnt; k++) if (s[k].status == 0) s[k].status = rc; });
}

// the lane a call runs on (the one that owns streams[0].d_dst) and, per stream, what can be refused before the device is asked
static Handle* many_begin(void* handle, knz_stream* s, int n, bool compress) {
    Handle* top = (Handle*)handle;
    Handle* h = lane_of_pointer(top, s[0].d_dst);
    if (!h) h = lane0(top);
    for (int k = 0; k < n; k++) {
        s[k].out_bytes = 0; s[k].status = 0; s[k].reserved = 0;
        if (!s[k].d_dst || (!s[k].d_src && (s[k].n || !compress))) { s[k].status = KNZ_ERR_MISSING_PARAM; continue; }
        if (((uintptr_t)s[k].d_dst & 3) || ((uintptr_t)s[k].d_src & (compress ? 15 : 3))) { s[k].status = KNZ_ERR_INVALID_PARAM; continue; }
        hipPointerAttribute_t at;
        if (top->multi) {
            if (hipPointerGetAttributes(&at, s[k].d_dst) == hipSuccess) { if (at.device != h->device) s[k].status = KNZ_ERR_INVALID_PARAM; }
            else (void)hipGetLastError();
        }
    }
    return h;
}

static int many_end(Handle* h, const knz_stream* s, int n) {
    for (int k = 0; k < n; k++)
        if (s[k].status) return knz_set_error(h, s[k].status, s[k].status == KNZ_ERR_WRITE_FILE ? "destination buffer of a stream too small" : "a stream of the call failed (see its status)");
    return KNZ_OK;
}

static unsigned many_copy_y(uint64_t stride) { return (unsigned)std::min<uint64_t>(64, std::max<uint64_t>(1, stride / (256 * 64))); }

static int compress_many_once(Handle* h, knz_stream* s, int n, hipStream_t st) {
    const knz_cfg& cfg = h->cfg;
    const uint64_t bs = cfg.block_size;
    if (h->many_pinned.reserve(sizeof(ManyStream) * (size_t)n)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "pinned host allocation failed");
    ManyStream* tab = h->many_pinned.as<ManyStream>();
    uint64_t nblocks = 0, maxLen = 0;
    for (int k = 0; k < n; k++) {
        ManyStream& m = tab[k];
        memset(&m, 0, sizeof(m));
        m.src = (uint64_t)s[k].d_src; m.n = s[k].n; m.dst = (uint64_t)s[k].d_dst; m.cap = s[k].dst_cap; m.status = s[k].status;
        m.hdr_bits = knz_build_stream_header(cfg, s[k].header_input_size, m.hdr_words);
        if (m.status) continue;
        nblocks += (m.n + bs - 1) / bs;
        maxLen = std::max(maxLen, std::min<uint64_t>(m.n, bs));
    }
    if (nblocks >= (1u << 30)) return knz_set_error(h, KNZ_ERR_BLOCK_SIZE, "too many blocks in one call");
    // block-local streams at a fixed stride, sized by the longest block of the call, not by the block size
    const uint64_t ostride = block_stream_bound(cfg.transform, cfg.entropy, maxLen);
    if (h->many_tab.reserve(sizeof(ManyStream) * (size_t)n) || h->many_blk_stream.reserve(4 * (nblocks + 1)) || h->many_blk_pos.reserve(8 * (nblocks + 1)) ||
        h->stage_out.reserve(ostride * nblocks + 64) || h->total_bits.reserve(64))
        return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
    ManyStream* dtab = h->many_tab.as<ManyStream>();
    HIP_OK(hipMemcpyAsync(dtab, tab, sizeof(ManyStream) * (size_t)n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(knz_many_scan_kernel, dim3(1), dim3(256), 0, st, dtab, (uint32_t)n, bs, 1u, h->total_bits.as<uint32_t>() + 8);
    EncodeBatch eb = EncodeBatch::block_streams(nullptr, 0, h->stage_out.as<uint8_t>(), ostride, nblocks);
    eb.many = {dtab, (uint32_t)n, (uint32_t)nblocks, (uint32_t)maxLen, h->many_blk_stream.as<uint32_t>()};
    int rc = encode_batch(h, eb, st);
    if (rc) return rc;
    ManyAsmArgs a;
    a.streams = dtab; a.K = (uint32_t)n; a.blk_written = h->blk_written.as<uint64_t>(); a.blk_status = h->blk_status.as<int32_t>();
    a.blk_stream = h->many_blk_stream.as<uint32_t>(); a.blk_pos = h->many_blk_pos.as<uint64_t>(); a.stage = h->stage_out.as<uint8_t>(); a.stride = ostride;
    KNZ_LAUNCH_PROBED(knz_many_asm_plan_kernel, dim3(n), dim3(256), 0, st, a);
    if (nblocks) KNZ_LAUNCH_PROBED(knz_many_asm_copy_kernel, dim3((unsigned)nblocks, many_copy_y(ostride)), dim3(256), 0, st, a);
    HIP_OK(hipMemcpyAsync(tab, dtab, sizeof(ManyStream) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    for (int k = 0; k < n; k++) { s[k].status = tab[k].status; s[k].out_bytes = tab[k].status ? 0 : tab[k].out; }
    return KNZ_OK;
}

extern "C" int knz_dev_compress_many(void* handle, knz_stream* streams, int n, void* hip_stream) {
    if (!handle || (!streams && n > 0)) return KNZ_ERR_MISSING_PARAM;
    if (n <= 0) return KNZ_OK;
    Handle* h = many_begin(handle, streams, n, true);
    DeviceGuard dg(h);
    hipStream_t st = dev_call_stream(h, hip_stream);
    many_split_retry(h, streams, n, st, [&](int lo, int cnt) { return compress_many_once(h, streams + lo, cnt, st); });
    return many_end(h, streams, n);
}

// rg == nullptr: every stream whole, staged side by side. Else entry k's range rg[k]: the walkers read the callers' buffers, and only the bytes that hold
// the selected frames are staged (knz_many_stage_range_kernel), so that walk, staging and batch follow the ranges and not the streams.
// entered: the blocks of these entries that went into a decode batch (the first pass: a later one runs fewer of the same).
// What happens to the decoded blocks, at ostride * b in the staging buffer, is the tail's choice: rd == nullptr places them into the entries' destinations ;
// rd: they are gathered into the reads of knz_dev_read_many (knz_read.inc) ; fd: they are searched for the patterns of knz_dev_find_many (knz_find.inc) ; the
// entries' d_dst / dst_cap are then not looked at.
struct ReadGather;
struct FindScan;
struct ManyBatchView {               // what the gather tail sees of the last pass: its entries' rows (host copy) and where the blocks were decoded
    const int* active; int A; const ManyStream* tab; const int32_t* status; uint64_t nblocks, ostride;
};
static int read_gather_tail(Handle* h, ReadGather& rd, const ManyBatchView& v, const knz_cfg& sc, int n, hipStream_t st);
static int find_tail(Handle* h, FindScan& fd, const ManyBatchView& v, const knz_cfg& sc, int n, hipStream_t st);
static int decompress_many_once(Handle* h, knz_stream* s, const uint32_t* firstBit, const knz_block_range* rg, const knz_cfg& sc, int n, hipStream_t st, uint64_t& entered,
                                ReadGather* rd = nullptr, FindScan* fd = nullptr) {
    uint64_t first_pass = 0;
    std::vector<int> active;
    std::vector<int32_t> status(n, 0);
    std::vector<uint64_t> out(n, 0);
    for (int k = 0; k < n; k++) if (s[k].status == 0) active.push_back(k);
    const uint64_t ostride = ((uint64_t)sc.block_size + 63) & ~(uint64_t)63;
    while (!active.empty()) {
        const int A = (int)active.size();
        const size_t tabBytes = sizeof(ManyStream) * (size_t)A, rgBytes = rg ? sizeof(ManyRange) * (size_t)A : 0;
        if (h->many_pinned.reserve(tabBytes + rgBytes)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "pinned host allocation failed");
        ManyStream* tab = h->many_pinned.as<ManyStream>();
        ManyRange* rtab = (ManyRange*)(h->many_pinned.as<uint8_t>() + tabBytes);
        uint64_t staged = 0;
        for (int i = 0; i < A; i++) {
            const knz_stream& c = s[active[i]];
            ManyStream& m = tab[i];
            memset(&m, 0, sizeof(m));
            m.src = (uint64_t)c.d_src; m.n = c.n; m.dst = (uint64_t)c.d_dst; m.cap = c.dst_cap; m.hdr_bits = firstBit[active[i]]; m.stage_off = staged;
            if (!rg) { staged += (c.n + 15) & ~(uint64_t)15; continue; }
            const knz_block_range& r = rg[active[i]];                     // (a range's place in the staging buffer: once the count walk has found its frames)
            ManyRange& g = rtab[i];
            memset(&g, 0, sizeof(g));
            g.from = r.from_block; g.to = r.to_block; g.start_bit = r.from_bit ? r.from_bit : m.hdr_bits; g.start_id = r.from_bit ? r.from_block : 1; g.hinted = r.from_bit ? 1 : 0;
        }
        if (h->many_tab.reserve(tabBytes) || (rg ? h->many_ranges.reserve(rgBytes) : h->stage_in.reserve(staged + 64)) || h->total_bits.reserve(64))
            return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
        ManyStream* dtab = h->many_tab.as<ManyStream>();
        ManyRange* drg = h->many_ranges.as<ManyRange>();
        HIP_OK(hipMemcpyAsync(dtab, tab, tabBytes, hipMemcpyHostToDevice, st));
        ManyWalkArgs w;
        w.streams = dtab; w.K = (uint32_t)A; w.stage = nullptr; w.fill = 0; w.blk_bit = nullptr; w.blk_bits = nullptr; w.blk_stream = nullptr;
        if (!rg) {
            HIP_OK(hipMemsetAsync(h->stage_in.as<uint8_t>() + staged, 0, 64, st));
            uint64_t longest = 0;
            for (int i = 0; i < A; i++) longest = std::max(longest, tab[i].n);
            hipLaunchKernelGGL(knz_many_stage_kernel, dim3(A, many_copy_y(longest)), dim3(256), 0, st, (const ManyStream*)dtab, h->stage_in.as<uint8_t>());
            w.stage = h->stage_in.as<uint8_t>();
            hipLaunchKernelGGL(knz_many_walk_kernel, dim3((A + 63) / 64), dim3(64), 0, st, w);
        } else {
            HIP_OK(hipMemcpyAsync(drg, rtab, rgBytes, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(knz_many_walk_range_kernel, dim3((A + 63) / 64), dim3(64), 0, st, w, drg);
        }
        hipLaunchKernelGGL(knz_many_scan_kernel, dim3(1), dim3(256), 0, st, dtab, (uint32_t)A, (uint64_t)sc.block_size, 0u, h->total_bits.as<uint32_t>() + 8);
        HIP_OK(hipMemcpyAsync(tab, dtab, tabBytes, hipMemcpyDeviceToHost, st));
        if (rg) HIP_OK(hipMemcpyAsync(rtab, drg, rgBytes, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        uint64_t nblocks = 0;
        for (int i = 0; i < A; i++) { status[active[i]] = tab[i].status; nblocks += tab[i].nblocks; }      // (a stream with damaged framing: its status, no blocks)
        if (nblocks == 0) break;
        first_pass = std::max(first_pass, nblocks);
        if (h->blk_dst_bit.reserve(8 * (nblocks + 1)) || h->blk_written.reserve(8 * (nblocks + 1)) || h->many_blk_stream.reserve(4 * (nblocks + 1)) ||
            h->many_blk_pos.reserve(8 * (nblocks + 1)) || h->stage_out.reserve(ostride * nblocks + 64))
            return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
        if (rg) {
            // the bytes that hold every entry's selected frames, side by side: from the 16 bytes its first payload bit lies in to its last payload byte
            uint64_t longest = 0;
            for (int i = 0; i < A; i++) {
                ManyStream& m = tab[i];
                ManyRange& g = rtab[i];
                if (m.status || !m.nblocks) continue;
                if (g.span_lo > g.span_hi || g.span_hi > 8 * m.n) return knz_set_error(h, KNZ_ERR_UNKNOWN, "framing walk left the stream");   // (the walk checks every frame)
                g.src_off = (g.span_lo >> 3) & ~(uint64_t)15; g.len = ((g.span_hi + 7) >> 3) - g.src_off;
                m.stage_off = staged;
                staged += (g.len + 15) & ~(uint64_t)15;
                longest = std::max(longest, g.len);
            }
            if (h->stage_in.reserve(staged + 64)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
            HIP_OK(hipMemcpyAsync(dtab, tab, tabBytes, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(drg, rtab, rgBytes, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemsetAsync(h->stage_in.as<uint8_t>() + staged, 0, 64, st));
            KNZ_LAUNCH_PROBED(knz_many_stage_range_kernel, dim3(A, many_copy_y(longest)), dim3(256), 0, st, (const ManyStream*)dtab, (const ManyRange*)drg, h->stage_in.as<uint8_t>());
        }
        w.fill = 1; w.blk_bit = h->blk_dst_bit.as<uint64_t>(); w.blk_bits = h->blk_written.as<uint64_t>(); w.blk_stream = h->many_blk_stream.as<uint32_t>();
        if (rg) hipLaunchKernelGGL(knz_many_walk_range_kernel, dim3((A + 63) / 64), dim3(64), 0, st, w, drg);
        else hipLaunchKernelGGL(knz_many_walk_kernel, dim3((A + 63) / 64), dim3(64), 0, st, w);
        DecodeBatch db(sc, h->stage_in.as<uint8_t>(), staged, h->stage_out.as<uint8_t>(), ostride * nblocks);
        db.unframed((uint32_t)nblocks, ostride); db.many = true;
        const int rc = decode_batch(h, db, st);
        if (rc && !db.done) {
            // a block was refused before the batch had run to its end: its stream takes the code and leaves, the others go through again
            std::vector<int> next;
            bool any = false;
            for (int i = 0; i < A; i++) {
                const int k = active[i];
                if (status[k]) continue;
                for (uint32_t b = tab[i].first_block; b < tab[i].first_block + tab[i].nblocks && b < db.status.size() && !status[k]; b++) status[k] = db.status[b];
                if (status[k]) any = true; else next.push_back(k);
            }
            if (!any) return rc;                                          // (nothing a stream can be blamed for: workspace, runtime)
            active.swap(next);
            continue;
        }
        if (rd || fd) {
            const ManyBatchView v = {active.data(), A, tab, status.data(), nblocks, ostride};
            const int grc = rd ? read_gather_tail(h, *rd, v, sc, n, st) : find_tail(h, *fd, v, sc, n, st);
            if (grc) return grc;
            break;
        }
        ManyPlaceArgs p;
        p.streams = dtab; p.K = (uint32_t)A; p.blk_len = h->blk_len.as<uint32_t>(); p.blk_status = h->blk_status.as<int32_t>();
        p.blk_stream = h->many_blk_stream.as<uint32_t>(); p.blk_pos = h->many_blk_pos.as<uint64_t>(); p.stage = h->stage_out.as<uint8_t>(); p.stride = ostride;
        p.block_size = sc.block_size;
        KNZ_LAUNCH_PROBED(knz_many_place_plan_kernel, dim3(A), dim3(256), 0, st, p);
        KNZ_LAUNCH_PROBED(knz_many_place_copy_kernel, dim3((unsigned)nblocks, many_copy_y(ostride)), dim3(256), 0, st, p);
        HIP_OK(hipMemcpyAsync(tab, dtab, sizeof(ManyStream) * (size_t)A, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipGetLastError());
        for (int i = 0; i < A; i++) { status[active[i]] = tab[i].status; out[active[i]] = tab[i].status ? 0 : tab[i].out; }
        break;
    }
    for (int k = 0; k < n; k++) if (s[k].status == 0) { s[k].status = status[k]; s[k].out_bytes = out[k]; }
    entered += first_pass;
    return KNZ_OK;
}

// every stream's head: one device-side gather, one copy into pinned memory; the headers are parsed here as knz_dev_decompress parses one. A stream whose
// header does not parse, or that differs from the first one that does, takes its code. KNZ_ERR_CREATE_DECOMPRESSOR: the tables could not be had.
static int many_parse_heads(Handle* h, knz_stream* streams, int n, hipStream_t st, knz_cfg& msc, std::vector<uint32_t>& firstBit, bool& have) {
    const size_t tabBytes = sizeof(ManyStream) * (size_t)n;
    if (h->many_pinned.reserve(tabBytes + 32 * (size_t)n) || h->many_tab.reserve(tabBytes) || h->many_heads.reserve(32 * (size_t)n)) return KNZ_ERR_CREATE_DECOMPRESSOR;
    ManyStream* tab = h->many_pinned.as<ManyStream>();
    uint8_t* heads = h->many_pinned.as<uint8_t>() + tabBytes;
    for (int k = 0; k < n; k++) {
        memset(&tab[k], 0, sizeof(ManyStream));
        tab[k].src = (uint64_t)streams[k].d_src; tab[k].n = streams[k].n; tab[k].status = streams[k].status;
    }
    HIP_OK(hipMemcpyAsync(h->many_tab.p, tab, tabBytes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(knz_many_heads_kernel, dim3((n * 8 + 255) / 256), dim3(256), 0, st, (const ManyStream*)h->many_tab.as<ManyStream>(), (uint32_t)n, h->many_heads.as<uint32_t>());
    HIP_OK(hipMemcpyAsync(heads, h->many_heads.p, 32 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (int k = 0; k < n; k++) {
        if (streams[k].status) continue;
        knz_cfg sc = h->cfg;
        int64_t outputSize = 0;
        const int rc = parse_stream_header(h, heads + 32 * (size_t)k, streams[k].n, sc, outputSize, firstBit[k]);
        if (rc) { streams[k].status = rc; continue; }
        if (!have) { msc = sc; have = true; continue; }
        if (sc.transform != msc.transform || sc.entropy != msc.entropy || sc.block_size != msc.block_size || sc.checksum_bits != msc.checksum_bits)
            streams[k].status = KNZ_ERR_INVALID_PARAM;                    // one batch, one set of codec parameters: the first stream's
    }
    return KNZ_OK;
}

// knz_dev_decompress_many (ranges == nullptr) and knz_dev_decompress_many_range
static int dev_decompress_many(void* handle, knz_stream* streams, const knz_block_range* ranges, int n, void* hip_stream) {
    if (!handle || (!streams && n > 0)) return KNZ_ERR_MISSING_PARAM;
    if (n <= 0) return KNZ_OK;
    Handle* h = many_begin(handle, streams, n, false);
    DeviceGuard dg(h);
    h->dec_blocks = 0;
    hipStream_t st = dev_call_stream(h, hip_stream);
    knz_cfg msc = h->cfg;                                                 // the call's codec parameters (the first stream's) and every first block's bit
    std::vector<uint32_t> firstBit(n, 0);
    bool have = false;
    const int hrc = many_parse_heads(h, streams, n, st, msc, firstBit, have);
    if (hrc == KNZ_ERR_CREATE_DECOMPRESSOR) {
        for (int k = 0; k < n; k++) if (!streams[k].status) streams[k].status = KNZ_ERR_CREATE_DECOMPRESSOR;
        return many_end(h, streams, n);
    }
    if (hrc) return hrc;
    for (int k = 0; k < n && ranges; k++)
        if (streams[k].status == 0) streams[k].status = check_block_range(h, ranges[k], streams[k].n, firstBit[k]);
    uint64_t entered = 0;                                                 // (knz_last_counter 7: over every batch of the call, halves and second passes included)
    if (have)
        many_split_retry(h, streams, n, st, [&](int lo, int cnt) { return decompress_many_once(h, streams + lo, firstBit.data() + lo, ranges ? ranges + lo : nullptr, msc, cnt, st, entered); });
    h->dec_blocks = entered;
    return many_end(h, streams, n);
}

extern "C" int knz_dev_decompress_many(void* handle, knz_stream* streams, int n, void* hip_stream) {
    return dev_decompress_many(handle, streams, nullptr, n, hip_stream);
}

extern "C" int knz_dev_decompress_many_range(void* handle, knz_stream* streams, const knz_block_range* ranges, int n, void* hip_stream) {
    if (!ranges && n > 0) return KNZ_ERR_MISSING_PARAM;
    return dev_decompress_many(handle, streams, ranges, n, hip_stream);
}
