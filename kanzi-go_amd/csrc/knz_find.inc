// knz_dev_find_many / knz_dev_find (included by knz_gpu.hip): Q queries (source, window, byte string) -> the decoded offsets at which the string starts.
// The plan is knz_read.inc's, over the queries' extended reads (offset, length + pattern_len - 1): the distinct (source, block) pairs as the entry list of
// ONE decompress_many_once, whose tail searches the decoded blocks where they lie (find.hip) instead of placing or gathering them. What is new here: the
// sources' blocks are counted first (one framing walk per queried source), so that a window "to the end" makes no entry for a block that does not exist.
// The table of queries goes up with the patterns behind it and comes back as one pinned copy each.

struct FindScan {
    const knz_stream* entries;       // the entry list of the call (status: refused before the batch, e.g. by the hint check)
    FindRow* rows; uint32_t Q;       // pinned: rows, then the entries' rows, then the patterns
    uint32_t E, pat_bytes;
    uint32_t tile, max_tiles;        // start positions a tile ; tiles the queries can come to: sizes the tile tables and the grids without a trip to the host
    bool any_cap = false;            // some query wants offsets, not only their number
    bool ran = false;                // the kernels have filled the rows (else no block was decoded: the host fills them)
};

static size_t find_table_bytes(uint32_t Q, uint32_t E, uint32_t P) { return sizeof(FindRow) * (size_t)Q + sizeof(ReadEntry) * (size_t)E + (size_t)P; }

// the tail of decompress_many_once for this call: the decoded blocks of the last pass lie at stage_out + ostride * b
static int find_tail(Handle* h, FindScan& fd, const ManyBatchView& v, const knz_cfg& sc, int n, hipStream_t st) {
    ReadEntry* ent = (ReadEntry*)(fd.rows + fd.Q);
    read_fill_entries(ent, fd.entries, v, n);
    const size_t bytes = find_table_bytes(fd.Q, fd.E, fd.pat_bytes);
    const uint32_t wpt = fd.tile / 64;
    if (h->read_tab.reserve(bytes) || h->read_base.reserve(8 * ((size_t)fd.Q + 1)) || h->find_cnt.reserve(8 * ((size_t)fd.max_tiles + 1)) ||
        h->find_bits.reserve(8 * (size_t)wpt * fd.max_tiles))
        return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
    HIP_OK(hipMemcpyAsync(h->read_tab.p, fd.rows, bytes, hipMemcpyHostToDevice, st));
    FindArgs a;
    a.rows = h->read_tab.as<FindRow>();
    a.rd.reads = nullptr; a.rd.R = fd.Q; a.rd.ent = (const ReadEntry*)(a.rows + fd.Q); a.rd.long_ids = nullptr; a.rd.n_long = 0;
    a.rd.blk_len = h->blk_len.as<uint32_t>(); a.rd.blk_status = h->blk_status.as<int32_t>(); a.rd.block_size = sc.block_size;
    a.rd.base = h->read_base.as<uint64_t>(); a.rd.stage = h->stage_out.as<uint8_t>(); a.rd.stride = v.ostride;
    a.pats = (const uint8_t*)(a.rd.ent + fd.E);
    a.tile = fd.tile; a.max_tiles = fd.max_tiles; a.cnt = h->find_cnt.as<uint64_t>(); a.bits = h->find_bits.as<uint64_t>();
    ReadArgs tiles = a.rd;                                                // the scan of the tiles' hits: knz_read_scan_kernel over cnt
    tiles.R = fd.max_tiles; tiles.base = a.cnt;
    const unsigned grid = std::min<uint32_t>(fd.max_tiles, 1u << 16);
    HIP_OK(hipMemsetAsync(a.cnt, 0, 8 * ((size_t)fd.max_tiles + 1), st));     // (tiles behind the last one of the call: no hits)
    KNZ_LAUNCH_PROBED(knz_find_plan_kernel, dim3((fd.Q + 3) / 4), dim3(256), 0, st, a);
    KNZ_LAUNCH_PROBED(knz_read_scan_kernel, dim3(1), dim3(KNZ_READ_SCAN_THREADS), 0, st, a.rd);
    KNZ_LAUNCH_PROBED(knz_find_match_kernel, dim3(grid), dim3(KNZ_FIND_THREADS), 0, st, a);
    KNZ_LAUNCH_PROBED(knz_read_scan_kernel, dim3(1), dim3(KNZ_READ_SCAN_THREADS), 0, st, tiles);
    KNZ_LAUNCH_PROBED(knz_find_finish_kernel, dim3((fd.Q + 255) / 256), dim3(256), 0, st, a);
    if (fd.any_cap) KNZ_LAUNCH_PROBED(knz_find_fill_kernel, dim3(grid), dim3(KNZ_FIND_THREADS), 0, st, a);
    HIP_OK(hipMemcpyAsync(fd.rows, h->read_tab.p, sizeof(FindRow) * (size_t)fd.Q, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    fd.ran = true;
    return KNZ_OK;
}

static bool find_live(const knz_find& f) { return f.status == 0 && f.length != 0; }

// Every source that a live query names gets its block count: one launch of the index's walk (knz_dec_walk_range_kernel) per source, from the header or
// the last hinted frame to the last block a query asks for, all results in one pinned copy. A walk that meets damaged framing counts the frames in
// front of it and one more: that block's entry takes the walk's code in the batch, and with it the queries that reach it.
static int find_count_blocks(Handle* h, std::vector<ReadSource>& src, const knz_find* finds, int n, uint64_t bs, hipStream_t st) {
    const size_t S = src.size();
    const uint64_t END = ~(uint64_t)0;
    std::vector<uint64_t> need(S, 0);                                     // the last block (ids from 1) some query asks for ; END: through the last one
    for (int k = 0; k < n; k++) {
        const knz_find& f = finds[k];
        if (!find_live(f)) continue;
        const uint64_t span = f.length == KNZ_LENGTH_END ? END : f.length - 1 + (f.pattern_len - 1);
        const uint64_t b1 = (span == END || f.offset + span < f.offset) ? END : (f.offset + span) / bs + 1;
        need[f.source] = std::max(need[f.source], b1);
    }
    struct Walk { size_t s; uint64_t first_id; };
    std::vector<Walk> walks;
    std::vector<WalkRangeArgs> args;
    for (size_t s = 0; s < S; s++) {
        ReadSource& r = src[s];
        if (need[s] == 0 || r.status != 0) continue;
        if (r.pos && need[s] <= r.n_pos) { r.n_blocks = r.n_pos; r.counted = true; continue; }      // (the hints name every block that is asked for: they are a caller's word, as for reads)
        const uint32_t bound = (uint32_t)std::min<uint64_t>(r.n / 3 + 1, 1u << 24);                  // (dec_walk_framing's: 8 framing + 16 payload bits a block at least)
        WalkRangeArgs wr;
        wr.stream = (const uint8_t*)r.d_src; wr.nbytes = r.n; wr.first_bit = r.first_bit; wr.first_id = 1; wr.hinted = 0;
        const uint64_t hint = r.pos ? r.pos[r.n_pos - 1].bit : 0;
        if (hint != 0 && hint < 8 * r.n && hint >= r.first_bit) { wr.first_bit = hint; wr.first_id = r.n_pos; wr.hinted = 1; }
        wr.from = wr.first_id; wr.to = need[s] > bound ? END : need[s] + 1;
        wr.max_blocks = bound; wr.cap = 0; wr.frames = 1; wr.stride = 2; wr.blk_bit = nullptr; wr.blk_bits = nullptr; wr.result = nullptr;
        walks.push_back({s, wr.first_id});
        args.push_back(wr);
    }
    if (walks.empty()) return KNZ_OK;
    const size_t bytes = 8 * 4 * walks.size();
    if (h->blk_dst_bit.reserve(bytes)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
    if (h->pinned_rows.reserve(bytes)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "pinned host allocation failed");
    for (size_t w = 0; w < walks.size(); w++) {
        args[w].result = h->blk_dst_bit.as<uint64_t>() + 4 * w;
        hipLaunchKernelGGL(knz_dec_walk_range_kernel, dim3(1), dim3(1), 0, st, args[w]);
    }
    const uint64_t* res = h->pinned_rows.as<uint64_t>();
    HIP_OK(hipMemcpyAsync(h->pinned_rows.p, h->blk_dst_bit.p, bytes, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    for (size_t w = 0; w < walks.size(); w++) {
        ReadSource& r = src[walks[w].s];
        r.n_blocks = (uint32_t)std::min<uint64_t>(walks[w].first_id - 1 + res[4 * w] + (res[4 * w + 1] ? 1 : 0), ((uint64_t)1 << 24) + 1);
        r.counted = true; r.walk_err = (int32_t)res[4 * w + 1];
    }
    return KNZ_OK;
}

// queries [0, n) of one half: 0 with every query's result set, or a code with none of them touched
static int find_many_once(Handle* h, const ReadSource* src, knz_find* finds, int n, const knz_cfg& sc, uint32_t tile, hipStream_t st, uint64_t& entered) {
    const uint64_t bs = sc.block_size;
    std::vector<ReadWindow> win(n);
    std::vector<uint64_t> len(n, 0);                                      // the windows' lengths, clamped to the sources' blocks
    uint32_t P = 0;
    for (int k = 0; k < n; k++) {
        const knz_find& f = finds[k];
        win[k] = {f.source, f.offset, 0, false};
        if (!find_live(f)) continue;
        const uint64_t total = (uint64_t)src[f.source].n_blocks * bs;    // (counted: find_count_blocks has seen every source of a live query)
        if (f.offset >= total) { finds[k].status = src[f.source].walk_err; continue; }      // (behind the last block ; behind damaged framing: the walk's code, as a read there gets it)
        len[k] = std::min(f.length, total - f.offset);                    // (KNZ_LENGTH_END is the largest length)
        win[k].length = len[k] + f.pattern_len - 1; win[k].live = true;
        P += f.pattern_len;
    }
    ReadPlan plan;
    const int prc = read_plan_spans(h, src, win.data(), n, bs, plan);
    if (prc) return prc;
    const uint32_t E = (uint32_t)plan.keys.size(), Q = (uint32_t)n;
    if (h->read_pinned.reserve(find_table_bytes(Q, E, P))) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "pinned host allocation failed");
    FindScan fd;
    fd.rows = h->read_pinned.as<FindRow>(); fd.Q = Q; fd.E = E; fd.pat_bytes = P; fd.tile = tile;
    uint8_t* pats = (uint8_t*)((ReadEntry*)(fd.rows + Q) + E);
    uint64_t tiles = 0;
    P = 0;
    for (int k = 0; k < n; k++) {
        const knz_find& f = finds[k];
        FindRow& w = fd.rows[k];
        memset(&w, 0, sizeof(w));
        w.hits = (uint64_t)f.d_hits; w.cap = f.hits_cap; w.offset = f.offset; w.length = len[k]; w.status = f.status;
        w.count = plan.spans[k].count; w.off0 = (uint32_t)(f.offset % bs); w.pat_len = 1;
        if (!w.count) continue;
        w.first = plan.first(k);
        w.pat = P; w.pat_len = f.pattern_len;
        memcpy(pats + P, f.pattern, f.pattern_len);
        P += f.pattern_len;
        tiles += std::min<uint64_t>(len[k], (uint64_t)w.count * bs) / tile + 1;
        fd.any_cap = fd.any_cap || f.hits_cap != 0;
    }
    if (tiles >= ((uint64_t)1 << 30)) return knz_set_error(h, KNZ_ERR_BLOCK_SIZE, "too many tiles in one call");
    fd.max_tiles = (uint32_t)tiles;
    read_plan_entries(h, src, plan);
    fd.entries = plan.es.data();
    if (E) {
        const int rc = decompress_many_once(h, plan.es.data(), plan.fb.data(), plan.rg.data(), sc, (int)E, st, entered, nullptr, &fd);
        if (rc) return rc;
    }
    for (int k = 0; k < n; k++) {
        const FindRow& w = fd.rows[k];
        if (finds[k].status) continue;
        if (fd.ran) { finds[k].status = w.status; finds[k].n_hits = w.status ? 0 : w.n_hits; finds[k].scanned = w.status ? 0 : w.scanned; continue; }
        for (uint32_t j = 0; j < w.count && !finds[k].status; j++) finds[k].status = plan.es[w.first + j].status;      // (no block was decoded: codes or nothing)
    }
    return KNZ_OK;
}

extern "C" int knz_dev_find_many(void* handle, knz_source* sources, int n_sources, knz_find* finds, int n_finds, void* hip_stream) {
    if (!handle) return KNZ_ERR_MISSING_PARAM;
    if (n_finds <= 0) return KNZ_OK;
    if (!finds || !sources) return KNZ_ERR_MISSING_PARAM;
    Handle* top = (Handle*)handle;
    Handle* h = lane_of_pointer(top, finds[0].d_hits);
    if (!h) h = lane0(top);
    DeviceGuard dg(h);
    h->dec_blocks = 0;
    hipStream_t st = dev_call_stream(h, hip_stream);
    const int S = std::max(n_sources, 0);
    knz_cfg msc = h->cfg;
    std::vector<ReadSource> src;
    bool have = false;
    const int src_rc = read_parse_sources(h, sources, S, st, msc, src, have);
    if (src_rc) return src_rc;
    for (int k = 0; k < n_finds; k++) {
        knz_find& f = finds[k];
        f.n_hits = 0; f.scanned = 0; f.status = 0; f.reserved = 0;
        if (f.pattern_len == 0 || f.pattern_len > KNZ_FIND_MAX_PATTERN || f.source >= (uint32_t)S) { f.status = KNZ_ERR_INVALID_PARAM; continue; }
        if ((f.length != KNZ_LENGTH_END && f.offset + f.length < f.offset) || ((uintptr_t)f.d_hits & 7)) { f.status = KNZ_ERR_INVALID_PARAM; continue; }
        if (!f.pattern || (!f.d_hits && f.hits_cap)) { f.status = KNZ_ERR_MISSING_PARAM; continue; }
        if (src[f.source].status) { f.status = src[f.source].status; continue; }
        hipPointerAttribute_t at;
        if (top->multi && f.hits_cap) {
            if (hipPointerGetAttributes(&at, f.d_hits) == hipSuccess) { if (at.device != h->device) f.status = KNZ_ERR_INVALID_PARAM; }
            else (void)hipGetLastError();
        }
    }
    uint32_t tile = KNZ_FIND_TILE;
    if (const char* e = knz_test_switch("KNZ_FIND_TILE")) tile = (uint32_t)std::min(std::max(atoi(e), 256), KNZ_FIND_TILE) & ~255u;   // (tests: tile edges inside small inputs)
    uint64_t entered = 0;
    if (have) {
        const int crc = find_count_blocks(h, src, finds, n_finds, msc.block_size, st);
        if (crc) { for (int k = 0; k < n_finds; k++) if (find_live(finds[k])) finds[k].status = crc; }
        else
            split_retry(h, 0, n_finds, true, &st, [&](int lo, int cnt) { return find_many_once(h, src.data(), finds + lo, cnt, msc, tile, st, entered); },
                        [&](int lo, int cnt, int rc) { for (int k = lo; k < lo + cnt; k++) if (finds[k].status == 0) finds[k].status = rc; });
    }
    h->dec_blocks = entered;
    for (int k = 0; k < n_finds; k++)
        if (finds[k].status) return knz_set_error(h, finds[k].status, "a query of the call failed (see its status)");
    return KNZ_OK;
}

extern "C" int knz_dev_find(void* handle, const void* d_src, uint64_t n_bytes, const void* pattern, uint32_t pattern_len, uint64_t* d_hits, uint64_t hits_cap,
                            uint64_t* n_hits, void* hip_stream) {
    if (!handle || !n_hits) return KNZ_ERR_MISSING_PARAM;
    knz_source s;
    memset(&s, 0, sizeof(s));
    s.d_src = d_src; s.n = n_bytes;
    knz_find f;
    memset(&f, 0, sizeof(f));
    f.pattern = pattern; f.pattern_len = pattern_len; f.length = KNZ_LENGTH_END; f.d_hits = d_hits; f.hits_cap = hits_cap;
    const int rc = knz_dev_find_many(handle, &s, 1, &f, 1, hip_stream);
    *n_hits = f.n_hits;
    return rc;
}
