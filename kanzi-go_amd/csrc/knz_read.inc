// knz_dev_read_many / knz_dev_read (included by knz_gpu.hip): K byte reads (source, offset, length) -> K destinations of any alignment. The plan is made
// here, in O(R log R): every read's block interval, the distinct (source, block) pairs as the entry list of ONE decompress_many_once, one entry
// {from = b, to = b + 1} each, so that a read's result depends on nothing but its own window. The batch's tail gathers instead of placing (read.hip).
// The table of reads goes up and comes back as one pinned copy each.

struct ReadGather {
    const knz_stream* entries;       // the entry list of the call (status: refused before the batch, e.g. by the hint check)
    ReadRow* rows; uint32_t R;       // pinned: rows, then the entries' rows, then the ids of the long reads
    uint32_t E, n_long;
    bool ran = false;                // the kernels have filled the rows (else no block was decoded: the host fills them)
};

static size_t read_table_bytes(uint32_t R, uint32_t E, uint32_t nLong) { return sizeof(ReadRow) * (size_t)R + sizeof(ReadEntry) * (size_t)E + 4 * (size_t)nLong; }

// the entries' rows of a gather or find tail, from what the last pass of the batch left
static void read_fill_entries(ReadEntry* ent, const knz_stream* entries, const ManyBatchView& v, int n) {
    for (int e = 0; e < n; e++) { ent[e].blk = KNZ_READ_NO_BLOCK; ent[e].status = entries[e].status ? entries[e].status : v.status[e]; }
    for (int i = 0; i < v.A; i++) {
        const ManyStream& m = v.tab[i];
        ReadEntry& en = ent[v.active[i]];
        en.status = m.status;                                             // (the walk's code: damaged framing in front of the block)
        if (m.status == 0 && m.nblocks != 0) en.blk = m.first_block;     // (no blocks: the stream ends in front of this one)
    }
}

// the tail of decompress_many_once for this call: the decoded blocks of the last pass lie at stage_out + ostride * b
static int read_gather_tail(Handle* h, ReadGather& rd, const ManyBatchView& v, const knz_cfg& sc, int n, hipStream_t st) {
    ReadEntry* ent = (ReadEntry*)(rd.rows + rd.R);
    read_fill_entries(ent, rd.entries, v, n);
    const size_t bytes = read_table_bytes(rd.R, rd.E, rd.n_long);
    if (h->read_tab.reserve(bytes) || h->read_base.reserve(8 * ((size_t)rd.R + 1))) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
    HIP_OK(hipMemcpyAsync(h->read_tab.p, rd.rows, bytes, hipMemcpyHostToDevice, st));
    ReadArgs a;
    a.reads = h->read_tab.as<ReadRow>(); a.R = rd.R; a.ent = (const ReadEntry*)(a.reads + rd.R); a.long_ids = (const uint32_t*)(a.ent + rd.E); a.n_long = rd.n_long;
    a.blk_len = h->blk_len.as<uint32_t>(); a.blk_status = h->blk_status.as<int32_t>(); a.block_size = sc.block_size;
    a.base = h->read_base.as<uint64_t>(); a.stage = h->stage_out.as<uint8_t>(); a.stride = v.ostride;
    uint64_t bound = 0;                                                   // chunks the reads can come to: sizes the gather's grid without a trip to the host
    for (uint32_t k = 0; k < rd.R; k++) bound += std::min<uint64_t>(rd.rows[k].length, (uint64_t)rd.rows[k].count * sc.block_size) / 16 + 2;
    KNZ_LAUNCH_PROBED(knz_read_plan_kernel, dim3((rd.R + 255) / 256), dim3(256), 0, st, a, 0u);
    if (rd.n_long) KNZ_LAUNCH_PROBED(knz_read_plan_kernel, dim3((rd.n_long + 3) / 4), dim3(256), 0, st, a, 1u);
    KNZ_LAUNCH_PROBED(knz_read_scan_kernel, dim3(1), dim3(KNZ_READ_SCAN_THREADS), 0, st, a);
    KNZ_LAUNCH_PROBED(knz_read_gather_kernel, dim3((unsigned)std::min<uint64_t>((bound + 255) / 256, 1u << 14)), dim3(256), 0, st, a);
    HIP_OK(hipMemcpyAsync(rd.rows, h->read_tab.p, sizeof(ReadRow) * (size_t)rd.R, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    rd.ran = true;
    return KNZ_OK;
}

// n_blocks (counted): the source's blocks, where a framing walk has counted them (knz_find.inc): no entry is made for a block behind them. walk_err: that walk's
// code where it met damaged framing: n_blocks then counts the frames in front of the damage and the one it could not read
struct ReadSource { const void* d_src; uint64_t n; const knz_block_pos* pos; uint32_t n_pos, first_bit; int32_t status; uint32_t n_blocks; bool counted; int32_t walk_err; };

// The plan the byte reads and the find calls share: windows (source, offset, length) -> per window its span of blocks, the distinct (source, block)
// pairs of all of them, sorted, and one entry {b, b + 1} of the many-streams batch per pair, hinted and checked.
struct ReadWindow { uint32_t source; uint64_t offset, length; bool live; };     // live: not refused, length != 0
struct ReadPlan {
    struct Span { uint64_t key; uint32_t count; };                       // key: source << 32 | first block (ids from 1)
    std::vector<Span> spans;
    std::vector<uint64_t> keys;                                           // the distinct (source, block) pairs, sorted
    uint32_t n_long = 0;                                                  // windows over more than KNZ_READ_LONG entries
    std::vector<knz_stream> es;
    std::vector<knz_block_range> rg;
    std::vector<uint32_t> fb;
    uint32_t first(int k) const { return (uint32_t)(std::lower_bound(keys.begin(), keys.end(), spans[k].key) - keys.begin()); }
};

static int read_plan_spans(Handle* h, const ReadSource* src, const ReadWindow* win, int n, uint64_t bs, ReadPlan& p) {
    p.spans.assign(n, {0, 0});
    std::vector<int> order;
    for (int k = 0; k < n; k++) {
        const ReadWindow& r = win[k];
        if (!r.live) continue;
        // a stream of n bytes holds fewer than n / 3 + 2 blocks (the walkers' bound): what lies behind is no block, whatever the length says
        const ReadSource& s = src[r.source];
        const uint64_t last = s.counted ? s.n_blocks : std::min<uint64_t>(s.n / 3 + 1, (uint64_t)1 << 24) + 1;
        const uint64_t b0 = r.offset / bs + 1, b1 = std::min((r.offset + r.length - 1) / bs + 1, last);
        if (b0 > b1) continue;
        p.spans[k] = {(uint64_t)r.source << 32 | b0, (uint32_t)(b1 - b0 + 1)};
        order.push_back(k);
        if (p.spans[k].count > KNZ_READ_LONG) p.n_long++;
    }
    std::sort(order.begin(), order.end(), [&](int x, int y) { return p.spans[x].key < p.spans[y].key; });
    uint64_t next = 0;
    for (int k : order) {
        const uint64_t lo = std::max(p.spans[k].key, next), hi = p.spans[k].key + p.spans[k].count;     // (a key behind `next` of another source is larger than it)
        for (uint64_t key = lo; key < hi; key++) p.keys.push_back(key);
        next = std::max(next, hi);
        if (p.keys.size() >= ((size_t)1 << 30)) return knz_set_error(h, KNZ_ERR_BLOCK_SIZE, "too many blocks in one call");
    }
    return KNZ_OK;
}

static void read_plan_entries(Handle* h, const ReadSource* src, ReadPlan& p) {
    const uint32_t E = (uint32_t)p.keys.size();
    p.es.resize(E); p.rg.resize(E); p.fb.resize(E);
    for (uint32_t e = 0; e < E; e++) {
        const ReadSource& s = src[p.keys[e] >> 32];
        const uint32_t b = (uint32_t)p.keys[e];
        memset(&p.es[e], 0, sizeof(knz_stream));
        p.es[e].d_src = s.d_src; p.es[e].n = s.n; p.es[e].dst_cap = ~(uint64_t)0;
        p.rg[e].from_block = b; p.rg[e].to_block = b + 1; p.rg[e].from_bit = 0;
        p.fb[e] = s.first_bit;
        if (s.pos && b <= s.n_pos) {
            p.rg[e].from_bit = s.pos[b - 1].bit;
            if (p.rg[e].from_bit == 0) p.es[e].status = knz_set_error(h, KNZ_ERR_INVALID_PARAM, "hint lies outside the stream's blocks");
        }
        if (!p.es[e].status) p.es[e].status = check_block_range(h, p.rg[e], s.n, s.first_bit);
    }
}

// reads [0, n) of one half: 0 with every read's result set, or a code with none of them touched
static int read_many_once(Handle* h, const ReadSource* src, knz_read* reads, int n, const knz_cfg& sc, hipStream_t st, uint64_t& entered) {
    const uint64_t bs = sc.block_size;
    std::vector<ReadWindow> win(n);
    for (int k = 0; k < n; k++) win[k] = {reads[k].source, reads[k].offset, reads[k].length, reads[k].status == 0 && reads[k].length != 0};
    ReadPlan plan;
    const int prc = read_plan_spans(h, src, win.data(), n, bs, plan);
    if (prc) return prc;
    const std::vector<ReadPlan::Span>& spans = plan.spans;
    const std::vector<uint64_t>& keys = plan.keys;
    uint32_t nLong = plan.n_long;
    const uint32_t E = (uint32_t)keys.size(), R = (uint32_t)n;
    if (h->read_pinned.reserve(read_table_bytes(R, E, nLong))) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "pinned host allocation failed");
    ReadGather rd;
    rd.rows = h->read_pinned.as<ReadRow>(); rd.R = R; rd.E = E; rd.n_long = nLong;
    uint32_t* longIds = (uint32_t*)((ReadEntry*)(rd.rows + R) + E);
    nLong = 0;
    for (int k = 0; k < n; k++) {
        ReadRow& w = rd.rows[k];
        memset(&w, 0, sizeof(w));
        w.dst = (uint64_t)reads[k].d_dst; w.length = reads[k].length; w.status = reads[k].status;
        w.count = spans[k].count; w.off0 = (uint32_t)(reads[k].offset % bs);
        if (w.count) w.first = plan.first(k);
        if (w.count > KNZ_READ_LONG) longIds[nLong++] = (uint32_t)k;
    }
    read_plan_entries(h, src, plan);
    std::vector<knz_stream>& es = plan.es;
    rd.entries = es.data();
    if (E) {
        const int rc = decompress_many_once(h, es.data(), plan.fb.data(), plan.rg.data(), sc, (int)E, st, entered, &rd);
        if (rc) return rc;
    }
    for (int k = 0; k < n; k++) {
        const ReadRow& w = rd.rows[k];
        if (reads[k].status) continue;
        if (rd.ran) { reads[k].status = w.status; reads[k].out_bytes = w.status ? 0 : w.out; continue; }
        for (uint32_t j = 0; j < w.count && !reads[k].status; j++) reads[k].status = es[w.first + j].status;      // (no block was decoded: codes or nothing)
    }
    return KNZ_OK;
}

// the sources of a read or find call: pointer checks, every header parsed as knz_dev_decompress_many parses them (msc: the first parsable one's parameters, have:
// there is one), each source's status set
static int read_parse_sources(Handle* h, knz_source* sources, int S, hipStream_t st, knz_cfg& msc, std::vector<ReadSource>& src, bool& have) {
    std::vector<knz_stream> heads((size_t)S);
    for (int s = 0; s < S; s++) {
        memset(&heads[s], 0, sizeof(knz_stream));
        heads[s].d_src = sources[s].d_src; heads[s].n = sources[s].n;
        heads[s].status = !sources[s].d_src ? KNZ_ERR_MISSING_PARAM : (((uintptr_t)sources[s].d_src & 3) ? KNZ_ERR_INVALID_PARAM : 0);
    }
    std::vector<uint32_t> firstBit((size_t)S, 0);
    if (S) {
        const int hrc = many_parse_heads(h, heads.data(), S, st, msc, firstBit, have);
        if (hrc == KNZ_ERR_CREATE_DECOMPRESSOR) { for (int s = 0; s < S; s++) if (!heads[s].status) heads[s].status = hrc; }
        else if (hrc) return hrc;
    }
    src.resize((size_t)S);
    for (int s = 0; s < S; s++) {
        sources[s].status = heads[s].status;
        src[s] = {sources[s].d_src, sources[s].n, sources[s].n_pos ? sources[s].pos : nullptr, sources[s].n_pos, firstBit[s], heads[s].status, 0, false, 0};
    }
    return KNZ_OK;
}

extern "C" int knz_dev_read_many(void* handle, knz_source* sources, int n_sources, knz_read* reads, int n_reads, void* hip_stream) {
    if (!handle) return KNZ_ERR_MISSING_PARAM;
    if (n_reads <= 0) return KNZ_OK;
    if (!reads || !sources) return KNZ_ERR_MISSING_PARAM;
    Handle* top = (Handle*)handle;
    Handle* h = lane_of_pointer(top, reads[0].d_dst);
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
    for (int k = 0; k < n_reads; k++) {
        knz_read& r = reads[k];
        r.out_bytes = 0; r.status = 0; r.reserved = 0; r.reserved2 = 0;
        if (r.source >= (uint32_t)S || r.offset + r.length < r.offset) { r.status = KNZ_ERR_INVALID_PARAM; continue; }
        if (!r.d_dst && r.length) { r.status = KNZ_ERR_MISSING_PARAM; continue; }
        if (src[r.source].status) { r.status = src[r.source].status; continue; }
        hipPointerAttribute_t at;
        if (top->multi && r.length) {
            if (hipPointerGetAttributes(&at, r.d_dst) == hipSuccess) { if (at.device != h->device) r.status = KNZ_ERR_INVALID_PARAM; }
            else (void)hipGetLastError();
        }
    }
    uint64_t entered = 0;
    if (have)
        split_retry(h, 0, n_reads, true, &st, [&](int lo, int cnt) { return read_many_once(h, src.data(), reads + lo, cnt, msc, st, entered); },
                    [&](int lo, int cnt, int rc) { for (int k = lo; k < lo + cnt; k++) if (reads[k].status == 0) reads[k].status = rc; });
    h->dec_blocks = entered;
    for (int k = 0; k < n_reads; k++)
        if (reads[k].status) return knz_set_error(h, reads[k].status, "a read of the call failed (see its status)");
    return KNZ_OK;
}

extern "C" int knz_dev_read(void* handle, const void* d_src, uint64_t n_bytes, uint64_t offset, uint64_t length, void* d_dst, uint64_t* out_bytes, void* hip_stream) {
    if (!handle || !out_bytes) return KNZ_ERR_MISSING_PARAM;
    knz_source s;
    memset(&s, 0, sizeof(s));
    s.d_src = d_src; s.n = n_bytes;
    knz_read r;
    memset(&r, 0, sizeof(r));
    r.offset = offset; r.length = length; r.d_dst = d_dst;
    const int rc = knz_dev_read_many(handle, &s, 1, &r, 1, hip_stream);
    *out_bytes = r.out_bytes;
    return rc;
}
