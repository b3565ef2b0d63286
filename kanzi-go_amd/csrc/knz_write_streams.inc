// knz_dev_write_streams (included by knz_gpu.hip): T targets (one source stream, one new stream each) and W writes that name their target. What
// knz_dev_write_many does for one target, write_streams_once does for a list of them with ONE pass of every stage: the heads of the distinct sources (one
// gather, one copy), their framing (write_streams.hip: a count pass and a fill pass over all of them, one synchronisation each), per target the plan of
// knz_write.inc (touched blocks, the writes resolved and swept into visible pieces, the rows of the encode batch, the pieces of the new stream), ONE
// decompress_many_once over the touched existing blocks of all targets (target g's block e at blocks + (slot0 + e) * block_size), ONE launch of
// knz_write_overlay_kernel over all visible pieces, ONE encode batch in the block-streams form (a table of "streams", one per target: its rows side by
// side, only the last of them short), ONE plan launch (a workgroup per target) and ONE copy launch for all outputs. A target that fails leaves the list
// and takes its own code ; nothing of a destination is written before the plan kernel has checked its dst_cap. Synchronisations do not grow with T.

struct WsTarget {                    // a target some write names: what the host has made of it so far, and its results
    int t = 0;                       // its row of targets[]
    std::vector<int> wi;             // its writes: rows of writes[], in index order
    std::vector<knz_write> w;        // ... side by side, as write_resolve and the sweep read them ; their status fields are the results
    int32_t status = 0;
    bool blamed = false;             // the writes at fault carry their codes (else the target's code goes to every write of it)
    uint64_t out_bytes = 0;
};

struct WsKey { uint64_t src, n; bool operator<(const WsKey& k) const { return src != k.src ? src < k.src : n < k.n; } bool operator==(const WsKey& k) const { return src == k.src && n == k.n; } };

struct WsPlan {                      // one target's plan inside a batch
    uint32_t s = 0;                  // its row of the distinct sources
    uint32_t nb = 0, hbits = 0;      // the source's blocks, its first frame's bit
    int64_t outputSize = 0;
    const WsFrame* fr = nullptr;     // the source's frames
    std::vector<uint32_t> T;         // touched existing blocks, ids from 1, sorted
    bool needL = false;
    std::vector<uint64_t> off;       // the writes' resolved offsets
    uint64_t newLen = 0, L = 0;
    int hole = -1;
    uint64_t slot0 = 0, slots = 0;   // its blocks' place in the buffer of decoded blocks: [slot0, slot0 + slots) * block_size
    uint64_t e0 = 0;                 // its first entry of the decode batch
    std::vector<uint32_t> rows;      // the blocks of the encode batch: touched existing ones, then the new ones
    uint64_t row0 = 0, lastLen = 0;  // its first row of the encode batch ; the length of its last row
    uint32_t keep = 0;
    uint64_t grow = 0;
    uint64_t frame_start(uint32_t i) const { return i ? fr[i - 1].bit + fr[i - 1].bits : (uint64_t)hbits; }     // i: block index from 0
    uint64_t frame_end(uint32_t i) const { return fr[i].bit + fr[i].bits; }
};

// outputs whose d_dst[0 .. dst_cap) meets a source of the call (its n_bytes rounded up to 4) or another output's range: KNZ_ERR_INVALID_PARAM
// (splice_mark_overlaps's sweep over the targets some write names)
static void write_streams_mark_overlaps(const knz_write_target* targets, const std::vector<WsTarget>& tg, std::vector<int32_t>& ost) {
    struct Span { uint64_t lo, hi; int out; };                            // out < 0: a source
    std::vector<Span> sp;
    for (size_t g = 0; g < tg.size(); g++) {
        const knz_write_target& t = targets[tg[g].t];
        if (t.d_src && t.n_bytes) sp.push_back({(uint64_t)t.d_src, (uint64_t)t.d_src + ((t.n_bytes + 3) & ~(uint64_t)3), -1});
        if (t.d_dst && t.dst_cap) sp.push_back({(uint64_t)t.d_dst, (uint64_t)t.d_dst + t.dst_cap, (int)g});
    }
    std::sort(sp.begin(), sp.end(), [](const Span& x, const Span& y) { return x.lo < y.lo; });
    uint64_t srcEnd = 0, outEnd = 0;
    int outOwner = -1;                                                    // the output whose range ends at outEnd
    for (const Span& s : sp) {
        if (s.out < 0) {
            if (s.lo < outEnd && !ost[outOwner]) ost[outOwner] = KNZ_ERR_INVALID_PARAM;
            srcEnd = std::max(srcEnd, s.hi);
            continue;
        }
        if (s.lo < srcEnd && !ost[s.out]) ost[s.out] = KNZ_ERR_INVALID_PARAM;
        if (s.lo < outEnd) {
            if (!ost[s.out]) ost[s.out] = KNZ_ERR_INVALID_PARAM;
            if (!ost[outOwner]) ost[outOwner] = KNZ_ERR_INVALID_PARAM;
        }
        if (s.hi > outEnd) { outEnd = s.hi; outOwner = s.out; }
    }
}

// The targets run[0 .. n), none of them refused so far. Returns 0 with every target's results set, or a code that is no target's (workspace, runtime)
// with no byte of a destination written. dec / enc: the blocks that entered the decode batch and the encode batch.
static int write_streams_once(Handle* h, WsTarget* const* run, int n, const knz_write_target* targets, hipStream_t st, uint64_t& dec, uint64_t& enc) {
    const knz_cfg& cfg = h->cfg;
    const uint64_t bs = cfg.block_size;
    h->nprobes = 0;
    if (!h->wr) h->wr.reset(new WriteBufs());
    WriteBufs& wb = *h->wr;
    for (int g = 0; g < n; g++) {
        run[g]->status = 0; run[g]->blamed = false; run[g]->out_bytes = 0;
        for (knz_write& w : run[g]->w) w.status = 0;
    }
    auto fail = [&](int g, int rc, bool blamed) { run[g]->status = rc; run[g]->blamed = blamed; };
    std::vector<WsPlan> plan(n);

    // the distinct sources and their heads: one gather, one copy
    std::vector<WsKey> keys;
    for (int g = 0; g < n; g++) keys.push_back({(uint64_t)targets[run[g]->t].d_src, targets[run[g]->t].n_bytes});
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const uint32_t S = (uint32_t)keys.size();
    std::vector<int32_t> sst(S, 0);
    std::vector<int64_t> ssize(S, 0);
    std::vector<uint32_t> sbit(S, 0);
    knz_cfg sc = cfg;
    {
        const size_t tabBytes = sizeof(ManyStream) * (size_t)S;
        if (h->many_pinned.reserve(tabBytes + 32 * (size_t)S)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "pinned host allocation failed");
        if (h->many_tab.reserve(tabBytes) || h->many_heads.reserve(32 * (size_t)S)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
        ManyStream* tab = h->many_pinned.as<ManyStream>();
        const uint8_t* heads = h->many_pinned.as<uint8_t>() + tabBytes;
        for (uint32_t s = 0; s < S; s++) { memset(&tab[s], 0, sizeof(ManyStream)); tab[s].src = keys[s].src; tab[s].n = keys[s].n; }
        HIP_OK(hipMemcpyAsync(h->many_tab.p, tab, tabBytes, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(knz_many_heads_kernel, dim3((S * 8 + 255) / 256), dim3(256), 0, st, (const ManyStream*)h->many_tab.as<ManyStream>(), S, h->many_heads.as<uint32_t>());
        HIP_OK(hipMemcpyAsync((void*)heads, h->many_heads.p, 32 * (size_t)S, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        bool have = false;
        for (uint32_t s = 0; s < S; s++) {
            knz_cfg c = cfg;
            sst[s] = parse_stream_header(h, heads + 32 * (size_t)s, keys[s].n, c, ssize[s], sbit[s]);
            if (!sst[s] && (c.transform != cfg.transform || c.entropy != cfg.entropy || c.block_size != cfg.block_size || c.checksum_bits != cfg.checksum_bits))
                sst[s] = knz_set_error(h, KNZ_ERR_INVALID_PARAM, "the source stream was not written under the handle's configuration");
            if (!sst[s] && !have) { sc = c; have = true; }
        }
    }

    // the framing of every distinct source, from the header to the end marker: a count pass sizes the rows, a fill pass leaves every block's payload bit and bit count
    std::vector<WsSource> src(S);
    std::vector<WsFrame> frames;
    {
        const size_t srcBytes = sizeof(WsSource) * (size_t)S;
        if (wb.pinned.reserve(srcBytes)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "pinned host allocation failed");
        if (wb.tab.reserve(srcBytes + 64)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
        for (uint32_t s = 0; s < S; s++) { memset(&src[s], 0, sizeof(WsSource)); src[s].src = keys[s].src; src[s].n = keys[s].n; src[s].first_bit = sbit[s]; src[s].status = sst[s]; }
        memcpy(wb.pinned.p, src.data(), srcBytes);
        HIP_OK(hipMemcpyAsync(wb.tab.p, wb.pinned.p, srcBytes, hipMemcpyHostToDevice, st));
        WsWalkArgs wa;
        wa.sources = wb.tab.as<WsSource>(); wa.S = S; wa.fill = 0; wa.frames = nullptr;
        KNZ_LAUNCH_PROBED(knz_ws_walk_kernel, dim3((S + 63) / 64), dim3(64), 0, st, wa);
        HIP_OK(hipMemcpyAsync(wb.pinned.p, wb.tab.p, srcBytes, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipGetLastError());
        memcpy(src.data(), wb.pinned.p, srcBytes);
        uint64_t nframes = 0;
        for (uint32_t s = 0; s < S; s++) {
            if (src[s].status || src[s].err) { src[s].count = 0; if (!sst[s]) sst[s] = knz_set_error(h, src[s].err, "invalid block framing in stream"); }
            src[s].row_first = nframes;
            nframes += src[s].count;
        }
        if (nframes) {
            const size_t frBytes = sizeof(WsFrame) * (size_t)nframes;
            if (wb.pinned.reserve(srcBytes + frBytes)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "pinned host allocation failed");
            if (wb.tab.reserve(srcBytes + frBytes + 64)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
            memcpy(wb.pinned.p, src.data(), srcBytes);
            HIP_OK(hipMemcpyAsync(wb.tab.p, wb.pinned.p, srcBytes, hipMemcpyHostToDevice, st));
            wa.sources = wb.tab.as<WsSource>(); wa.fill = 1; wa.frames = (WsFrame*)(wb.tab.as<uint8_t>() + srcBytes);
            HIP_OK(hipMemsetAsync(wa.frames, 0, frBytes, st));
            KNZ_LAUNCH_PROBED(knz_ws_walk_kernel, dim3((S + 63) / 64), dim3(64), 0, st, wa);
            HIP_OK(hipMemcpyAsync(wb.pinned.as<uint8_t>() + srcBytes, wa.frames, frBytes, hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            HIP_OK(hipGetLastError());
            frames.resize(nframes);
            memcpy(frames.data(), wb.pinned.as<uint8_t>() + srcBytes, frBytes);
        }
    }

    // per target: the existing blocks its writes touch, whether L is needed, its room in the buffer of decoded blocks (knz_write.inc's plan)
    uint64_t slots = 0, E0 = 0;
    for (int g = 0; g < n; g++) {
        WsTarget& tg = *run[g];
        WsPlan& p = plan[g];
        const knz_write_target& t = targets[tg.t];
        p.s = (uint32_t)(std::lower_bound(keys.begin(), keys.end(), WsKey{(uint64_t)t.d_src, t.n_bytes}) - keys.begin());
        if (sst[p.s]) { fail(g, sst[p.s], false); continue; }
        p.nb = src[p.s].count; p.hbits = sbit[p.s]; p.outputSize = ssize[p.s]; p.fr = frames.data() + src[p.s].row_first;
        const uint32_t nb = p.nb;
        const uint64_t base = nb ? (uint64_t)(nb - 1) * bs : 0;
        const int nw = (int)tg.w.size();
        std::vector<std::pair<uint64_t, uint64_t>> iv;                    // block ids [first, last]
        for (int i = 0; i < nw; i++) {
            const knz_write& w = tg.w[i];
            if (w.offset == KNZ_OFFSET_END || w.offset + w.length > base) p.needL = true;
            if (w.offset == KNZ_OFFSET_END || w.length == 0) continue;
            const uint64_t a = w.offset / bs + 1, b = std::min<uint64_t>((w.offset + w.length - 1) / bs + 1, nb);
            if (a <= b) iv.push_back({a, b});
        }
        if (p.needL && nb) iv.push_back({nb, nb});
        std::sort(iv.begin(), iv.end());
        uint64_t next = 1;
        for (const auto& v : iv) {
            for (uint64_t b = std::max(v.first, next); b <= v.second; b++) p.T.push_back((uint32_t)b);
            next = std::max(next, v.second + 1);
        }
        // room for the touched and the new blocks before the decode batch places into it: L <= n_blocks * block_size bounds the growth
        p.off.resize(nw);
        p.hole = write_resolve(tg.w.data(), nw, (uint64_t)nb * bs, p.off, p.newLen);
        if (p.hole >= 0) continue;                                        // (a hole under the largest L there can be: found again below)
        const uint64_t grown = (p.newLen + bs - 1) / bs;
        p.slots = p.T.size() + (grown > nb ? grown - nb : 0);
        if (p.slots >= ((uint64_t)1 << 30)) { fail(g, knz_set_error(h, KNZ_ERR_BLOCK_SIZE, "too many blocks in one call"), false); continue; }
        p.slot0 = slots; p.e0 = E0;
        slots += p.slots; E0 += p.T.size();
    }
    if (slots >= ((uint64_t)1 << 30)) return knz_set_error(h, KNZ_ERR_BLOCK_SIZE, "too many blocks in one call");
    if (wb.blocks.reserve(slots * bs + 64)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
    auto live = [&](int g) { return run[g]->status == 0 && plan[g].hole < 0; };

    // ONE decode batch over the touched existing blocks of all targets ; its rows bring the decoded lengths: L
    if (E0) {
        std::vector<knz_stream> es((size_t)E0);
        std::vector<knz_block_range> rg((size_t)E0);
        std::vector<uint32_t> fb((size_t)E0, 0);
        for (int g = 0; g < n; g++) {
            if (!live(g)) continue;
            const WsPlan& p = plan[g];
            const knz_write_target& t = targets[run[g]->t];
            for (size_t e = 0; e < p.T.size(); e++) {
                const size_t k = (size_t)p.e0 + e;
                memset(&es[k], 0, sizeof(knz_stream));
                es[k].d_src = t.d_src; es[k].n = t.n_bytes; es[k].d_dst = wb.blocks.as<uint8_t>() + (p.slot0 + e) * bs; es[k].dst_cap = bs;
                rg[k].from_block = p.T[e]; rg[k].to_block = p.T[e] + 1; rg[k].from_bit = p.frame_start(p.T[e] - 1);
                fb[k] = p.hbits;
            }
        }
        uint64_t entered = 0;
        many_split_retry(h, es.data(), (int)E0, st, [&](int lo, int cnt) { return decompress_many_once(h, es.data() + lo, fb.data() + lo, rg.data() + lo, sc, cnt, st, entered); });
        dec += entered;
        for (int g = 0; g < n; g++) {
            if (!live(g) || plan[g].T.empty()) continue;
            WsTarget& tg = *run[g];
            WsPlan& p = plan[g];
            const std::vector<uint32_t>& T = p.T;
            const uint32_t nb = p.nb;
            const uint64_t base = (uint64_t)(nb - 1) * bs;
            knz_stream* te = es.data() + p.e0;
            bool bad = false;
            for (size_t e = 0; e < T.size(); e++) {
                if (!te[e].status && T[e] != nb && te[e].out_bytes != bs) te[e].status = knz_set_error(h, KNZ_ERR_INVALID_PARAM, "a write touches a short inner block");
                bad = bad || te[e].status != 0;
            }
            if (bad) {                                                    // every write takes the code of the first failing block it touches
                int first = KNZ_OK;
                for (size_t i = 0; i < tg.w.size(); i++) {
                    knz_write& w = tg.w[i];
                    uint64_t a = nb, b = nb;                              // (a write that needs L touches the last block)
                    if (w.offset != KNZ_OFFSET_END) {
                        if (w.offset + w.length <= base && w.length == 0) continue;
                        a = std::min<uint64_t>(w.offset / bs + 1, nb);
                        if (w.offset + w.length <= base) b = (w.offset + w.length - 1) / bs + 1;
                    }
                    for (size_t e = std::lower_bound(T.begin(), T.end(), (uint32_t)a) - T.begin(); e < T.size() && T[e] <= b && !w.status; e++) w.status = te[e].status;
                    if (w.status && !first) first = w.status;
                }
                fail(g, first ? first : KNZ_ERR_UNKNOWN, first != KNZ_OK);
                continue;
            }
            if (p.needL) p.L = base + te[T.size() - 1].out_bytes;
        }
    }

    // per target: the writes resolved under its L, the rows of the encode batch, the visible pieces, the pieces of the new stream
    std::vector<WriteCopy> cps;
    std::vector<WritePiece> pcs;
    std::vector<WsOut> outs(n);
    uint64_t E = 0, maxLen = 0, estimate = 0;
    int nEnc = 0;
    auto piece = [&](uint32_t kind, uint64_t s, uint64_t nbits) { WritePiece q; memset(&q, 0, sizeof(q)); q.kind = kind; q.src = s; q.nbits = nbits; pcs.push_back(q); };
    for (int g = 0; g < n; g++) {
        WsTarget& tg = *run[g];
        WsPlan& p = plan[g];
        const knz_write_target& t = targets[tg.t];
        const int nw = (int)tg.w.size();
        if (tg.status == 0 && p.hole < 0 && p.needL) p.hole = write_resolve(tg.w.data(), nw, p.L, p.off, p.newLen);      // (no L: every write lies in front of the last block, nothing moves)
        if (tg.status == 0 && p.hole >= 0) {
            tg.w[p.hole].status = KNZ_ERR_INVALID_PARAM;
            fail(g, knz_set_error(h, KNZ_ERR_INVALID_PARAM, "a write starts behind the end of the stream (or its end overflows)"), true);
        }
        WsOut& o = outs[g];
        memset(&o, 0, sizeof(o));
        o.dst = (uint64_t)t.d_dst; o.cap = t.dst_cap; o.old_words = (uint64_t)t.d_src; o.piece_first = (uint32_t)pcs.size(); o.status = tg.status;
        if (tg.status) continue;
        const uint32_t nb = p.nb;
        p.grow = p.needL ? p.newLen - p.L : 0;
        const uint64_t nbNew = p.needL ? (p.newLen + bs - 1) / bs : nb;   // blocks of the new stream
        for (uint32_t b : p.T) if (b <= nbNew) p.rows.push_back(b);      // (a last block that decoded to nothing and got nothing leaves)
        p.keep = (uint32_t)std::min<uint64_t>(nb, nbNew);
        for (uint64_t b = (uint64_t)nb + 1; b <= nbNew; b++) p.rows.push_back((uint32_t)b);
        const std::vector<uint32_t>& rows = p.rows;
        const uint32_t Et = (uint32_t)rows.size();
        p.lastLen = (p.needL && Et && rows[Et - 1] == nbNew) ? p.newLen - (nbNew - 1) * bs : bs;
        p.row0 = E;
        E += Et;
        if (Et) { nEnc++; maxLen = std::max(maxLen, Et > 1 ? bs : p.lastLen); }
        auto row_of = [&](uint64_t id) { return (uint64_t)(std::lower_bound(rows.begin(), rows.end(), (uint32_t)id) - rows.begin()); };
        {   // the visible pieces: the writes from the last to the first, each takes what no later one has covered
            std::map<uint64_t, uint64_t> cov;                             // covered intervals lo -> hi, disjoint
            for (int i = nw - 1; i >= 0; i--) {
                if (!tg.w[i].length) continue;
                const uint64_t lo = p.off[i], hi = lo + tg.w[i].length;
                auto emit = [&](uint64_t a, uint64_t b) {
                    cps.push_back({(uint64_t)wb.blocks.p + (p.slot0 + row_of(a / bs + 1)) * bs + a % bs, (uint64_t)tg.w[i].d_data + (a - lo), b - a});
                };
                auto it = cov.upper_bound(lo);
                if (it != cov.begin() && std::prev(it)->second > lo) --it;
                uint64_t cur = lo, mlo = lo, mhi = hi;
                while (it != cov.end() && it->first < hi) {
                    if (it->first > cur) emit(cur, it->first);
                    cur = std::max(cur, it->second);
                    mlo = std::min(mlo, it->first); mhi = std::max(mhi, it->second);
                    it = cov.erase(it);
                }
                if (cur < hi) emit(cur, hi);
                cov[mlo] = mhi;
            }
        }
        int64_t hs = t.header_input_size;
        if (hs == KNZ_HEADER_SIZE_KEEP) hs = p.outputSize ? p.outputSize + (int64_t)p.grow : 0;
        piece(KNZ_WP_HEADER, 0, knz_build_stream_header(cfg, hs, o.hdr_words));
        uint32_t at = 1;                                                  // the next block to place
        for (uint32_t r = 0; r <= Et; r++) {
            const uint32_t upto = r < Et ? std::min(rows[r] - 1, p.keep) : p.keep;     // untouched frames at .. upto go verbatim, as one run
            if (at <= upto) piece(KNZ_WP_RUN, p.frame_start(at - 1), p.frame_end(upto - 1) - p.frame_start(at - 1));
            if (r < Et) { piece(KNZ_WP_FRAME, p.row0 + r, 0); at = rows[r] + 1; }
        }
        piece(KNZ_WP_END, 0, 8);
        o.P = (uint32_t)pcs.size() - o.piece_first;
    }
    const size_t K = cps.size(), P = pcs.size();
    if (K >= ((size_t)1 << 31) || P >= ((size_t)1 << 31) || E >= ((uint64_t)1 << 30)) return knz_set_error(h, KNZ_ERR_BLOCK_SIZE, "too many writes in one call");

    // tables: [copies | their scan] for the overlay ; [targets | pieces | bit counts | scan of the groups] for the splice, behind them
    const size_t ovBytes = sizeof(WriteCopy) * K + 8 * (K + 1);
    const size_t spBytes = sizeof(WsOut) * (size_t)n + sizeof(WritePiece) * P + 8 * (size_t)E, spDev = spBytes + 8 * ((size_t)n + 1);
    const uint64_t ostride = block_stream_bound(cfg.transform, cfg.entropy, bs);
    if (wb.pinned.reserve(ovBytes + spBytes)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "pinned host allocation failed");
    if (wb.tab.reserve(ovBytes + spDev + 64) || wb.streams.reserve(ostride * E + 64) || h->total_bits.reserve(64))
        return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
    if (K) {                                                              // ONE overlay launch (the encode batch below synchronises behind it)
        WriteCopy* hc = wb.pinned.as<WriteCopy>();
        uint64_t* hb = (uint64_t*)(hc + K);
        hb[0] = 0;
        for (size_t k = 0; k < K; k++) { hc[k] = cps[k]; hb[k + 1] = hb[k] + (((cps[k].dst + cps[k].len + 15) >> 4) - (cps[k].dst >> 4)); }
        HIP_OK(hipMemcpyAsync(wb.tab.p, hc, ovBytes, hipMemcpyHostToDevice, st));
        WriteOverlayArgs oa;
        oa.pieces = wb.tab.as<WriteCopy>(); oa.K = (uint32_t)K; oa.base = (const uint64_t*)(oa.pieces + K);
        KNZ_LAUNCH_PROBED(knz_write_overlay_kernel, dim3((unsigned)std::min<uint64_t>((hb[K] + 255) / 256, 1u << 14)), dim3(256), 0, st, oa);
    }

    // ONE encode batch over the touched and the new blocks of all targets, in the block-streams form: a target's rows are one "stream" of the table
    std::vector<uint64_t> written((size_t)E, 0);
    if (E) {
        if (h->many_pinned.reserve(sizeof(ManyStream) * (size_t)nEnc)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "pinned host allocation failed");
        if (h->many_tab.reserve(sizeof(ManyStream) * (size_t)nEnc) || h->many_blk_stream.reserve(4 * (E + 1)))
            return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
        ManyStream* tab = h->many_pinned.as<ManyStream>();
        int k = 0;
        for (int g = 0; g < n; g++) {
            const WsPlan& p = plan[g];
            if (run[g]->status || p.rows.empty()) continue;
            ManyStream& m = tab[k++];
            memset(&m, 0, sizeof(m));
            m.src = (uint64_t)wb.blocks.p + p.slot0 * bs; m.n = (uint64_t)(p.rows.size() - 1) * bs + p.lastLen;
        }
        ManyStream* dtab = h->many_tab.as<ManyStream>();
        HIP_OK(hipMemcpyAsync(dtab, tab, sizeof(ManyStream) * (size_t)nEnc, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(knz_many_scan_kernel, dim3(1), dim3(256), 0, st, dtab, (uint32_t)nEnc, bs, 1u, h->total_bits.as<uint32_t>() + 8);
        EncodeBatch eb = EncodeBatch::block_streams(nullptr, 0, wb.streams.as<uint8_t>(), ostride, E);
        eb.many = {dtab, (uint32_t)nEnc, (uint32_t)E, (uint32_t)maxLen, h->many_blk_stream.as<uint32_t>()};
        eb.keep_probes = 1;
        const int erc = encode_batch(h, eb, st);
        if (erc) return erc;
        enc += E;
        const Handle::ResultRow* rr = h->pinned_rows.as<Handle::ResultRow>();
        for (int g = 0; g < n; g++) {
            const WsPlan& p = plan[g];
            if (run[g]->status) continue;
            for (size_t r = 0; r < p.rows.size(); r++) {
                written[(size_t)p.row0 + r] = rr[p.row0 + r].written;
                if (rr[p.row0 + r].status && !run[g]->status) fail(g, knz_set_error(h, rr[p.row0 + r].status, "block failed (the reference panics on this input: ERR_PROCESS_BLOCK)"), false);
            }
            if (run[g]->status) outs[g].status = run[g]->status;
        }
    } else if (K) HIP_OK(hipStreamSynchronize(st));

    // the splice: ONE plan launch (a workgroup per target), the scan of the targets' groups, ONE copy launch
    uint8_t* hsp = wb.pinned.as<uint8_t>() + ovBytes;
    WsOut* ho = (WsOut*)hsp;
    WritePiece* hp = (WritePiece*)(ho + n);
    uint64_t* hw = (uint64_t*)(hp + P);
    for (int g = 0; g < n; g++) {
        ho[g] = outs[g];
        if (outs[g].status) continue;
        uint64_t bits = 0;                                                // (sizes the copy kernel's grid ; the plan kernel's total is the one that counts)
        for (uint32_t q = outs[g].piece_first; q < outs[g].piece_first + outs[g].P; q++) bits += pcs[q].kind == KNZ_WP_FRAME ? 5 + write_lw(written[pcs[q].src]) + written[pcs[q].src] : pcs[q].nbits;
        estimate += (bits / 32 + 8) / 4 + 3;
    }
    for (size_t q = 0; q < P; q++) hp[q] = pcs[q];
    for (size_t r = 0; r < (size_t)E; r++) hw[r] = written[r];
    uint8_t* dsp = wb.tab.as<uint8_t>() + ((ovBytes + 15) & ~(size_t)15);
    HIP_OK(hipMemcpyAsync(dsp, hsp, spBytes, hipMemcpyHostToDevice, st));
    WsArgs sa;
    sa.outs = (WsOut*)dsp; sa.T = (uint32_t)n; sa.pieces = (WritePiece*)(sa.outs + n); sa.written = (const uint64_t*)(sa.pieces + P);
    sa.streams = wb.streams.as<uint8_t>(); sa.stride = ostride; sa.base = (uint64_t*)(sa.written + E);
    KNZ_LAUNCH_PROBED(knz_ws_plan_kernel, dim3((unsigned)n), dim3(256), 0, st, sa);
    ReadArgs scan;                                                        // read.hip's scan, as it stands: it looks at R and base only
    memset(&scan, 0, sizeof(scan));
    scan.R = (uint32_t)n; scan.base = sa.base;
    KNZ_LAUNCH_PROBED(knz_read_scan_kernel, dim3(1), dim3(KNZ_READ_SCAN_THREADS), 0, st, scan);
    KNZ_LAUNCH_PROBED(knz_ws_copy_kernel, dim3((unsigned)std::min<uint64_t>((estimate + 255) / 256 + 1, 1u << 14)), dim3(256), 0, st, sa);
    HIP_OK(hipMemcpyAsync(ho, dsp, sizeof(WsOut) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    for (int g = 0; g < n; g++) {
        if (run[g]->status) continue;
        if (ho[g].status) { fail(g, knz_set_error(h, ho[g].status, "destination buffer too small"), false); continue; }
        run[g]->out_bytes = (ho[g].total_bits + 7) >> 3;
    }
    return KNZ_OK;
}

extern "C" int knz_dev_write_streams(void* handle, knz_write_target* targets, int n_targets, knz_write_to* writes, int n_writes, void* hip_stream) {
    if (!handle) return KNZ_ERR_MISSING_PARAM;
    if (n_targets <= 0) return KNZ_OK;
    if (n_writes < 0) n_writes = 0;
    if (!targets || (!writes && n_writes)) return KNZ_ERR_MISSING_PARAM;
    Handle* top = (Handle*)handle;
    Handle* h = lane_of_pointer(top, targets[0].d_dst);
    if (!h) h = lane0(top);
    DeviceGuard dg(h);
    h->dec_blocks = 0; h->enc_blocks = 0;
    bool malformed = false;
    for (int t = 0; t < n_targets; t++) { targets[t].out_bytes = 0; targets[t].status = 0; targets[t].reserved = 0; }
    for (int i = 0; i < n_writes; i++) { writes[i].status = 0; writes[i].reserved = 0; if (writes[i].target >= (uint32_t)n_targets) malformed = true; }
    if (malformed) {
        for (int t = 0; t < n_targets; t++) targets[t].status = KNZ_ERR_INVALID_PARAM;
        for (int i = 0; i < n_writes; i++) writes[i].status = KNZ_ERR_INVALID_PARAM;
        return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "writes[].target must index targets[]");
    }
    // the targets some write names (the others: status 0, out_bytes 0, nothing written: the single call's n_writes <= 0), each with its writes in index order
    std::vector<int> of(n_targets, -1);
    std::vector<WsTarget> tg;
    for (int i = 0; i < n_writes; i++) {
        int& g = of[writes[i].target];
        if (g < 0) { g = (int)tg.size(); tg.emplace_back(); tg.back().t = (int)writes[i].target; }
        knz_write w;
        memset(&w, 0, sizeof(w));
        w.offset = writes[i].offset; w.length = writes[i].length; w.d_data = writes[i].d_data;
        tg[g].wi.push_back(i);
        tg[g].w.push_back(w);
    }
    std::sort(tg.begin(), tg.end(), [](const WsTarget& a, const WsTarget& b) { return a.t < b.t; });
    // what the single call refuses before it looks at the stream, in its order: NULL pointers (the writes are not looked at), a write's own arguments, alignment ;
    // then the call's own rules for a destination: its device, its overlaps
    std::vector<int32_t> ost(tg.size(), 0);
    for (size_t g = 0; g < tg.size(); g++) {
        const knz_write_target& t = targets[tg[g].t];
        if (!t.d_src || !t.d_dst) { ost[g] = KNZ_ERR_MISSING_PARAM; tg[g].blamed = true; continue; }
        int first = KNZ_OK;
        for (knz_write& w : tg[g].w) {
            if (w.offset != KNZ_OFFSET_END && w.offset + w.length < w.offset) w.status = KNZ_ERR_INVALID_PARAM;
            else if (!w.d_data && w.length) w.status = KNZ_ERR_MISSING_PARAM;
            if (w.status && !first) first = w.status;
        }
        if (first) { ost[g] = first; tg[g].blamed = true; continue; }
        if (((uintptr_t)t.d_src & 3) || ((uintptr_t)t.d_dst & 3)) { ost[g] = KNZ_ERR_INVALID_PARAM; continue; }
        hipPointerAttribute_t at;
        if (top->multi) {
            if (hipPointerGetAttributes(&at, t.d_dst) == hipSuccess) { if (at.device != h->device) ost[g] = KNZ_ERR_INVALID_PARAM; }
            else (void)hipGetLastError();
        }
    }
    write_streams_mark_overlaps(targets, tg, ost);
    std::vector<WsTarget*> run;
    for (size_t g = 0; g < tg.size(); g++) { tg[g].status = ost[g]; if (!ost[g]) run.push_back(&tg[g]); }
    if (!run.empty()) {
        hipStream_t st = dev_call_stream(h, hip_stream);
        uint64_t dec = 0, enc = 0;
        split_retry(h, 0, (int)run.size(), true, &st, [&](int lo, int cnt) {
            uint64_t d = 0, e = 0;
            const int rc = write_streams_once(h, run.data() + lo, cnt, targets, st, d, e);
            if (!rc) { dec += d; enc += e; }
            return rc;
        }, [&](int lo, int cnt, int rc) { for (int g = lo; g < lo + cnt; g++) { run[g]->status = rc; run[g]->blamed = false; run[g]->out_bytes = 0; } });
        h->dec_blocks = dec; h->enc_blocks = enc;
    }
    int first = KNZ_OK;
    for (const WsTarget& g : tg) {
        targets[g.t].status = g.status;
        targets[g.t].out_bytes = g.status ? 0 : g.out_bytes;
        for (size_t i = 0; i < g.wi.size(); i++) writes[g.wi[i]].status = (g.status && !g.blamed) ? g.status : g.w[i].status;
        if (g.status && !first) first = g.status;
    }
    if (first) return knz_set_error(h, first, first == KNZ_ERR_WRITE_FILE ? "destination buffer of a target too small" : "a target of the call failed (see its status and its writes')");
    return KNZ_OK;
}
