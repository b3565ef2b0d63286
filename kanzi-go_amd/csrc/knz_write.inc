// knz_dev_write_many / knz_dev_append (included by knz_gpu.hip): W byte writes into one source stream -> one new stream. The plan is made here, in
// O(W log W) beside the framing walk: which existing blocks the writes touch (one entry {b, b + 1} each of ONE decompress_many_once, placed side by side at
// a stride of one block size), the old length L from that batch's result rows where the last block is touched, the writes resolved and swept into disjoint
// visible pieces (a later write wins), the new blocks, the pieces of the new stream. write.hip lays the visible pieces over the decoded blocks, the encode
// batch turns every touched and new block into its block-local stream, and the splice kernels put header, verbatim runs, new frames and end marker
// together. Nothing of d_dst is written before the plan kernel has checked dst_cap, and nothing at all by a call that fails.
#include <map>

// the writes applied in order to a stream of len bytes: every write's resolved offset and the new length. Returns the first write that would leave a
// hole (or whose end overflows), -1: none
static int write_resolve(const knz_write* w, int n, uint64_t len, std::vector<uint64_t>& off, uint64_t& newLen) {
    uint64_t cur = len;
    for (int i = 0; i < n; i++) {
        const uint64_t o = w[i].offset == KNZ_OFFSET_END ? cur : w[i].offset;
        if (o > cur || o + w[i].length < o) return i;
        off[i] = o;
        cur = std::max(cur, o + w[i].length);
    }
    newLen = cur;
    return -1;
}

static uint32_t write_lw(uint64_t written) { return written >= 8 ? (63u - (uint32_t)__builtin_clzll(written >> 3)) + 4 : 3; }      // knz_many_lw

// blamed: the writes at fault carry their codes (else the code is the call's, and goes to every write)
static int write_many_run(Handle* h, const void* d_src, uint64_t n_bytes, knz_write* writes, int n, int64_t header_input_size, void* d_dst, uint64_t dst_cap,
                          uint64_t* out_bytes, hipStream_t st, bool& blamed) {
    const knz_cfg& cfg = h->cfg;
    knz_cfg sc = cfg;
    int64_t outputSize = 0;
    uint32_t hbits = 0;
    int rc = read_stream_header(h, d_src, n_bytes, st, sc, outputSize, hbits);
    if (rc) return rc;
    if (sc.transform != cfg.transform || sc.entropy != cfg.entropy || sc.block_size != cfg.block_size || sc.checksum_bits != cfg.checksum_bits)
        return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "the source stream was not written under the handle's configuration");
    if (!h->wr) h->wr.reset(new WriteBufs());
    WriteBufs& wb = *h->wr;

    // the framing, from the header to the end marker: every block's payload bit and bit count (frame i starts where frame i - 1 ends)
    const uint32_t bound = (uint32_t)std::min<uint64_t>(n_bytes / 3 + 1, 1u << 24);
    uint32_t nb = 0;
    std::vector<uint64_t> pay, bits;
    for (uint32_t cap = std::min<uint32_t>(bound, 4096);;) {
        const size_t bytes = 8 * (4 + 2 * (size_t)cap);
        if (h->blk_dst_bit.reserve(bytes)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
        if (h->pinned_rows.reserve(bytes)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "pinned host allocation failed");
        WalkRangeArgs wr;
        wr.stream = (const uint8_t*)d_src; wr.nbytes = n_bytes; wr.first_bit = hbits; wr.first_id = 1; wr.from = 1; wr.to = ~(uint64_t)0;
        wr.max_blocks = bound; wr.cap = cap; wr.frames = 0; wr.stride = 2; wr.hinted = 0;
        wr.result = h->blk_dst_bit.as<uint64_t>(); wr.blk_bit = wr.result + 4; wr.blk_bits = wr.result + 5;
        hipLaunchKernelGGL(knz_dec_walk_range_kernel, dim3(1), dim3(1), 0, st, wr);
        const uint64_t* res = h->pinned_rows.as<uint64_t>();
        HIP_OK(hipMemcpyAsync(h->pinned_rows.p, h->blk_dst_bit.p, bytes, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipGetLastError());
        if (res[1]) return knz_set_error(h, (int)res[1], "invalid block framing in stream");
        nb = (uint32_t)res[0];
        if (nb > cap) { cap = nb; continue; }                             // (more frames than rows: once more, with room for all)
        pay.resize(nb); bits.resize(nb);
        for (uint32_t i = 0; i < nb; i++) { pay[i] = res[4 + 2 * (size_t)i]; bits[i] = res[5 + 2 * (size_t)i]; }
        break;
    }
    auto frame_start = [&](uint32_t i) { return i ? pay[i - 1] + bits[i - 1] : (uint64_t)hbits; };     // i: block index from 0
    auto frame_end = [&](uint32_t i) { return pay[i] + bits[i]; };

    // the existing blocks the writes touch, and whether L is needed
    const uint64_t bs = cfg.block_size, base = nb ? (uint64_t)(nb - 1) * bs : 0;
    bool needL = false;
    std::vector<std::pair<uint64_t, uint64_t>> iv;                        // block ids [first, last]
    for (int i = 0; i < n; i++) {
        const knz_write& w = writes[i];
        if (w.offset == KNZ_OFFSET_END || w.offset + w.length > base) needL = true;
        if (w.offset == KNZ_OFFSET_END || w.length == 0) continue;
        const uint64_t a = w.offset / bs + 1, b = std::min<uint64_t>((w.offset + w.length - 1) / bs + 1, nb);
        if (a <= b) iv.push_back({a, b});
    }
    if (needL && nb) iv.push_back({nb, nb});
    std::sort(iv.begin(), iv.end());
    std::vector<uint32_t> T;                                              // touched existing blocks, ids from 1, sorted
    uint64_t next = 1;
    for (const auto& v : iv) {
        for (uint64_t b = std::max(v.first, next); b <= v.second; b++) T.push_back((uint32_t)b);
        next = std::max(next, v.second + 1);
    }
    // room for the touched and the new blocks before the decode batch places into it: L <= n_blocks * block_size bounds the growth
    std::vector<uint64_t> off(n);
    uint64_t newLen = 0;
    int hole = write_resolve(writes, n, (uint64_t)nb * bs, off, newLen);
    if (hole < 0) {
        const uint64_t grown = (newLen + bs - 1) / bs, rowsMax = T.size() + (grown > nb ? grown - nb : 0);
        if (rowsMax >= ((uint64_t)1 << 30)) return knz_set_error(h, KNZ_ERR_BLOCK_SIZE, "too many blocks in one call");
        if (wb.blocks.reserve(rowsMax * bs + 64)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
    }

    // ONE decode batch over the touched existing blocks, block e placed at blocks + e * block_size ; its rows bring the decoded lengths: L
    uint64_t L = 0;
    if (hole < 0 && !T.empty()) {
        const int E0 = (int)T.size();
        std::vector<knz_stream> es(E0);
        std::vector<knz_block_range> rg(E0);
        std::vector<uint32_t> fb(E0, hbits);
        for (int e = 0; e < E0; e++) {
            memset(&es[e], 0, sizeof(knz_stream));
            es[e].d_src = d_src; es[e].n = n_bytes; es[e].d_dst = wb.blocks.as<uint8_t>() + (uint64_t)e * bs; es[e].dst_cap = bs;
            rg[e].from_block = T[e]; rg[e].to_block = T[e] + 1; rg[e].from_bit = frame_start(T[e] - 1);
        }
        uint64_t entered = 0;
        many_split_retry(h, es.data(), E0, st, [&](int lo, int cnt) { return decompress_many_once(h, es.data() + lo, fb.data() + lo, rg.data() + lo, sc, cnt, st, entered); });
        h->dec_blocks = entered;
        bool bad = false;
        for (int e = 0; e < E0; e++) {
            if (!es[e].status && T[e] != nb && es[e].out_bytes != bs) es[e].status = knz_set_error(h, KNZ_ERR_INVALID_PARAM, "a write touches a short inner block");
            bad = bad || es[e].status != 0;
        }
        if (bad) {                                                        // every write takes the code of the first failing block it touches
            int first = KNZ_OK;
            for (int i = 0; i < n; i++) {
                const knz_write& w = writes[i];
                uint64_t a = nb, b = nb;                                  // (a write that needs L touches the last block)
                if (w.offset != KNZ_OFFSET_END) {
                    if (w.offset + w.length <= base && w.length == 0) continue;
                    a = std::min<uint64_t>(w.offset / bs + 1, nb);
                    if (w.offset + w.length <= base) b = (w.offset + w.length - 1) / bs + 1;
                }
                for (size_t e = std::lower_bound(T.begin(), T.end(), (uint32_t)a) - T.begin(); e < T.size() && T[e] <= b && !writes[i].status; e++) writes[i].status = es[e].status;
                if (writes[i].status && !first) first = writes[i].status;
            }
            blamed = first != KNZ_OK;
            return first ? first : KNZ_ERR_UNKNOWN;
        }
        if (needL) L = base + es[E0 - 1].out_bytes;
    }
    if (hole < 0 && needL) hole = write_resolve(writes, n, L, off, newLen);      // (no L: every write lies in front of the last block, nothing moves)
    if (hole >= 0) {
        writes[hole].status = KNZ_ERR_INVALID_PARAM;
        blamed = true;
        return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "a write starts behind the end of the stream (or its end overflows)");
    }
    const uint64_t grow = needL ? newLen - L : 0;
    const uint64_t nbNew = needL ? (newLen + bs - 1) / bs : nb;           // blocks of the new stream
    std::vector<uint32_t> rows;                                           // the blocks of the encode batch: touched existing ones, then the new ones
    for (uint32_t b : T) if (b <= nbNew) rows.push_back(b);              // (a last block that decoded to nothing and got nothing leaves)
    const uint32_t keep = (uint32_t)std::min<uint64_t>(nb, nbNew);
    for (uint64_t b = (uint64_t)nb + 1; b <= nbNew; b++) rows.push_back((uint32_t)b);
    const uint32_t E = (uint32_t)rows.size();
    const uint64_t lastLen = (needL && E && rows[E - 1] == nbNew) ? newLen - (nbNew - 1) * bs : bs;
    auto row_of = [&](uint64_t id) { return (uint64_t)(std::lower_bound(rows.begin(), rows.end(), (uint32_t)id) - rows.begin()); };

    // the visible pieces: the writes from the last to the first, each takes what no later one has covered
    std::vector<WriteCopy> cps;
    {
        std::map<uint64_t, uint64_t> cov;                                 // covered intervals lo -> hi, disjoint
        for (int i = n - 1; i >= 0; i--) {
            if (!writes[i].length) continue;
            const uint64_t lo = off[i], hi = lo + writes[i].length;
            auto emit = [&](uint64_t a, uint64_t b) {
                cps.push_back({(uint64_t)wb.blocks.p + row_of(a / bs + 1) * bs + a % bs, (uint64_t)writes[i].d_data + (a - lo), b - a});
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
    // the pieces of the new stream
    std::vector<WritePiece> pcs;
    auto piece = [&](uint32_t kind, uint64_t src, uint64_t nbits) { WritePiece p; memset(&p, 0, sizeof(p)); p.kind = kind; p.src = src; p.nbits = nbits; pcs.push_back(p); };
    WriteSpliceArgs sa;
    int64_t hs = header_input_size;
    if (hs == KNZ_HEADER_SIZE_KEEP) hs = outputSize ? outputSize + (int64_t)grow : 0;
    piece(KNZ_WP_HEADER, 0, knz_build_stream_header(cfg, hs, sa.hdr_words));
    uint32_t at = 1;                                                      // the next block to place
    for (uint32_t r = 0; r <= E; r++) {
        const uint32_t upto = r < E ? std::min(rows[r] - 1, keep) : keep; // untouched frames at .. upto go verbatim, as one run
        if (at <= upto) piece(KNZ_WP_RUN, frame_start(at - 1), frame_end(upto - 1) - frame_start(at - 1));
        if (r < E) { piece(KNZ_WP_FRAME, r, 0); at = rows[r] + 1; }
    }
    piece(KNZ_WP_END, 0, 8);
    const uint32_t K = (uint32_t)cps.size(), P = (uint32_t)pcs.size();
    if (cps.size() >= ((size_t)1 << 31)) return knz_set_error(h, KNZ_ERR_BLOCK_SIZE, "too many writes in one call");

    // tables: [copies | their scan] for the overlay, [pieces | bit counts] for the splice
    const size_t ovBytes = sizeof(WriteCopy) * (size_t)K + 8 * ((size_t)K + 1), spBytes = sizeof(WritePiece) * (size_t)P + 8 * (size_t)E;
    const uint64_t ostride = block_stream_bound(cfg.transform, cfg.entropy, bs);
    if (wb.pinned.reserve(std::max(ovBytes, spBytes))) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "pinned host allocation failed");
    if (wb.tab.reserve(std::max(ovBytes, spBytes) + 64) || wb.streams.reserve(ostride * E + 64))
        return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
    if (K) {
        WriteCopy* hc = wb.pinned.as<WriteCopy>();
        uint64_t* hb = (uint64_t*)(hc + K);
        hb[0] = 0;
        for (uint32_t k = 0; k < K; k++) { hc[k] = cps[k]; hb[k + 1] = hb[k] + (((cps[k].dst + cps[k].len + 15) >> 4) - (cps[k].dst >> 4)); }
        HIP_OK(hipMemcpyAsync(wb.tab.p, hc, ovBytes, hipMemcpyHostToDevice, st));
        WriteOverlayArgs oa;
        oa.pieces = wb.tab.as<WriteCopy>(); oa.K = K; oa.base = (const uint64_t*)(oa.pieces + K);
        KNZ_LAUNCH_PROBED(knz_write_overlay_kernel, dim3((unsigned)std::min<uint64_t>((hb[K] + 255) / 256, 1u << 14)), dim3(256), 0, st, oa);
        HIP_OK(hipStreamSynchronize(st));                                 // (the pinned table is filled again below)
    }

    // ONE encode batch over the touched and the new blocks, in the block-streams form (in halves where the device refuses its workspace)
    std::vector<uint64_t> written(E, 0);
    if (E) {
        rc = split_retry(h, 0, (int)E, false, &st, [&](int lo, int cnt) {
            const uint64_t nbytes = (uint64_t)(cnt - 1) * bs + ((uint32_t)(lo + cnt) == E ? lastLen : bs);
            EncodeBatch eb = EncodeBatch::block_streams(wb.blocks.as<uint8_t>() + (uint64_t)lo * bs, nbytes, wb.streams.as<uint8_t>() + (uint64_t)lo * ostride, ostride, (uint64_t)cnt);
            eb.keep_probes = 1;
            const int erc = encode_batch(h, eb, st);
            if (erc) return erc;
            const Handle::ResultRow* rr = h->pinned_rows.as<Handle::ResultRow>();
            for (int i = 0; i < cnt; i++) written[lo + i] = rr[i].written;
            return (int)KNZ_OK;
        }, [](int, int, int) {});
        if (rc) return rc;
    }
    h->enc_blocks = E;

    // the splice
    WritePiece* hp = wb.pinned.as<WritePiece>();
    uint64_t* hw = (uint64_t*)(hp + P);
    uint64_t estimate = 0;                                                // (sizes the copy kernel's grid ; the plan kernel's total is the one that counts)
    for (uint32_t p = 0; p < P; p++) { hp[p] = pcs[p]; estimate += pcs[p].kind == KNZ_WP_FRAME ? 5 + write_lw(written[pcs[p].src]) + written[pcs[p].src] : pcs[p].nbits; }
    for (uint32_t r = 0; r < E; r++) hw[r] = written[r];
    if (h->total_bits.reserve(64)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
    HIP_OK(hipMemcpyAsync(wb.tab.p, hp, spBytes, hipMemcpyHostToDevice, st));
    sa.pieces = wb.tab.as<WritePiece>(); sa.P = P; sa.written = (const uint64_t*)(sa.pieces + P);
    sa.old_words = (const uint32_t*)d_src; sa.streams = wb.streams.as<uint8_t>(); sa.stride = ostride;
    sa.dst = (uint32_t*)d_dst; sa.cap = dst_cap; sa.result = h->total_bits.as<uint64_t>();
    KNZ_LAUNCH_PROBED(knz_write_splice_plan_kernel, dim3(1), dim3(256), 0, st, sa);
    const uint64_t groups = (estimate / 32 + 8) / 4 + 2;
    KNZ_LAUNCH_PROBED(knz_write_splice_copy_kernel, dim3((unsigned)std::min<uint64_t>((groups + 255) / 256, 1u << 14)), dim3(256), 0, st, sa);
    uint64_t* res = (uint64_t*)h->pinned;
    HIP_OK(hipMemcpyAsync(res, h->total_bits.p, 16, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    if (res[0]) return knz_set_error(h, (int)res[0], "destination buffer too small");
    *out_bytes = (res[1] + 7) >> 3;
    return KNZ_OK;
}

extern "C" int knz_dev_write_many(void* handle, const void* d_src, uint64_t n_bytes, knz_write* writes, int n_writes, int64_t header_input_size,
                                  void* d_dst, uint64_t dst_cap, uint64_t* out_bytes, void* hip_stream) {
    if (!handle) return KNZ_ERR_MISSING_PARAM;
    if (out_bytes) *out_bytes = 0;
    if (n_writes <= 0) return KNZ_OK;
    if (!writes || !d_src || !d_dst || !out_bytes) return KNZ_ERR_MISSING_PARAM;
    Handle* h = lane_of_pointer((Handle*)handle, d_dst);
    if (!h) return KNZ_ERR_MISSING_PARAM;
    DeviceGuard dg(h);
    h->dec_blocks = 0; h->enc_blocks = 0;
    int first = KNZ_OK;
    for (int i = 0; i < n_writes; i++) {
        knz_write& w = writes[i];
        w.status = 0; w.reserved = 0;
        if (w.offset != KNZ_OFFSET_END && w.offset + w.length < w.offset) w.status = KNZ_ERR_INVALID_PARAM;
        else if (!w.d_data && w.length) w.status = KNZ_ERR_MISSING_PARAM;
        if (w.status && !first) first = w.status;
    }
    bool blamed = first != KNZ_OK;
    int rc = first;
    if (rc) knz_set_error(h, rc, "a write of the call has invalid arguments (see its status)");
    else if (((uintptr_t)d_src & 3) || ((uintptr_t)d_dst & 3)) rc = knz_set_error(h, KNZ_ERR_INVALID_PARAM, "d_src and d_dst must be 4-byte aligned");
    else rc = write_many_run(h, d_src, n_bytes, writes, n_writes, header_input_size, d_dst, dst_cap, out_bytes, dev_call_stream(h, hip_stream), blamed);
    if (rc) {
        *out_bytes = 0;
        for (int i = 0; i < n_writes && !blamed; i++) writes[i].status = rc;
    }
    return rc;
}

extern "C" int knz_dev_append(void* handle, const void* d_src, uint64_t n_bytes, const void* d_data, uint64_t length, int64_t header_input_size,
                              void* d_dst, uint64_t dst_cap, uint64_t* out_bytes, void* hip_stream) {
    knz_write w;
    memset(&w, 0, sizeof(w));
    w.offset = KNZ_OFFSET_END; w.length = length; w.d_data = d_data;
    return knz_dev_write_many(handle, d_src, n_bytes, &w, 1, header_input_size, d_dst, dst_cap, out_bytes, hip_stream);
}
