// knz_dev_splice_many / knz_dev_concat / knz_dev_slice (included by knz_gpu.hip): parts (source stream, block range) -> output streams, whole frames
// moved as bits (splice.hip). The host does what needs no look at the framing: the pointer checks, the overlap of destinations with sources and with
// each other, the distinct sources and their heads (ONE gather, ONE pinned copy, parsed as knz_dev_decompress_many parses them), per source the sorted
// distinct boundaries its parts ask for, the outputs' headers. Everything else happens on the device behind ONE upload of the tables: walk, plan, scan,
// copy, and ONE pinned copy brings the output and part rows back. Two synchronisations and five launches, whatever the number of parts and outputs.

// outputs whose d_dst[0 .. dst_cap) meets a source of the call (its n_bytes rounded up to 4) or another output's range: KNZ_ERR_INVALID_PARAM. A sweep over
// the ranges sorted by their start: an output that overlaps anything meets, when the later of the two is visited, the furthest end seen so far.
static void splice_mark_overlaps(const knz_splice_part* parts, int n_parts, const knz_splice_out* outs, int n_outs, std::vector<int32_t>& ost) {
    struct Span { uint64_t lo, hi; int out; };                            // out < 0: a source
    std::vector<Span> sp;
    for (int i = 0; i < n_parts; i++)
        if (parts[i].d_src && parts[i].n_bytes) sp.push_back({(uint64_t)parts[i].d_src, (uint64_t)parts[i].d_src + ((parts[i].n_bytes + 3) & ~(uint64_t)3), -1});
    for (int o = 0; o < n_outs; o++)
        if (outs[o].d_dst && outs[o].dst_cap) sp.push_back({(uint64_t)outs[o].d_dst, (uint64_t)outs[o].d_dst + outs[o].dst_cap, o});
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

// pst / ost: what the host has refused so far (0: nothing). Returns 0 with every result row set, or a code that is no part's and no output's (workspace, runtime).
static int splice_run(Handle* h, knz_splice_part* parts, int n_parts, knz_splice_out* outs, int n_outs, hipStream_t st, std::vector<int32_t>& pst,
                      const std::vector<int32_t>& ost) {
    const knz_cfg& cfg = h->cfg;
    h->nprobes = 0;
    if ((uint64_t)n_parts + 2 * (uint64_t)n_outs >= ((uint64_t)1 << 31)) return knz_set_error(h, KNZ_ERR_BLOCK_SIZE, "too many parts in one call");
    // the distinct sources
    struct Key { uint64_t src, n; bool operator<(const Key& k) const { return src != k.src ? src < k.src : n < k.n; } bool operator==(const Key& k) const { return src == k.src && n == k.n; } };
    std::vector<Key> keys;
    for (int i = 0; i < n_parts; i++) if (!pst[i]) keys.push_back({(uint64_t)parts[i].d_src, parts[i].n_bytes});
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const uint32_t S = (uint32_t)keys.size();
    std::vector<int32_t> sst(S, 0);
    std::vector<int64_t> ssize(S, 0);
    std::vector<uint32_t> sbit(S, 0);
    if (S) {                                                              // their heads: one gather, one copy
        const size_t tabBytes = sizeof(ManyStream) * (size_t)S;
        if (h->many_pinned.reserve(tabBytes + 32 * (size_t)S)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "pinned host allocation failed");
        if (h->many_tab.reserve(tabBytes) || h->many_heads.reserve(32 * (size_t)S)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
        ManyStream* tab = h->many_pinned.as<ManyStream>();
        const uint8_t* heads = h->many_pinned.as<uint8_t>() + tabBytes;
        for (uint32_t s = 0; s < S; s++) { memset(&tab[s], 0, sizeof(ManyStream)); tab[s].src = keys[s].src; tab[s].n = keys[s].n; }
        HIP_OK(hipMemcpyAsync(h->many_tab.p, tab, tabBytes, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(knz_many_heads_kernel, dim3((S * 8 + 255) / 256), dim3(256), 0, st, (const ManyStream*)h->many_tab.as<ManyStream>(), S, h->many_heads.as<uint32_t>());
        HIP_OK(hipMemcpyAsync((void*)heads, h->many_heads.p, 32 * (size_t)S, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        for (uint32_t s = 0; s < S; s++) {
            knz_cfg sc = cfg;
            sst[s] = parse_stream_header(h, heads + 32 * (size_t)s, keys[s].n, sc, ssize[s], sbit[s]);
            if (!sst[s] && (sc.transform != cfg.transform || sc.entropy != cfg.entropy || sc.block_size != cfg.block_size || sc.checksum_bits != cfg.checksum_bits))
                sst[s] = knz_set_error(h, KNZ_ERR_INVALID_PARAM, "a source stream was not written under the handle's configuration");
        }
    }
    // per part its source ; per source the sorted distinct boundaries: block counts at which the walk leaves a mark (from_block - 1 and to_block - 1)
    std::vector<uint32_t> srcOf(n_parts, 0);
    std::vector<uint64_t> bkeys;                                          // source << 32 | boundary
    auto bound_hi = [](const knz_splice_part& p) { return p.to_block == KNZ_BLOCK_END ? KNZ_SPLICE_END : p.to_block - 1; };
    for (int i = 0; i < n_parts; i++) {
        if (pst[i]) continue;
        srcOf[i] = (uint32_t)(std::lower_bound(keys.begin(), keys.end(), Key{(uint64_t)parts[i].d_src, parts[i].n_bytes}) - keys.begin());
        if (sst[srcOf[i]]) { pst[i] = sst[srcOf[i]]; continue; }
        bkeys.push_back((uint64_t)srcOf[i] << 32 | (parts[i].from_block - 1));
        bkeys.push_back((uint64_t)srcOf[i] << 32 | bound_hi(parts[i]));
    }
    std::sort(bkeys.begin(), bkeys.end());
    bkeys.erase(std::unique(bkeys.begin(), bkeys.end()), bkeys.end());
    const size_t B = bkeys.size(), O = (size_t)n_outs, Pn = (size_t)n_parts;
    // the tables: [outputs | parts | sources | boundaries] go up ; [marks | pieces | scan] live on the device only
    const size_t boundBytes = (4 * B + 7) & ~(size_t)7;
    const size_t upBytes = sizeof(SpliceOut) * O + sizeof(SplicePart) * Pn + sizeof(SpliceSource) * (size_t)S + boundBytes;
    const size_t devBytes = upBytes + sizeof(SpliceMark) * B + sizeof(SplicePiece) * (Pn + 2 * O) + 8 * (O + 1);
    if (h->splice_pinned.reserve(upBytes)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "pinned host allocation failed");
    if (h->splice_tab.reserve(devBytes + 64)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
    SpliceOut* ho = h->splice_pinned.as<SpliceOut>();
    SplicePart* hp = (SplicePart*)(ho + O);
    SpliceSource* hs = (SpliceSource*)(hp + Pn);
    uint32_t* hb = (uint32_t*)(hs + S);
    for (uint32_t s = 0; s < S; s++) {
        SpliceSource& r = hs[s];
        r.src = keys[s].src; r.n = keys[s].n; r.first_bit = sbit[s]; r.status = sst[s];
        r.b_first = (uint32_t)(std::lower_bound(bkeys.begin(), bkeys.end(), (uint64_t)s << 32) - bkeys.begin());
        r.b_count = (uint32_t)(std::lower_bound(bkeys.begin(), bkeys.end(), (uint64_t)(s + 1) << 32) - bkeys.begin()) - r.b_first;
    }
    for (size_t b = 0; b < B; b++) hb[b] = (uint32_t)bkeys[b];
    uint64_t groups = 0;                                                  // an upper bound of the destination groups: sizes the copy kernel's grid
    for (int i = 0; i < n_parts; i++) {
        SplicePart& r = hp[i];
        memset(&r, 0, sizeof(r));
        r.status = pst[i];
        if (pst[i]) continue;
        r.source = srcOf[i];
        r.lo = (uint32_t)(std::lower_bound(bkeys.begin(), bkeys.end(), (uint64_t)srcOf[i] << 32 | (parts[i].from_block - 1)) - bkeys.begin());
        r.hi = (uint32_t)(std::lower_bound(bkeys.begin(), bkeys.end(), (uint64_t)srcOf[i] << 32 | bound_hi(parts[i])) - bkeys.begin());
        groups += parts[i].n_bytes / 16 + 1;
    }
    int at = 0;                                                           // the outputs' parts: consecutive, out non-decreasing (checked by the caller)
    for (int o = 0; o < n_outs; o++) {
        SpliceOut& r = ho[o];
        memset(&r, 0, sizeof(r));
        r.dst = (uint64_t)outs[o].d_dst; r.cap = outs[o].dst_cap; r.status = ost[o]; r.part_first = (uint32_t)at;
        bool whole = true;                                                // KNZ_HEADER_SIZE_KEEP: every part a whole stream that has the field
        int64_t sum = 0;
        for (; at < n_parts && parts[at].out == (uint32_t)o; at++) {
            const knz_splice_part& p = parts[at];
            if (pst[at] || p.from_block != 1 || p.to_block != KNZ_BLOCK_END || ssize[srcOf[at]] == 0) whole = false;
            else sum += ssize[srcOf[at]];
        }
        r.n_parts = (uint32_t)at - r.part_first;
        const int64_t size = outs[o].header_input_size == KNZ_HEADER_SIZE_KEEP ? (whole ? sum : 0) : outs[o].header_input_size;
        r.hdr_bits = knz_build_stream_header(cfg, size, r.hdr_words);
        groups += 8;
    }
    uint8_t* d = h->splice_tab.as<uint8_t>();
    SpliceArgs a;
    a.outs = (SpliceOut*)d; a.O = (uint32_t)O; a.parts = (SplicePart*)(a.outs + O); a.sources = (const SpliceSource*)(a.parts + Pn); a.S = S;
    a.bounds = (const uint32_t*)(a.sources + S); a.marks = (SpliceMark*)(d + upBytes); a.pieces = (SplicePiece*)(a.marks + B); a.base = (uint64_t*)(a.pieces + Pn + 2 * O);
    HIP_OK(hipMemcpyAsync(d, ho, upBytes, hipMemcpyHostToDevice, st));
    if (B) KNZ_LAUNCH_PROBED(knz_splice_walk_kernel, dim3((S + 63) / 64), dim3(64), 0, st, a);
    KNZ_LAUNCH_PROBED(knz_splice_plan_kernel, dim3((unsigned)O), dim3(256), 0, st, a);
    ReadArgs sc;                                                          // read.hip's scan, as it stands: it looks at R and base only
    memset(&sc, 0, sizeof(sc));
    sc.R = (uint32_t)O; sc.base = a.base;
    KNZ_LAUNCH_PROBED(knz_read_scan_kernel, dim3(1), dim3(KNZ_READ_SCAN_THREADS), 0, st, sc);
    KNZ_LAUNCH_PROBED(knz_splice_copy_kernel, dim3((unsigned)std::min<uint64_t>((groups + 255) / 256, 1u << 14)), dim3(256), 0, st, a);
    const size_t backBytes = sizeof(SpliceOut) * O + sizeof(SplicePart) * Pn;
    HIP_OK(hipMemcpyAsync(ho, d, backBytes, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    for (int i = 0; i < n_parts; i++) { parts[i].status = hp[i].status; parts[i].blocks = hp[i].status ? 0 : hp[i].blocks; parts[i].bits = hp[i].status ? 0 : hp[i].bits; }
    for (int o = 0; o < n_outs; o++) {
        outs[o].status = ho[o].status;
        outs[o].out_bytes = ho[o].status ? 0 : (ho[o].total_bits + 7) >> 3;
        outs[o].out_blocks = ho[o].status ? 0 : ho[o].blocks;
    }
    return KNZ_OK;
}

extern "C" int knz_dev_splice_many(void* handle, knz_splice_part* parts, int n_parts, knz_splice_out* outs, int n_outs, void* hip_stream) {
    if (!handle) return KNZ_ERR_MISSING_PARAM;
    if (n_outs <= 0) return KNZ_OK;
    if (n_parts < 0) n_parts = 0;
    if (!outs || (!parts && n_parts)) return KNZ_ERR_MISSING_PARAM;
    Handle* top = (Handle*)handle;
    Handle* h = lane_of_pointer(top, outs[0].d_dst);
    if (!h) h = lane0(top);
    DeviceGuard dg(h);
    h->dec_blocks = 0; h->enc_blocks = 0;
    bool order = true;
    for (int i = 0; i < n_parts; i++) {
        parts[i].status = 0; parts[i].blocks = 0; parts[i].bits = 0;
        if (parts[i].out >= (uint32_t)n_outs || (i && parts[i].out < parts[i - 1].out)) order = false;
    }
    for (int o = 0; o < n_outs; o++) { outs[o].out_bytes = 0; outs[o].out_blocks = 0; outs[o].status = 0; outs[o].reserved = 0; }
    if (!order) {
        for (int o = 0; o < n_outs; o++) outs[o].status = KNZ_ERR_INVALID_PARAM;
        return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "parts[].out must index outs[] and must not decrease");
    }
    std::vector<int32_t> pst(n_parts, 0), ost(n_outs, 0);
    for (int i = 0; i < n_parts; i++) {
        const knz_splice_part& p = parts[i];
        if (!p.d_src) pst[i] = KNZ_ERR_MISSING_PARAM;
        else if (((uintptr_t)p.d_src & 3) || p.from_block == 0 || p.to_block <= p.from_block) pst[i] = KNZ_ERR_INVALID_PARAM;
    }
    for (int o = 0; o < n_outs; o++) {
        if (!outs[o].d_dst) { ost[o] = KNZ_ERR_MISSING_PARAM; continue; }
        if ((uintptr_t)outs[o].d_dst & 3) { ost[o] = KNZ_ERR_INVALID_PARAM; continue; }
        hipPointerAttribute_t at;
        if (top->multi) {
            if (hipPointerGetAttributes(&at, outs[o].d_dst) == hipSuccess) { if (at.device != h->device) ost[o] = KNZ_ERR_INVALID_PARAM; }
            else (void)hipGetLastError();
        }
    }
    splice_mark_overlaps(parts, n_parts, outs, n_outs, ost);
    const int rc = splice_run(h, parts, n_parts, outs, n_outs, dev_call_stream(h, hip_stream), pst, ost);
    if (rc) {                                                             // (no row has come back: the code is every output's, nothing was written)
        for (int i = 0; i < n_parts; i++) { parts[i].status = pst[i]; parts[i].blocks = 0; parts[i].bits = 0; }
        for (int o = 0; o < n_outs; o++) { outs[o].status = ost[o] ? ost[o] : rc; outs[o].out_bytes = 0; outs[o].out_blocks = 0; }
    }
    for (int o = 0; o < n_outs; o++)
        if (outs[o].status) return knz_set_error(h, outs[o].status, outs[o].status == KNZ_ERR_WRITE_FILE ? "destination buffer of an output too small" : "an output of the call failed (see its status and its parts')");
    return KNZ_OK;
}

extern "C" int knz_dev_concat(void* handle, const void* const* d_srcs, const uint64_t* n_bytes, int n, int64_t header_input_size, void* d_dst, uint64_t dst_cap,
                              uint64_t* out_bytes, void* hip_stream) {
    if (!handle || !out_bytes) return KNZ_ERR_MISSING_PARAM;
    *out_bytes = 0;
    if (n < 0) n = 0;
    if (n && (!d_srcs || !n_bytes)) return KNZ_ERR_MISSING_PARAM;
    std::vector<knz_splice_part> parts((size_t)n);
    for (int i = 0; i < n; i++) {
        memset(&parts[i], 0, sizeof(knz_splice_part));
        parts[i].d_src = d_srcs[i]; parts[i].n_bytes = n_bytes[i]; parts[i].from_block = 1; parts[i].to_block = KNZ_BLOCK_END;
    }
    knz_splice_out out;
    memset(&out, 0, sizeof(out));
    out.d_dst = d_dst; out.dst_cap = dst_cap; out.header_input_size = header_input_size;
    const int rc = knz_dev_splice_many(handle, parts.data(), n, &out, 1, hip_stream);
    *out_bytes = out.out_bytes;
    return rc;
}

extern "C" int knz_dev_slice(void* handle, const void* d_src, uint64_t n_bytes, uint32_t from_block, uint32_t to_block, int64_t header_input_size, void* d_dst,
                             uint64_t dst_cap, uint64_t* out_bytes, void* hip_stream) {
    if (!handle || !out_bytes) return KNZ_ERR_MISSING_PARAM;
    *out_bytes = 0;
    knz_splice_part part;
    memset(&part, 0, sizeof(part));
    part.d_src = d_src; part.n_bytes = n_bytes; part.from_block = from_block; part.to_block = to_block;
    knz_splice_out out;
    memset(&out, 0, sizeof(out));
    out.d_dst = d_dst; out.dst_cap = dst_cap; out.header_input_size = header_input_size;
    const int rc = knz_dev_splice_many(handle, &part, 1, &out, 1, hip_stream);
    *out_bytes = out.out_bytes;
    return rc;
}
