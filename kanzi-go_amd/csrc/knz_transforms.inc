// Host side of the transform pipeline: ByteTransformSequence.Forward / Inverse (v2/transform/Sequence.go:64-186) over a
// whole batch of blocks. Every stage runs for all blocks at once; a block whose stage declines (Forward error) keeps its
// previous bytes and its skip bit (Sequence.go:86-91); applied blocks ping-pong between two device regions.

static int seq_tokens(uint64_t t, uint32_t out[8]) {            // transform.New (Factory.go:58-95)
    int n = 0;
    for (int s = 42; s >= 0; s -= 6) { uint32_t id = (uint32_t)((t >> s) & 63); if (id) out[n++] = id; }
    if (n == 0) out[n++] = KNZ_T_NONE;
    return n;
}

struct XfBatch {
    uint32_t nblocks; uint64_t stride; uint32_t spb;            // region bytes per block, segments per block
    uint64_t* cur_ptr; uint32_t* cur_len; uint8_t* skip; uint8_t* side; uint8_t* active; uint8_t* take;
    uint64_t* out_ptr; uint32_t* out_len; int32_t* ok; int32_t* blk_status;
    uint8_t* blk_dt = nullptr;                                   // ctx["dataType"] per block (encode batches with a UTF stage), else null
    // ctx["entropy"] / ctx["blockSize"] of the STREAM the batch belongs to (the TEXT stage reads them, TextCodec.go:610-650, Factory.go:100-120):
    // the handle's configuration on the encode side, the stream header's values on the decode side; 0xFFFFFFFF = take the handle's
    uint32_t ctx_entropy = 0xFFFFFFFFu, ctx_block_size = 0;
    const uint8_t* piped = nullptr; int piped_zrlt = -1, piped_rank = -1;   // decode: blocks (and the two stages) the fused ZRLT / RANK inverse has already done (rank_pipe.hip)

    uint32_t cap() const { return (uint32_t)std::min<uint64_t>(stride, 0xFFFFFFFFu); }   // bytes a stage may write per block
    // the batch restricted to blocks g0 .. g0 + gn: every per-block table moves (workspaces indexed per group stay with the stage)
    XfBatch group(uint32_t g0, uint32_t gn) const {
        XfBatch g = *this;
        auto adv = [g0](auto*& p) { if (p) p += g0; };
        g.nblocks = gn; adv(g.cur_ptr); adv(g.cur_len); adv(g.skip); adv(g.side); adv(g.active); adv(g.take);
        adv(g.out_ptr); adv(g.out_len); adv(g.ok); adv(g.blk_status); adv(g.blk_dt); adv(g.piped);
        return g;
    }
    XfIo io() const { return XfIo{nblocks, spb, cur_ptr, cur_len, out_ptr, cap(), out_len, ok, active}; }
    template <typename Args> Args args() const { Args a; static_cast<XfIo&>(a) = io(); return a; }   // a stage's argument struct, its block tables filled
};

static int xf_alloc(Handle* h, XfBatch& x, uint32_t nblocks, uint64_t stride) {
    x.nblocks = nblocks; x.stride = stride; x.spb = (uint32_t)((stride + KNZ_SEG - 1) / KNZ_SEG);
    const size_t nb = (size_t)nblocks + 1;
    if (h->xf_r1.reserve(stride * nblocks + 256) || h->xf_r2.reserve(stride * nblocks + 256) || h->xf_outptr.reserve(8 * nb) ||
        h->xf_outlen.reserve(4 * nb) || h->xf_ok.reserve(4 * nb) || h->xf_side.reserve(nb) || h->xf_active.reserve(nb) ||
        h->xf_take.reserve(nb) || h->xf_sega.reserve((size_t)nblocks * x.spb * 256 * 4 + 64) ||
        h->xf_segb.reserve((size_t)nblocks * x.spb * 256 * 4 + 64) || h->xf_gstart.reserve(4 * (nb + 1)) || h->xf_misc.reserve(64 * nb))
        return -1;
    x.out_ptr = h->xf_outptr.as<uint64_t>(); x.out_len = h->xf_outlen.as<uint32_t>(); x.ok = h->xf_ok.as<int32_t>();
    x.side = h->xf_side.as<uint8_t>(); x.active = h->xf_active.as<uint8_t>(); x.take = h->xf_take.as<uint8_t>();
    return 0;
}

static CommitArgs xf_commit_args(Handle* h, const XfBatch& x, uint32_t stage) {
    CommitArgs c;
    c.nblocks = x.nblocks; c.stage = stage; c.ok = x.ok; c.out_len = x.out_len; c.out_ptr = x.out_ptr;
    c.cur_ptr = x.cur_ptr; c.cur_len = x.cur_len; c.skip = x.skip; c.side = x.side; c.target_if_side1 = 2; c.target_else = 1;
    c.base1 = (uint64_t)h->xf_r1.p; c.base2 = (uint64_t)h->xf_r2.p; c.stride = x.stride; c.blk_status = x.blk_status;
    return c;
}

static XfArgs xf_args(Handle* h, const XfBatch& x, uint32_t mode) {
    XfArgs a = x.args<XfArgs>();
    a.seg_a = h->xf_sega.as<int32_t>(); a.seg_b = h->xf_segb.as<int32_t>(); a.mode = mode;
    return a;
}

// ---- BWT forward for every active block: prefix-doubling suffix sort over the concatenated blocks (bwt_sort.hip) --------------
// One suffix sort covers at most 2^30 suffixes (slot numbers carry two flag bits in the lists): larger batches go through it
// in groups of consecutive blocks.
#define KNZ_BWT_GROUP_BLOCKS (1u << 20)
#define KNZ_BWT_GROUP_BYTES 0x40000001ull                  // (a group may hold 2^30 suffixes = the largest block of the format: slots 0 .. 2^30 - 1)
#define KNZ_SS_RUN_LIST_MAX (4u << 20)                      // large-list length from which its keys are run-aware

// entries of the normal list a workgroup takes per round = the largest group that list holds (bwt_sort.hip). The emulator build (tests) can
// run the small instantiations so that short inputs reach the large list and several rows per thread.
static uint32_t knz_sg_t() {
#ifdef KNZ_HIP_EMU
    if (const char* e = getenv("KNZ_EMU_SG_T")) { const int v = atoi(e); if (v == 128 || v == 256) return (uint32_t)v; }
#endif
    return KNZ_SG_T;
}
template <int T, int THREADS>
static void knz_sg_launch_sort(const SgArgs& sg, uint32_t nT, hipStream_t st) {
    hipLaunchKernelGGL((knz_sg_sort_kernel<T, THREADS>), dim3(nT), dim3(THREADS), 0, st, sg);
}

#ifdef KNZ_HIP_EMU
// TEST INFRASTRUCTURE (emulator build only, KNZ_EMU_SS_CHECK=1): invariants of the suffix sort between rounds. 'Device' memory is host memory here.
static bool ss_emu_check(const char* when, uint32_t total, uint32_t nb, const uint32_t* gstart, const uint32_t* sa, const uint32_t* rank,
                         const uint32_t* posN, uint32_t mN, const uint32_t* posL, const uint32_t* gidL, uint32_t mL, uint32_t T) {
    bool ok = true;
    std::vector<uint8_t> seen(total, 0), listed(total, 0);
    for (uint32_t b = 0; b < nb; b++)
        for (uint32_t j = gstart[b]; j < gstart[b + 1]; j++) {
            const uint32_t i = sa[j];
            if (i < gstart[b] || i >= gstart[b + 1] || seen[i]) { if (ok) fprintf(stderr, "ss check (%s): slot %u holds %u (block %u: %u..%u, seen %d)\n", when, j, i, b, gstart[b], gstart[b + 1], i < total ? seen[i] : -1); ok = false; }
            else seen[i] = 1;
        }
    auto walk = [&](const uint32_t* pos, uint32_t m, bool large) {
        uint32_t k = 0;
        while (k < m) {
            if (!(pos[k] & KNZ_SS_HEAD)) { if (ok) fprintf(stderr, "ss check (%s): %s list entry %u is not a head\n", when, large ? "large" : "normal", k); ok = false; k++; continue; }
            uint32_t e = k + 1;
            while (e < m && !(pos[e] & KNZ_SS_HEAD)) e++;
            const uint32_t size = e - k, j0 = pos[k] & KNZ_SS_MASK;
            if (size < 2 || (large ? size <= T : size > T)) { if (ok) fprintf(stderr, "ss check (%s): %s list group at %u has %u members\n", when, large ? "large" : "normal", k, size); ok = false; }
            for (uint32_t q = k; q < e; q++) {
                const uint32_t j = pos[q] & KNZ_SS_MASK;
                if (j != j0 + (q - k) || j >= total || listed[j]) { if (ok) fprintf(stderr, "ss check (%s): %s list entry %u: slot %u, group starts at slot %u\n", when, large ? "large" : "normal", q, j, j0); ok = false; continue; }
                listed[j] = 1;
                uint32_t b = 0;
                while (b + 1 < nb && gstart[b + 1] <= j) b++;
                while (gstart[b] == gstart[b + 1] && b + 1 < nb) b++;
                if (sa[j] < total && rank[sa[j]] != j0 - gstart[b] + 1) { if (ok) fprintf(stderr, "ss check (%s): rank of suffix %u is %u, its group starts at slot %u (block %u starts at %u)\n", when, sa[j], rank[sa[j]], j0, b, gstart[b]); ok = false; }
                if (large && gidL[q] != gidL[k]) { if (ok) fprintf(stderr, "ss check (%s): large entry %u has group id %u, its head %u\n", when, q, gidL[q], gidL[k]); ok = false; }
            }
            k = e;
        }
    };
    walk(posN, mN, false);
    walk(posL, mL, true);
    for (uint32_t b = 0; b < nb; b++)
        for (uint32_t j = gstart[b]; j < gstart[b + 1]; j++)
            if (!listed[j] && sa[j] < total && rank[sa[j]] != j - gstart[b] + 1) { if (ok) fprintf(stderr, "ss check (%s): resolved slot %u: suffix %u has rank %u\n", when, j, sa[j], rank[sa[j]]); ok = false; }
    return ok;
}
#endif

static unsigned knz_bits_for(uint64_t v) { unsigned b = 1; while ((1ull << b) <= v) b++; return b; }     // bits that hold the values 0..v

static int bwt_forward_group(Handle* h, const XfBatch& x, hipStream_t st, const uint32_t* lenG, const uint8_t* takeG) {   // x: the group's slice of the batch
    const uint32_t nb = x.nblocks;
    // geometry: blocks that do not take part get length 0 (gstart[b] == gstart[b+1], no radix tile)
    std::vector<uint32_t> geo(3 * (size_t)(nb + 1));
    uint32_t* gstart = geo.data(); uint32_t* tbase = gstart + (nb + 1); uint32_t* glen = tbase + (nb + 1);
    uint64_t total64 = 0, tiles64 = 0;
    uint32_t maxLen = 0;
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t l = takeG[b] ? lenG[b] : 0;
        gstart[b] = (uint32_t)total64; tbase[b] = (uint32_t)tiles64; glen[b] = l;
        total64 += l; tiles64 += (l + KNZ_RS_TILE - 1) / KNZ_RS_TILE;
        maxLen = std::max(maxLen, l);
    }
    gstart[nb] = (uint32_t)total64; tbase[nb] = (uint32_t)tiles64; glen[nb] = 0;
    if (total64 >= KNZ_BWT_GROUP_BYTES || nb > KNZ_BWT_GROUP_BLOCKS) return knz_set_error(h, KNZ_ERR_BLOCK_SIZE, "BWT group too large for one suffix sort");
    const uint32_t total = (uint32_t)total64, rtiles = (uint32_t)tiles64;
    if (total == 0) return KNZ_OK;
    const uint32_t ctilesMax = (total + 4095) / 4096;             // tiles of the classification kernels (flat, 4096 list entries)
    const uint32_t sgT = knz_sg_t();
    const size_t tileWords = 64 + 11 * (size_t)(ctilesMax + 2) + 2 * ((size_t)total / sgT + 4);
    const size_t histBytes = ((size_t)256 * rtiles * 4 + 255) & ~(size_t)255, sumsBytes = (((size_t)256 * rtiles / KNZ_RS_TILE + 2) * 4 + 255) & ~(size_t)255;
    if (h->sa_keys0.reserve(8 * (size_t)total + 64) || h->sa_keys1.reserve(8 * (size_t)total + 64) || h->sa_vals0.reserve(4 * (size_t)total + 64) ||
        h->sa_vals1.reserve(4 * (size_t)total + 64) || h->sa_rank.reserve(4 * (size_t)total + 64) || h->sa_hb.reserve(2 * 8 * ((size_t)ctilesMax + 2) * 64) ||
        h->sa_tiles.reserve(4 * tileWords) || h->sa_tmp.reserve(histBytes + sumsBytes + 256) || h->xf_gstart.reserve(4 * geo.size()))
        return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed (suffix sort)");
    HIP_OK(hipMemcpyAsync(h->xf_gstart.p, geo.data(), 4 * geo.size(), hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));                             // (geo is a host temporary)
    SsGeom g;
    g.nblocks = nb; g.gstart = h->xf_gstart.as<uint32_t>(); g.tile_base = g.gstart + (nb + 1); g.in_len = g.tile_base + (nb + 1); g.in_ptr = x.cur_ptr;
    uint64_t* kA = h->sa_keys0.as<uint64_t>(); uint64_t* kB = h->sa_keys1.as<uint64_t>();
    uint32_t* vA = h->sa_vals0.as<uint32_t>(); uint32_t* vB = h->sa_vals1.as<uint32_t>();
    uint32_t* rank = h->sa_rank.as<uint32_t>();
    uint64_t* hb = h->sa_hb.as<uint64_t>();
    uint64_t* rbits64 = hb + ((size_t)ctilesMax + 2) * 64;         // run bits of the text (made when the large list first gets short)
    bool runBitsReady = false;
    uint32_t* cnt = h->sa_tiles.as<uint32_t>();                  // 64 counter words, then the per-tile arrays
    uint32_t* tfirst = cnt + 64; uint32_t* tlast1 = tfirst + (ctilesMax + 2); uint32_t* prev1 = tlast1 + (ctilesMax + 2); uint32_t* nextf = prev1 + (ctilesMax + 2);
    uint32_t* cntN = nextf + (ctilesMax + 2); uint32_t* cntL = cntN + (ctilesMax + 2); uint32_t* cntLh = cntL + (ctilesMax + 2);
    uint32_t* rtfirst = cntLh + (ctilesMax + 2); uint32_t* rtlast1 = rtfirst + (ctilesMax + 2); uint32_t* rprev1 = rtlast1 + (ctilesMax + 2); uint32_t* rnextf = rprev1 + (ctilesMax + 2);
    uint32_t* tileA = rnextf + (ctilesMax + 2); uint32_t* tileCnt = tileA + ((size_t)total / sgT + 4);
    uint32_t* hist = h->sa_tmp.as<uint32_t>(); uint32_t* sums = (uint32_t*)(h->sa_tmp.as<uint8_t>() + histBytes);
    volatile uint32_t* pc = (volatile uint32_t*)((uint8_t*)h->pinned + 2048);
    const bool prof = knz_measure_switch("KNZ_BWT_PROF") != nullptr;          // diagnostics: unresolved suffixes per round
    // round 0: per-block radix sort of the first KNZ_SS_K0 symbols; the first pass reads the text
    const uint64_t* ks = nullptr; const uint32_t* vs = nullptr;
    int pr = probe_begin(h, st, "phase:bwt_sort_round0");
    for (unsigned p = 0; p < KNZ_SS_K0; p++) {
        uint64_t* kd = (p & 1) ? kB : kA; uint32_t* vd = (p & 1) ? vB : vA;
        if (p == 0) hipLaunchKernelGGL(knz_ss_hist_kernel<true>, dim3(rtiles), dim3(KNZ_RS_THREADS), 0, st, g, ks, 0u, hist);
        else hipLaunchKernelGGL(knz_ss_hist_kernel<false>, dim3(rtiles), dim3(KNZ_RS_THREADS), 0, st, g, ks, 8u * p, hist);
        knz_own_scan_excl_sum(hist, (uint64_t)256 * rtiles, sums, st);
        if (p == 0) hipLaunchKernelGGL(knz_ss_scatter_kernel<true>, dim3(rtiles), dim3(KNZ_RS_THREADS), 0, st, g, ks, vs, kd, vd, 0u, (const uint32_t*)hist);
        else hipLaunchKernelGGL(knz_ss_scatter_kernel<false>, dim3(rtiles), dim3(KNZ_RS_THREADS), 0, st, g, ks, vs, kd, vd, 8u * p, (const uint32_t*)hist);
        ks = kd; vs = vd;
    }
    probe_end(h, st, pr);
    pr = probe_begin(h, st, "phase:bwt_sort_classify");
    uint32_t* sa = (uint32_t*)vs;                                 // the suffix array under construction
    uint32_t* vfree = sa == vA ? vB : vA;                         // the other value buffer: input of the large list's sorts
    // groups -> head bits -> ranks and the two lists
    HIP_OK(hipMemsetAsync(cnt, 0, 64 * 4, st));
    hipLaunchKernelGGL(knz_ss_heads_kernel, dim3(ctilesMax), dim3(256), 0, st, g, ks, total, hb);
    SsClassArgs ca;
    ca.g = g; ca.hb = hb; ca.M = total; ca.lpos = nullptr; ca.sa = sa; ca.rank = rank; ca.prev1 = prev1; ca.nextf = nextf;
    ca.cnt_n = cntN; ca.cnt_l = cntL; ca.cnt_lh = cntLh; ca.base_n = cnt + 4; ca.pos_n = nullptr; ca.pos_l = nullptr; ca.gid_l = nullptr; ca.T = sgT;
    hipLaunchKernelGGL(knz_ss_tile_heads_kernel, dim3((ctilesMax + 3) / 4), dim3(256), 0, st, (const uint64_t*)hb, total, ctilesMax, tfirst, tlast1);
    hipLaunchKernelGGL(knz_ss_tile_scan_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t*)tfirst, (const uint32_t*)tlast1, ctilesMax, total, prev1, nextf);
    hipLaunchKernelGGL(knz_ss_class_count_kernel, dim3(ctilesMax), dim3(256), 0, st, ca);
    hipLaunchKernelGGL(knz_ss_scan_kernel, dim3(1), dim3(1024), 0, st, cntN, cntL, cntLh, ctilesMax, cnt + 5);
    HIP_OK(hipMemcpyAsync((void*)pc, cnt, 16 * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    uint32_t mN = pc[5], mL = pc[6], nLg = pc[7];
    // the lists are sized by what round 0 left (they only shrink afterwards; entries move from the large list to the normal one)
    const size_t listN = (size_t)mN + mL, listL = mL;
    if (h->sa_pos.reserve(4 * listN + 64) || h->sa_head.reserve(4 * listN + 64) || h->sa_gs.reserve(4 * listN + 64) || h->sa_posl0.reserve(4 * listL + 64) ||
        h->sa_posl1.reserve(4 * listL + 64) || h->sa_gid0.reserve(4 * listL + 64) || h->sa_gid1.reserve(4 * listL + 64) || h->sa_unres.reserve(4 * listL + 64))
        return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed (suffix sort lists)");
    uint32_t* posN = h->sa_pos.as<uint32_t>(); uint32_t* posN2 = h->sa_head.as<uint32_t>(); uint32_t* res = h->sa_gs.as<uint32_t>();
    uint32_t* posL = h->sa_posl0.as<uint32_t>(); uint32_t* posL2 = h->sa_posl1.as<uint32_t>();
    uint32_t* gidL = h->sa_gid0.as<uint32_t>(); uint32_t* gidL2 = h->sa_gid1.as<uint32_t>(); uint32_t* lvals = h->sa_unres.as<uint32_t>();
    ca.pos_n = posN; ca.pos_l = posL; ca.gid_l = gidL;
    hipLaunchKernelGGL(knz_ss_class_write_kernel<true>, dim3(ctilesMax), dim3(256), 0, st, ca);
    probe_end(h, st, pr);
#ifdef KNZ_HIP_EMU
    const bool chk = getenv("KNZ_EMU_SS_CHECK") != nullptr;
    if (chk && !ss_emu_check("round 0", total, nb, gstart, sa, rank, posN, mN, posL, gidL, mL, sgT)) return knz_set_error(h, KNZ_ERR_UNKNOWN, "suffix sort check failed");
#endif
    if (prof) fprintf(stderr, "suffix sort: %u suffixes, after %d symbols: %u in groups of 2..%u, %u in %u larger groups\n", total, KNZ_SS_K0, mN, sgT, mL, nLg);
    unsigned runBitsPad = 0;
    if (const char* e = knz_test_switch("KNZ_SS_RUN_BITS_PAD")) runBitsPad = (unsigned)std::max(0, atoi(e));   // (tests: the width decision of blocks >= 64 MiB on small inputs)
    for (uint64_t hstep = KNZ_SS_K0; mN + mL > 0; hstep *= 2) {
        if (hstep > 2 * (uint64_t)maxLen + 16) return knz_set_error(h, KNZ_ERR_UNKNOWN, "suffix sort did not converge");
        const uint32_t hs = (uint32_t)std::min<uint64_t>(hstep, 0x7FFFFFFFu);
        const unsigned rbits = knz_bits_for((uint64_t)maxLen + std::min<uint64_t>(hstep, maxLen) + 1);
        pr = probe_begin(h, st, "phase:bwt_sort_doubling");
        HIP_OK(hipMemsetAsync(cnt + 4, 0, 4 * 4, st));             // [4] normal entries that stay, [5..7] what the large list hands over / keeps
        SgArgs sg;
        sg.prof = (unsigned long long*)(cnt + 32);
        sg.g = g; sg.m = mN; sg.pos = posN; sg.sa = sa; sg.rank = rank; sg.res = res; sg.tile_a = tileA; sg.tile_cnt = tileCnt; sg.pos_out = posN2;
        sg.tile_off = tileCnt; sg.h = hs; sg.rbits = rbits; sg.err = (int32_t*)(cnt + 8);
        const uint32_t nT = (mN + sgT - 1) / sgT;
        sg.key2 = (const uint32_t*)kA; sg.suf = (const uint32_t*)kA + mN;     // (kA is free until the large list's keys are made, behind the sort)
        if (mN) {
            hipLaunchKernelGGL(knz_sg_keys_kernel, dim3((mN + 255) / 256), dim3(256), 0, st, g, (const uint32_t*)posN, mN, (const uint32_t*)sa, (const uint32_t*)rank, hs,
                               (uint32_t*)kA, (uint32_t*)kA + mN);
#ifdef KNZ_HIP_EMU
            if (sgT == 128) knz_sg_launch_sort<128, 256>(sg, nT, st);
            else if (sgT == 256) knz_sg_launch_sort<256, 256>(sg, nT, st);
            else
#endif
            knz_sg_launch_sort<KNZ_SG_T, KNZ_SG_THREADS>(sg, nT, st);
            hipLaunchKernelGGL(knz_ss_scan_kernel, dim3(1), dim3(1024), 0, st, tileCnt, (uint32_t*)nullptr, (uint32_t*)nullptr, nT, cnt + 4);
        }
        // large list: run-aware keys once it is short (bwt_sort.hip): a long run of one symbol is resolved in one round instead of log2(run / h)
        // the sort key is (group id : gbits | payload : pbits) in 64 bits. The run-aware payload needs 1 + lbits + rkbits bits: at 64 MiB
        // blocks and beyond that no longer fits beside an 11-bit group id, and the list falls back to the plain doubling keys (rbits <= 33).
        const unsigned gbits = nLg > 1 ? knz_bits_for(nLg - 1) : 0;
        const unsigned runBits = 1 + knz_bits_for(maxLen) + knz_bits_for((uint64_t)maxLen + 1) + runBitsPad;
        const bool runKeys = mL > 0 && mL <= KNZ_SS_RUN_LIST_MAX && std::max(rbits, runBits) + gbits <= 64;
        unsigned pbits = rbits;
        if (mL) {
            SlKeyArgs ka;
            ka.g = g; ka.lpos = posL; ka.gid = gidL; ka.m = mL; ka.sa = sa; ka.rank = rank; ka.h = hs; ka.rb = nullptr; ka.rnextf = nullptr; ka.total = total;
            ka.lmax = maxLen; ka.lbits = knz_bits_for(maxLen); ka.rkbits = knz_bits_for((uint64_t)maxLen + 1); ka.keys = kA; ka.vals = vfree;
            if (runKeys) {
                if (!runBitsReady) {
                    hipLaunchKernelGGL(knz_ss_run_bits_kernel, dim3(ctilesMax), dim3(256), 0, st, g, total, rbits64);
                    hipLaunchKernelGGL(knz_ss_tile_heads_kernel, dim3((ctilesMax + 3) / 4), dim3(256), 0, st, (const uint64_t*)rbits64, total, ctilesMax, rtfirst, rtlast1);
                    hipLaunchKernelGGL(knz_ss_tile_scan_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t*)rtfirst, (const uint32_t*)rtlast1, ctilesMax, total, rprev1, rnextf);
                    runBitsReady = true;
                }
                ka.rb = rbits64; ka.rnextf = rnextf;
                pbits = std::max<unsigned>(rbits, 1 + ka.lbits + ka.rkbits);
            }
            ka.pbits = pbits;
            hipLaunchKernelGGL(knz_sl_keys_kernel, dim3((mL + 255) / 256), dim3(256), 0, st, ka);
        }
        if (mN) hipLaunchKernelGGL((knz_sg_update_kernel<KNZ_SG_THREADS>), dim3(nT), dim3(KNZ_SG_THREADS), 0, st, sg, nT);
        if (mL) {
            if (pbits + gbits > 64) return knz_set_error(h, KNZ_ERR_UNKNOWN, "suffix sort: key wider than 64 bits");
            if (knz_sort_pairs_u64(h->sa_tmp, kA, kB, vfree, lvals, mL, 0, pbits + gbits, st)) return knz_set_error(h, KNZ_ERR_UNKNOWN, "radix sort failed");
            const uint32_t lt = (mL + 4095) / 4096;
            hipLaunchKernelGGL(knz_sl_writeback_kernel, dim3(lt), dim3(256), 0, st, (const uint32_t*)posL, mL, (const uint64_t*)kB, (const uint32_t*)lvals, sa, hb);
            SsClassArgs cl = ca;
            cl.M = mL; cl.lpos = posL; cl.pos_n = posN2; cl.pos_l = posL2; cl.gid_l = gidL2;
            hipLaunchKernelGGL(knz_ss_tile_heads_kernel, dim3((lt + 3) / 4), dim3(256), 0, st, (const uint64_t*)hb, mL, lt, tfirst, tlast1);
            hipLaunchKernelGGL(knz_ss_tile_scan_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t*)tfirst, (const uint32_t*)tlast1, lt, mL, prev1, nextf);
            hipLaunchKernelGGL(knz_ss_class_count_kernel, dim3(lt), dim3(256), 0, st, cl);
            hipLaunchKernelGGL(knz_ss_scan_kernel, dim3(1), dim3(1024), 0, st, cntN, cntL, cntLh, lt, cnt + 5);
            hipLaunchKernelGGL(knz_ss_class_write_kernel<false>, dim3(lt), dim3(256), 0, st, cl);
        }
        probe_end(h, st, pr);
        HIP_OK(hipMemcpyAsync((void*)pc, cnt, 16 * 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (pc[8]) return knz_set_error(h, KNZ_ERR_UNKNOWN, "suffix sort: group larger than a segment on the normal list");
        mN = pc[4] + pc[5]; mL = pc[6]; nLg = pc[7];
        std::swap(posN, posN2); std::swap(posL, posL2); std::swap(gidL, gidL2);
#ifdef KNZ_HIP_EMU
        if (chk && !ss_emu_check("doubling", total, nb, gstart, sa, rank, posN, mN, posL, gidL, mL, sgT)) {
            fprintf(stderr, "  (after the round with h = %llu)\n", (unsigned long long)hstep);
            return knz_set_error(h, KNZ_ERR_UNKNOWN, "suffix sort check failed");
        }
#endif
#ifdef KNZ_SG_PROF
        if (prof) {
            unsigned long long pv[16];
            hipMemcpy(pv, cnt + 32, sizeof(pv), hipMemcpyDeviceToHost);
            fprintf(stderr, "   sg_sort cycles/tile: window %llu gather+groups %llu sort %llu heads %llu write %llu | passes/tile %.2f items/tile %.0f groups/tile %.0f tiles %llu\n",
                    pv[0] / std::max(1ull, pv[7]), pv[1] / std::max(1ull, pv[7]), pv[2] / std::max(1ull, pv[7]), pv[3] / std::max(1ull, pv[7]), pv[4] / std::max(1ull, pv[7]),
                    (double)pv[5] / std::max(1ull, pv[7]), (double)pv[6] / std::max(1ull, pv[7]), (double)pv[8] / std::max(1ull, pv[7]), pv[7]);
            hipMemset(cnt + 32, 0, 16 * 8);
        }
#endif
        if (prof) fprintf(stderr, "suffix sort: h %llu -> %u in groups of 2..%u, %u in %u larger groups\n", (unsigned long long)hstep, mN, sgT, mL, nLg);
    }
    const XfIo io = x.io();
    BwtOutArgs oa; oa.g.nblocks = io.nblocks; oa.g.gstart = g.gstart; oa.g.in_ptr = io.in_ptr; oa.g.in_len = g.in_len; oa.g.active = x.take;
    oa.sa = sa; oa.rank = rank; oa.out_ptr = io.out_ptr; oa.out_cap = io.out_cap; oa.out_len = io.out_len; oa.ok = io.ok;
    KNZ_LAUNCH_PROBED(knz_bwt_output_kernel, dim3((total + 255) / 256), dim3(256), 0, st, oa, total);
    return KNZ_OK;
}

static int bwt_inverse_group(Handle* h, const XfBatch& x, hipStream_t st) {   // x: the group's slice of the batch
    const uint32_t nb = x.nblocks;
    const XfIo io = x.io();
    BwtInvArgs a;
    a.nblocks = io.nblocks; a.gstart = h->xf_gstart.as<uint32_t>(); a.in_ptr = io.in_ptr; a.in_len = io.in_len; a.active = io.active;
    a.hdr = (uint32_t*)((uint8_t*)h->xf_misc.p + 16 * (size_t)(nb + 1)); a.out_ptr = io.out_ptr; a.out_cap = io.out_cap; a.out_len = io.out_len; a.ok = io.ok;
    uint32_t* d_plen = (uint32_t*)h->xf_misc.p;
    hipLaunchKernelGGL(knz_bwt_inv_header_kernel, dim3((nb + 63) / 64), dim3(64), 0, st, a, d_plen);
    std::vector<uint32_t> plen(nb), gstart(nb + 1);
    HIP_OK(hipMemcpyAsync(plen.data(), d_plen, 4 * (size_t)nb, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    uint64_t total64 = 0;
    for (uint32_t b = 0; b < nb; b++) { gstart[b] = (uint32_t)total64; total64 += plen[b]; }
    gstart[nb] = (uint32_t)total64;
    if (total64 >= 0xFFFFFFF0ull || nb >= (1u << 24)) return knz_set_error(h, KNZ_ERR_BLOCK_SIZE, "BWT batch too large");
    const uint32_t total = (uint32_t)total64;
    if (total == 0) return KNZ_OK;
    HIP_OK(hipMemcpyAsync(h->xf_gstart.p, gstart.data(), 4 * (size_t)(nb + 1), hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
    if (h->sa_vals0.reserve(4 * (size_t)total) || h->sa_vals1.reserve(4 * (size_t)total) || h->sa_gs.reserve(4 * (size_t)total) ||
        h->sa_head.reserve(4 * (size_t)total) || h->sa_links.reserve(8 * (size_t)total + 64))
        return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed (inverse BWT)");
    uint32_t* k0 = h->sa_gs.as<uint32_t>(); uint32_t* k1 = h->sa_head.as<uint32_t>();
    uint32_t* v0 = h->sa_vals0.as<uint32_t>(); uint32_t* v1 = h->sa_vals1.as<uint32_t>();
    const unsigned grid = (total + 255) / 256;
    hipLaunchKernelGGL(knz_bwt_inv_keys_kernel, dim3(grid), dim3(256), 0, st, a, total, k0, v0);
    unsigned bits = 8;
    while ((1ull << (bits - 8)) < nb) bits++;
    if (knz_sort_pairs_u32(h->sa_tmp, k0, k1, v0, v1, total, 0, bits, st)) return knz_set_error(h, KNZ_ERR_UNKNOWN, "radix sort failed");
    hipLaunchKernelGGL(knz_bwt_inv_links_kernel, dim3(grid), dim3(256), 0, st, a, total, k1, v1, h->sa_links.as<uint2>());
    // links -> 2 symbols per hop -> 4 symbols per hop (two gather passes), then the chains
    if (h->sa_keys0.reserve(8 * (size_t)total + 64) || h->sa_keys1.reserve(8 * (size_t)total + 64))
        return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed (inverse BWT)");
    hipLaunchKernelGGL(knz_bwt_inv_double_kernel, dim3(grid), dim3(256), 0, st, a, total, k1, (const uint2*)h->sa_links.as<uint2>(), h->sa_keys0.as<uint2>(), 8u);
    hipLaunchKernelGGL(knz_bwt_inv_double_kernel, dim3(grid), dim3(256), 0, st, a, total, k1, (const uint2*)h->sa_keys0.as<uint2>(), h->sa_keys1.as<uint2>(), 16u);
    // list ranking with splitters for the blocks that are large enough (bwt.hip); the chains kernel takes the rest and any block the
    // ranking rejects (damaged stream)
    const char* rmin = knz_test_switch("KNZ_BWT_RANK_MIN");                                           // (tests: small blocks through the ranking too)
    const uint32_t rankMin = rmin ? (uint32_t)atoi(rmin) : 65536u;
    std::vector<uint32_t> spBase(nb + 1);
    std::vector<uint8_t> useChain(nb);
    uint64_t totalSp = 0;
    for (uint32_t b = 0; b < nb; b++) {
        spBase[b] = (uint32_t)totalSp;
        const bool ranked = plen[b] >= rankMin && plen[b] >= 256;                            // (8 chunk chains from 256 bytes on)
        useChain[b] = ranked ? 0 : 1;
        if (ranked) totalSp += (plen[b] + KNZ_BWT_SPLIT - 1) / KNZ_BWT_SPLIT + 8;
    }
    spBase[nb] = (uint32_t)totalSp;
    const size_t ucBytes = ((size_t)nb + 255) & ~(size_t)255, baseBytes = (4 * (size_t)(nb + 1) + 255) & ~(size_t)255;
    if (h->sa_sp.reserve(ucBytes + baseBytes + 6 * 4 * (size_t)totalSp + 256))
        return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed (inverse BWT)");
    uint8_t* d_useChain = h->sa_sp.as<uint8_t>();
    uint32_t* base = (uint32_t*)(h->sa_sp.as<uint8_t>() + ucBytes);
    HIP_OK(hipMemcpyAsync(d_useChain, useChain.data(), nb, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(base, spBase.data(), 4 * (size_t)(nb + 1), hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
    if (totalSp) {
        BwtRankArgs r;
        r.a = a; r.links = (const uint2*)h->sa_links.as<uint2>(); r.links4 = (const uint2*)h->sa_keys1.as<uint2>(); r.sp_base = base;
        uint32_t* arr = (uint32_t*)(h->sa_sp.as<uint8_t>() + ucBytes + baseBytes);
        r.sp_succ = arr; r.sp_len = arr + totalSp; r.sp_succ2 = arr + 2 * totalSp; r.sp_dist = arr + 3 * totalSp; r.sp_dist2 = arr + 4 * totalSp;
        r.sp_pos = arr + 5 * totalSp; r.use_chain = d_useChain;
        const unsigned gsp = (unsigned)((totalSp + 255) / 256);
        KNZ_LAUNCH_PROBED(knz_bwt_inv_walk_kernel, dim3(gsp), dim3(256), 0, st, r, (uint32_t)totalSp);
        KNZ_LAUNCH_PROBED(knz_bwt_inv_rank_kernel, dim3(nb), dim3(1024), 0, st, r);
        KNZ_LAUNCH_PROBED(knz_bwt_inv_emit_kernel, dim3(gsp), dim3(256), 0, st, r, (uint32_t)totalSp);
    }
    KNZ_LAUNCH_PROBED(knz_bwt_inv_chains_kernel, dim3(nb), dim3(64), 0, st, a, (const uint2*)h->sa_links.as<uint2>(), (const uint2*)h->sa_keys1.as<uint2>(), (const uint8_t*)d_useChain);
    return KNZ_OK;
}

// Both directions take the batch in groups of consecutive blocks, by input length (inverse: header included, an upper bound of the payload)
static int bwt_stage(Handle* h, XfBatch& x, uint32_t, bool forward, hipStream_t st) {
    const uint32_t nb = x.nblocks;
    std::vector<uint32_t> len(nb);
    std::vector<uint8_t> take(nb, 1);
    if (forward) hipLaunchKernelGGL(knz_bwt_precheck_kernel, dim3((nb + 63) / 64), dim3(64), 0, st, nb, x.cur_len, x.active, x.cap(), x.take, x.ok);
    HIP_OK(hipMemcpyAsync(len.data(), x.cur_len, 4 * (size_t)nb, hipMemcpyDeviceToHost, st));
    if (forward) HIP_OK(hipMemcpyAsync(take.data(), x.take, nb, hipMemcpyDeviceToHost, st));   // (the inverse takes every block of the batch)
    HIP_OK(hipStreamSynchronize(st));
    for (uint32_t g0 = 0; g0 < nb;) {
        uint32_t gn = 0;
        uint64_t tot = 0;
        while (g0 + gn < nb && gn < KNZ_BWT_GROUP_BLOCKS) {
            const uint64_t add = take[g0 + gn] ? len[g0 + gn] : 0;
            if (gn > 0 && tot + add >= KNZ_BWT_GROUP_BYTES) break;
            tot += add; gn++;
        }
        const int rc = forward ? bwt_forward_group(h, x.group(g0, gn), st, len.data() + g0, take.data() + g0) : bwt_inverse_group(h, x.group(g0, gn), st);
        if (rc) return rc;
        g0 += gn;
    }
    return KNZ_OK;
}

// ---- TEXT (text.hip) -------------------------------------------------------------------------------------------------------
// Static dictionary tables for the device: createDictionary (TextCodec.go:451-490) over the 1024-word list. hash | data | offset | letters.
static int text_upload_static(Handle* h, hipStream_t st) {
    if (h->text_stat_ready) return 0;
    static const char words[] =
#include "text_dict.inc"
        ;
    const size_t nl = sizeof(words) - 1;
    if (nl + 32 > KNZ_TC_LETTERS_PAD) return -1;
    std::vector<uint32_t> tab(3 * KNZ_TC_STATIC + KNZ_TC_LETTERS_PAD / 4, 0);
    uint8_t* letters = (uint8_t*)(tab.data() + 3 * KNZ_TC_STATIC);
    memcpy(letters, words, nl);
    uint32_t nw = 0, anchor = 0, hsh = KNZ_TC_HASH1;
    auto put = [&](uint32_t end) { tab[nw] = hsh; tab[KNZ_TC_STATIC + nw] = ((end - anchor) << 24) | nw; tab[2 * KNZ_TC_STATIC + nw] = anchor; nw++; };
    for (uint32_t i = 0; i < nl && nw < KNZ_TC_STATIC; i++) {
        if (letters[i] >= 'A' && letters[i] <= 'Z') {
            if (i > anchor) { put(i); anchor = i; hsh = KNZ_TC_HASH1; }
            letters[i] ^= 0x20;
        }
        hsh = (hsh * KNZ_TC_HASH1) ^ ((uint32_t)letters[i] * KNZ_TC_HASH2);
    }
    if (nw < KNZ_TC_STATIC) put((uint32_t)nl);
    if (nw != KNZ_TC_STATIC) return -1;
    if (h->text_stat.reserve(tab.size() * 4)) return -1;
    if (hipMemcpyAsync(h->text_stat.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    if (hipStreamSynchronize(st) != hipSuccess) return -1;                // (tab is a local)
    h->text_stat_ready = true;
    return 0;
}

// Factory.go:100-120: the stream format follows the entropy stage ; TextCodec.go:610-650 / :1137-1188: the hash table size follows ctx["blockSize"]
static void text_params(uint32_t entropy, uint32_t block_size, uint32_t& kind, uint32_t& logHash) {
    kind = (entropy == KNZ_E_NONE || entropy == KNZ_E_HUFFMAN || entropy == 4u /* RANGE */ || entropy == KNZ_E_ANS0) ? 2u : 1u;
    uint32_t lg = 13;
    auto ilog2 = [](uint32_t v) { uint32_t l = 0; while (v > 1) { v >>= 1; l++; } return l; };
    if (kind == 1) { if (block_size >= 8) lg = std::min(26u, std::max(13u, ilog2(block_size / 8))); }
    else if (block_size >= 32) lg = std::min(24u, std::max(13u, ilog2(block_size / 32)));
    if (entropy == 9u /* TPAQX */) lg++;
    logHash = lg;
}

static int text_stage(Handle* h, XfBatch& x, uint32_t, bool forward, hipStream_t st) {
    const uint32_t nb = x.nblocks;
    uint32_t kind, logHash;
    // the stream's own ctx values, not the handle's: a stream is decoded with what ITS header says (the reference builds the codec from the
    // stream's ctx["entropy"] / ctx["blockSize"], CompressedStream.go:1483-1522)
    text_params(x.ctx_entropy == 0xFFFFFFFFu ? h->cfg.entropy : x.ctx_entropy, x.ctx_entropy == 0xFFFFFFFFu ? h->cfg.block_size : x.ctx_block_size, kind, logHash);
    if (text_upload_static(h, st)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "static dictionary upload failed (TEXT)");
    const bool par = knz_test_switch("KNZ_TEXT_CHAIN") == nullptr;         // (KNZ_TEXT_CHAIN: tests run the one-lane scan alone)
    // bounded groups of blocks: one hash table (4 << logHash bytes), 2^19 entries (6 MiB) and the parallel form's token / position arrays
    // (22 bytes per possible token, 2 bytes per position) per block, at most ~3 GiB per group
    const uint64_t tokStride = (x.stride / 3 + 64 + 15) & ~(uint64_t)15, posStride = (x.stride + 64 + 15) & ~(uint64_t)15;
    const uint64_t perBlock = ((uint64_t)4 << logHash) + (uint64_t)12 * KNZ_TC_MAX_DICT + (par ? 22 * tokStride + 2 * posStride + 4 * (uint64_t)KNZ_TC_MAX_DICT : 0);
    const uint32_t G = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(nb, 64), ((uint64_t)3 << 30) / perBlock));
    if (h->text_cnt.reserve(16)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed (TEXT)");
    HIP_OK(hipMemsetAsync(h->text_cnt.p, 0, 16, st));
    if (h->text_map.reserve(((size_t)G << logHash) * 4) || h->text_ent.reserve((size_t)G * 12 * KNZ_TC_MAX_DICT) || h->text_mode.reserve((size_t)nb * 4 + 64) ||
        (par && (h->text_tok.reserve((size_t)G * 22 * tokStride + 64) || h->text_pos.reserve((size_t)G * 2 * posStride + 64) ||
                 h->text_instok.reserve((size_t)G * 4 * KNZ_TC_MAX_DICT))))
        return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed (TEXT)");
    for (uint32_t g0 = 0; g0 < nb; g0 += G) {
        const uint32_t gn = std::min<uint32_t>(G, nb - g0);
        const XfBatch g = x.group(g0, gn);
        TextArgs a = g.args<TextArgs>();
        a.blk_dt = g.blk_dt;
        a.tmode = h->text_mode.as<int32_t>() + g0; a.dict_map = h->text_map.as<int32_t>(); a.ent = h->text_ent.as<uint32_t>();
        a.stat = h->text_stat.as<uint32_t>(); a.log_hash = logHash; a.kind = kind; a.chain_count = h->text_cnt.as<uint32_t>();
        TextParArgs pa;
        if (par) {
            pa.a = a; pa.tok_stride = tokStride; pa.pos_stride = posStride;
            uint8_t* tb = h->text_tok.as<uint8_t>();
            const size_t tn = (size_t)G * tokStride;
            pa.tok_end = (uint32_t*)tb; pa.tok_h1 = pa.tok_end + tn; pa.tok_h2 = pa.tok_h1 + tn; pa.tok_p = pa.tok_h2 + tn; pa.tok_ref = pa.tok_p + tn;
            pa.tok_len = (uint8_t*)(pa.tok_ref + tn); pa.tok_ins = pa.tok_len + tn;
            pa.mark = h->text_pos.as<uint8_t>(); pa.refb = pa.mark + (size_t)G * posStride; pa.ins_tok = h->text_instok.as<uint32_t>();
            pa.prof = nullptr;
            if (knz_measure_switch("KNZ_TEXT_PROF") != nullptr) {               // diagnostics: phase time stamps of the forward kernel to stderr
                if (h->text_prof.reserve((size_t)G * 64)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed (TEXT)");
                HIP_OK(hipMemsetAsync(h->text_prof.p, 0, (size_t)G * 64, st));
                pa.prof = (unsigned long long*)h->text_prof.p;
            }
        }
        // the chain kernels take the blocks the parallel ones left (no fixed point within their rounds, a dictionary that wraps) and the
        // KNZ_TEXT_CHAIN runs
        if (forward) hipLaunchKernelGGL(knz_text_stats_kernel, dim3(gn), dim3(256), 0, st, a);
        else HIP_OK(hipMemsetAsync(a.tmode, 0, (size_t)gn * 4, st));
        if (par && forward) KNZ_LAUNCH_PROBED(knz_text_forward_par_kernel, dim3(gn), dim3(KNZ_TCP_THREADS), 0, st, pa);
        if (par && !forward) KNZ_LAUNCH_PROBED(knz_text_inverse_par_kernel, dim3(gn), dim3(KNZ_TCP_THREADS), 0, st, pa);
        if (par && pa.prof) {
            std::vector<unsigned long long> pr((size_t)gn * 8);
            HIP_OK(hipStreamSynchronize(st));
            HIP_OK(hipMemcpy(pr.data(), pa.prof, pr.size() * 8, hipMemcpyDeviceToHost));
            for (uint32_t q = 0; q < gn; q++) {
                const unsigned long long* r = pr.data() + (size_t)q * 8;
                if (r[4] && forward) fprintf(stderr, "TEXT block %u: tokens %llu rounds %llu cycles A %llu B %llu C %llu D %llu\n", g0 + q, r[7], r[6], r[1] - r[0], r[2] - r[1], r[3] - r[2], r[4] - r[3]);
                if (r[4] && !forward) fprintf(stderr, "TEXT inverse block %u: tokens %llu cycles I %llu II %llu III %llu IV %llu\n", g0 + q, r[7], r[1] - r[0], r[2] - r[1], r[3] - r[2], r[4] - r[3]);
            }
        }
        HIP_OK(hipMemsetAsync(h->text_map.p, 0xFF, ((size_t)gn << logHash) * 4, st));
        if (forward) KNZ_LAUNCH_PROBED(knz_text_forward_chain_kernel, dim3(gn), dim3(64), 0, st, a);
        else KNZ_LAUNCH_PROBED(knz_text_inverse_chain_kernel, dim3(gn), dim3(64), 0, st, a);
    }
    return KNZ_OK;
}

// Second form of the LZ / LZX forward stage (lz_par.hip): candidates and common prefixes of all positions by one stable sort, then the parse.
// Returns 0 when it ran, 1 when the batch does not fit (one sort, or the workspace: the caller takes the first form), 2 on a HIP error.
static int lz_forward_par(Handle* h, XfBatch& x, const LzArgs& la, unsigned hashLog, hipStream_t st) {
    const uint32_t nb = x.nblocks;
    std::vector<uint32_t> len(nb), gstart(nb + 1);
    std::vector<uint8_t> act(nb);
    if (hipMemcpyAsync(len.data(), x.cur_len, 4 * (size_t)nb, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(act.data(), x.active, nb, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return 2;
    uint64_t total64 = 0;
    uint32_t maxPlen = 0;
    for (uint32_t b = 0; b < nb; b++) {
        gstart[b] = (uint32_t)total64;
        const uint32_t plen = (act[b] && len[b] >= KNZ_LZ_MIN_BLOCK) ? len[b] - 16 : 0;
        total64 += plen;
        maxPlen = std::max(maxPlen, plen);
        if (total64 >= 0xFFFFFFF0ull) return 1;
    }
    gstart[nb] = (uint32_t)total64;
    const uint32_t total = (uint32_t)total64;
    unsigned blkBits = 0;
    while ((1ull << blkBits) < nb) blkBits++;
    if (hashLog + blkBits > 32) return 1;
    const uint64_t holeStride = ((x.stride >> 5) + 4 + 3) & ~(uint64_t)3;         // (a multiple of 4 words: knz_lzs_compare_kernel reads the maps 16 bytes at a time)
    if (h->lz_gstart.reserve(4 * (size_t)(nb + 1)) || h->lz_k0.reserve(4 * (size_t)total + 64) || h->lz_k1.reserve(4 * (size_t)total + 64) ||
        h->lz_v0.reserve(4 * (size_t)total + 64) || h->lz_v1.reserve(4 * (size_t)total + 64) || h->lz_cand.reserve(4 * (size_t)total + 64) ||
        h->lz_cp.reserve((size_t)total + 64) || h->lz_holes.reserve((size_t)nb * holeStride * 4 + 64))
        { (void)hipGetLastError(); return 1; }                     // does not fit: the caller takes the first form (and the sticky allocation error is cleared)
    if (hipMemcpyAsync(h->lz_gstart.p, gstart.data(), 4 * (size_t)(nb + 1), hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return 2;
    if (hipMemsetAsync(h->lz_holes.p, 0, (size_t)nb * holeStride * 4, st) != hipSuccess) return 2;
    LzPreArgs pre;
    pre.nblocks = nb; pre.in_ptr = x.cur_ptr; pre.in_len = x.cur_len; pre.active = x.active; pre.gstart = h->lz_gstart.as<uint32_t>(); pre.hash_log = hashLog;
    pre.keys = h->lz_k0.as<uint32_t>(); pre.vals = h->lz_v0.as<uint32_t>(); pre.cand = h->lz_cand.as<uint32_t>(); pre.cp8 = h->lz_cp.as<uint8_t>();
    if (total) {
        hipLaunchKernelGGL(knz_lz_keys_kernel, dim3((maxPlen + 255) / 256, nb), dim3(256), 0, st, pre);
        // (sorted by block : hash. By the hash bits alone - the sort is stable, the groups of a block would still sit side by side - the sort is a pass shorter, 1.6 ms, and
        // knz_lz_cand_kernel, whose writes then scatter over the candidates of ALL blocks, 4.4 ms longer: measured in round 6)
        if (knz_sort_pairs_u32(h->sa_tmp, h->lz_k0.as<uint32_t>(), h->lz_k1.as<uint32_t>(), h->lz_v0.as<uint32_t>(), h->lz_v1.as<uint32_t>(), total, 0, hashLog + blkBits, st))
            return 2;
        hipLaunchKernelGGL(knz_lz_cand_kernel, dim3((total + 255) / 256), dim3(256), 0, st, pre, (const uint32_t*)h->lz_k1.as<uint32_t>(), (const uint32_t*)h->lz_v1.as<uint32_t>(), total);
        hipLaunchKernelGGL(knz_lz_cp_kernel, dim3((maxPlen + 255) / 256, nb), dim3(256), 0, st, pre);
    }
    LzParArgs pa;
    pa.a = la; pa.gstart = h->lz_gstart.as<uint32_t>(); pa.cand = h->lz_cand.as<uint32_t>(); pa.cp8 = h->lz_cp.as<uint8_t>();
    pa.holes = h->lz_holes.as<uint32_t>(); pa.hole_stride = holeStride;
    pa.prof = nullptr;
    h->lzs_n = 0; h->lzs_rounds = 0;
    if (knz_test_switch("KNZ_LZ_ONE_WAVE") == nullptr) {                               // third form: segments side by side, iterated to the fixed point (lz_fwd_seg.hip)
        const char* sv = knz_test_switch("KNZ_LZ_SEG");                               // (tests: small segments on small inputs)
        // round 6: one LANE per segment (short segments, every live segment of a block with holes in every round); KNZ_LZS_WAVES = one wave per segment
        // with the query log and the carried map stretches (rounds 3-5), kept as a second form for the tests and for A/B
        const bool lanes = knz_test_switch("KNZ_LZS_WAVES") == nullptr;
        const uint32_t segSize = sv ? std::max(64u, (uint32_t)atoi(sv)) : (lanes ? KNZ_LZS_LANE_SEG : KNZ_LZS_SEG);
        uint32_t maxLen = 0;                                               // (over the blocks that take part: inactive ones must not size the workspace)
        for (uint32_t b = 0; b < nb; b++) if (act[b]) maxLen = std::max(maxLen, len[b]);
        const uint32_t segs = std::max(1u, (maxLen + segSize - 1) / segSize);
        const char* wv = knz_measure_switch("KNZ_LZ_WARM");                              // (measurements: warm-up of the first guess, positions)
        const uint32_t warm = std::min<uint32_t>(wv ? (uint32_t)atoi(wv) : 0u, segSize);   // measured on S-silesia: 0, 1024, 4096 all settle in the same rounds (5); record-shaped data settles SLOWER with a warm-up (repeat distances lock in differently)
        const uint32_t tokCap = (segSize + warm) / 4 + 4;
        const size_t nseg = (size_t)nb * segs;
        const uint64_t ms = holeStride;
        // lzs_state: entry | used | exit (5 words each) | ntok | segsum (4 words) | need (bytes)
        if (h->lzs_state.reserve(nseg * (15 + 1 + 4) * 4 + nseg + 64) || h->lzs_tok.reserve(nseg * tokCap * 16 + 64) ||
            h->lzs_maps.reserve((size_t)nb * ms * 4 * 4 + (size_t)nb * KNZ_LZS_COARSE * 4 * 2 + (size_t)nb * 2 * 4 * 2 + 64) ||
            h->lzs_misc.reserve((size_t)nb + 64 + (size_t)nb * 16 + (size_t)nb * 32 + 64) || h->lzs_mask.reserve(nb + 64) ||
            h->lzs_q.reserve(((lanes ? 0 : nseg) + nb) * KNZ_LZS_COARSE * 4 + nseg + 64))
            { (void)hipGetLastError(); return 1; }                     // does not fit: the caller takes the first form (and the sticky allocation error is cleared)
        LzSegArgs g;
        memset(&g, 0, sizeof(g));
        g.pa = pa; g.seg_size = segSize; g.segs = segs; g.tok_cap = tokCap; g.warm = warm; g.map_stride = ms;
        uint32_t* w = h->lzs_state.as<uint32_t>();
        g.entry = w; g.used = w + 5 * nseg; g.exit_ = w + 10 * nseg; g.ntok = w + 15 * nseg;
        uint32_t* segsum = w + 16 * nseg;
        g.need = (uint8_t*)(w + 20 * nseg);
        g.tok = h->lzs_tok.as<uint4>();
        uint32_t* m = h->lzs_maps.as<uint32_t>();
        const size_t mapWords = (size_t)nb * ms;
        g.Jp = m; g.Mp = m + mapWords; g.Jn = m + 2 * mapWords; g.Mn = m + 3 * mapWords;
        g.Cp = m + 4 * mapWords; g.Cn = g.Cp + (size_t)nb * KNZ_LZS_COARSE; g.Sp = g.Cn + (size_t)nb * KNZ_LZS_COARSE; g.Sn = g.Sp + 2 * (size_t)nb;
        g.blk_state = h->lzs_misc.as<uint8_t>();
        g.blk_flags = (uint32_t*)(h->lzs_misc.as<uint8_t>() + (((size_t)nb + 63) & ~(size_t)63));
        uint32_t* blkout = g.blk_flags + 4 * (size_t)nb;
        g.qmap = h->lzs_q.as<uint32_t>(); g.cmap = g.qmap + (lanes ? 0 : nseg) * KNZ_LZS_COARSE; g.qhit = (uint8_t*)(g.cmap + (size_t)nb * KNZ_LZS_COARSE);
        if (lanes) g.qmap = nullptr;                                                      // (no query log: who has to run again is found from the data, knz_lzs_mark_kernel)
        // exactness moves forward one segment per round at least: the same reach in positions whatever the segment size (48 rounds of 4096 positions)
        g.max_rounds = (uint32_t)std::min<uint64_t>(256, (uint64_t)KNZ_LZS_MAX_ROUNDS * std::max<uint32_t>(1, KNZ_LZS_SEG / segSize));
        g.all_again = knz_measure_switch("KNZ_LZS_ALL_AGAIN") != nullptr ? 1u : 0u;       // (measurements: every live segment of a block with holes in every round)
        // the list of map words that moved in a round holds a whole block's map: with 8192 words (rounds 1-2 of a 4 MiB block move more) the third round of
        // S-silesia ran every segment, 5.2 ms; selective it takes 2.9 ms. (KNZ_LZS_CHG_CAP: a short list, for the tests of the "too many" path)
        const char* cc = knz_test_switch("KNZ_LZS_CHG_CAP");
        const uint32_t chgCap = cc ? std::max(1u, (uint32_t)atoi(cc)) : (uint32_t)std::min<uint64_t>(std::max<uint64_t>(ms, 64), 1u << 22);
        if (lanes && !g.all_again) {
            if (h->lzs_chg.reserve((size_t)nb * chgCap * 4 + (size_t)nb * 4 + 64)) { (void)hipGetLastError(); return 1; }
            g.chg = h->lzs_chg.as<uint32_t>(); g.chg_n = g.chg + (size_t)nb * chgCap; g.chg_cap = chgCap;
            g.skeys = h->lz_k1.as<uint32_t>(); g.svals = h->lz_v1.as<uint32_t>(); g.total = total; g.hash_log = hashLog;
        }
        h->lzs_n = nb;
        const bool lzsProf = knz_measure_switch("KNZ_LZS_PROF") != nullptr;
        if (lzsProf) {
            const size_t rpBytes = ((size_t)256 * nb * 12 + 63) & ~(size_t)63;
            if (h->text_prof.reserve(rpBytes + nseg * 32 + 64)) { (void)hipGetLastError(); return 1; }
            g.rprof = (uint32_t*)h->text_prof.p;
            g.sprof = (unsigned long long*)((uint8_t*)h->text_prof.p + rpBytes);
            if (hipMemsetAsync(g.sprof, 0, nseg * 32, st) != hipSuccess) return 2;
        }
        if (hipMemsetAsync(m, 0, (4 * mapWords + (size_t)nb * KNZ_LZS_COARSE * 2 + (size_t)nb * 4) * 4, st) != hipSuccess ||
            hipMemsetAsync(blkout, 0, (size_t)nb * 32, st) != hipSuccess) return 2;
        hipLaunchKernelGGL(knz_lzs_init_kernel, dim3((segs + 255) / 256, nb), dim3(256), 0, st, g);
        std::vector<uint8_t> state(nb);
        uint32_t round = 0;
        for (;; round++) {
            if (hipMemsetAsync(g.Jn, 0, mapWords * 4, st) != hipSuccess || hipMemsetAsync(g.Mn, 0, mapWords * 4, st) != hipSuccess ||
                hipMemsetAsync(g.Cn, 0, (size_t)nb * KNZ_LZS_COARSE * 4, st) != hipSuccess || hipMemsetAsync(g.Sn, 0, (size_t)nb * 8, st) != hipSuccess ||
                hipMemsetAsync(g.cmap, 0, (size_t)nb * KNZ_LZS_COARSE * 4, st) != hipSuccess) return 2;
            if (g.chg && (hipMemsetAsync(g.chg_n, 0, (size_t)nb * 4, st) != hipSuccess || hipMemsetAsync(g.qhit, 0, nseg, st) != hipSuccess)) return 2;
            if (lanes) KNZ_LAUNCH_PROBED(knz_lzs_parse_lanes_kernel, dim3((segs + 63) / 64, nb), dim3(64), 0, st, g);
            else KNZ_LAUNCH_PROBED(knz_lzs_parse_kernel, dim3(segs, nb), dim3(64), 0, st, g);
            if (round > 0 && !g.all_again) hipLaunchKernelGGL(knz_lzs_carry_kernel, dim3(segs, nb), dim3(64), 0, st, g);
            hipLaunchKernelGGL(knz_lzs_compare_kernel, dim3((unsigned)((ms + 1023) / 1024), nb), dim3(256), 0, st, g, (uint32_t)ms);
            if (g.chg) hipLaunchKernelGGL(knz_lzs_mark_kernel, dim3(std::min(256u, (chgCap + 7) / 8), nb), dim3(256), 0, st, g);
            else if (!lanes) hipLaunchKernelGGL(knz_lzs_qhit_kernel, dim3(segs, nb), dim3(64), 0, st, g);
            hipLaunchKernelGGL(knz_lzs_relink_kernel, dim3(nb), dim3(KNZ_LZS_RUNS), 0, st, g, round);
            if (lzsProf && g.chg) {                                              // diagnostics: map words that moved in this round, per block
                std::vector<uint32_t> cn(nb);
                if (hipMemcpyAsync(cn.data(), g.chg_n, 4 * (size_t)nb, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess) {
                    fprintf(stderr, "LZ forward round %u, map words that moved per block:", round + 1);
                    for (uint32_t q = 0; q < nb; q++) fprintf(stderr, " %u", cn[q]);
                    fprintf(stderr, "\n");
                }
            }
            std::swap(g.Jp, g.Jn); std::swap(g.Mp, g.Mn); std::swap(g.Cp, g.Cn); std::swap(g.Sp, g.Sn);
            // the host looks at the blocks' states after every round at first, then after every fourth one (a round over settled blocks is a handful of
            // launches that return at once; a round trip to the host costs more)
            if (round >= 8 && (round & 3) != 3 && round + 1 < g.max_rounds) continue;
            if (hipMemcpyAsync(state.data(), g.blk_state, nb, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return 2;
            bool running = false;
            for (uint32_t b = 0; b < nb; b++) running |= state[b] == 0;
            if (!running || round + 1 >= g.max_rounds) break;
        }
        {   // rounds the fixed point took = the largest number of rounds a block ran (blk_flags[4 b + 2])
            std::vector<uint32_t> fl((size_t)nb * 4);
            if (hipMemcpyAsync(fl.data(), g.blk_flags, fl.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return 2;
            h->lzs_rounds = 1;
            for (uint32_t b = 0; b < nb; b++) h->lzs_rounds = std::max(h->lzs_rounds, fl[4 * (size_t)b + 2]);
        }
        if (lzsProf) {                                                         // diagnostics: where each round's first change sat (segment, map position)
            std::vector<uint32_t> rp((size_t)(round + 1) * nb * 3);
            if (hipMemcpy(rp.data(), g.rprof, rp.size() * 4, hipMemcpyDeviceToHost) == hipSuccess)
                for (uint32_t r = 0; r <= round; r++) {
                    fprintf(stderr, "LZ forward round %u, per block first segment with a new entry state / of / first moved map word as a segment / segments that run next:", r + 1);
                    for (uint32_t q = 0; q < nb; q++) {
                        const uint32_t a0 = rp[((size_t)r * nb + q) * 3], a1 = rp[((size_t)r * nb + q) * 3 + 1], a2 = rp[((size_t)r * nb + q) * 3 + 2];
                        if (a0 == 0 && a1 == 0) continue;
                        fprintf(stderr, " %u/%u/%d/%u", a0 & 0xFFFF, a0 >> 16, a1 == 0xFFFFFFFFu ? -1 : (int)((uint64_t)a1 * 32 / segSize), a2);
                    }
                    fprintf(stderr, "\n");
                }
        }
        if (lzsProf) {                                                         // diagnostics: the segments whose parses took longest
            std::vector<unsigned long long> sp(nseg * 4);
            if (hipMemcpy(sp.data(), g.sprof, sp.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
                std::vector<size_t> order(nseg);
                for (size_t i = 0; i < nseg; i++) order[i] = i;
                std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return sp[4 * x + 3] > sp[4 * y + 3]; });
                unsigned long long sum = 0; for (size_t i = 0; i < nseg; i++) sum += sp[4 * i + 3];
                fprintf(stderr, "LZ forward, last parse of each segment: mean %.1f kticks; slowest (block/segment: kticks last, kticks all rounds, steps, hole-chain steps):", (double)sum / 1000.0 / (double)nseg);
                for (size_t i = 0; i < std::min<size_t>(nseg, 24); i++) { const size_t q = order[i];
                    fprintf(stderr, " %zu/%zu:%llu,%llu,%llu,%llu", q / segs, q % segs, sp[4 * q + 3] / 1000, sp[4 * q] / 1000, sp[4 * q + 1], sp[4 * q + 2]); }
                fprintf(stderr, "\n");
            }
        }
        if (lzsProf) {                                                         // diagnostics: rounds each block took to settle
            std::vector<uint32_t> fl((size_t)nb * 4);
            if (hipMemcpy(fl.data(), g.blk_flags, fl.size() * 4, hipMemcpyDeviceToHost) == hipSuccess) {
                fprintf(stderr, "LZ forward, rounds per block (state):");
                for (uint32_t q = 0; q < nb; q++) fprintf(stderr, " %u(%u)", fl[4 * q + 2], (unsigned)state[q]);
                fprintf(stderr, "\n");
            }
        }
        hipLaunchKernelGGL(knz_lzs_emit_count_kernel, dim3(segs, nb), dim3(256), 0, st, g, segsum);
        hipLaunchKernelGGL(knz_lzs_emit_offsets_kernel, dim3(nb), dim3(64), 0, st, g, segsum, blkout);
        KNZ_LAUNCH_PROBED(knz_lzs_emit_write_kernel, dim3(segs, nb), dim3(256), 0, st, g, (const uint32_t*)segsum, (const uint32_t*)blkout);
        hipLaunchKernelGGL(knz_lzs_emit_tail_kernel, dim3(nb), dim3(256), 0, st, g, (const uint32_t*)blkout);
        hipLaunchKernelGGL(knz_lzs_serial_mask_kernel, dim3((nb + 63) / 64), dim3(64), 0, st, g, h->lzs_mask.as<uint8_t>());
        pa.a.active = h->lzs_mask.as<uint8_t>();                               // the one-wave kernel below takes what is left
    }
    if (knz_measure_switch("KNZ_LZ_PROF") != nullptr) {                                 // diagnostics: cycles per part of the parse to stderr
        if (h->text_prof.reserve((size_t)nb * 64)) { (void)hipGetLastError(); return 1; }
        if (hipMemsetAsync(h->text_prof.p, 0, (size_t)nb * 64, st) != hipSuccess) return 2;
        pa.prof = (unsigned long long*)h->text_prof.p;
    }
    KNZ_LAUNCH_PROBED(knz_lz_forward_par_kernel, dim3(nb), dim3(64), 0, st, pa);
    if (pa.prof) {
        std::vector<unsigned long long> pr((size_t)nb * 8);
        if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(pr.data(), pa.prof, pr.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return 2;
        for (uint32_t q = 0; q < nb; q++) {
            const unsigned long long* r = pr.data() + (size_t)q * 8;
            if (r[4] + r[5]) fprintf(stderr, "LZ block %u: misses %llu matches %llu cycles load %llu miss %llu search %llu emit %llu\n", q, r[4], r[5], r[0], r[1], r[2], r[3]);
        }
    }
    return 0;
}

// LZ / LZX inverse, parallel form (lz_inv_par.hip). On return h->lzi_serial marks the blocks that are left to the one-wave kernel
// (damaged or unusual streams; everything when the batch does not fit 32-bit token indexes).
static int lz_inverse_par(Handle* h, XfBatch& x, const LzArgs& la, hipStream_t st) {
    const uint32_t nb = x.nblocks;
    if (h->lzi_geo.reserve(64 * (size_t)nb) || h->lzi_tokbase.reserve(4 * (size_t)(nb + 1)) || h->lzi_serial.reserve(nb + 64) || h->lzi_flag.reserve(64))
        return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed (LZ inverse)");
    h->lzi_serial_n = nb;
    LziArgs g;
    memset(&g, 0, sizeof(g));
    g.a = la; g.geo = h->lzi_geo.as<uint32_t>(); g.serial = h->lzi_serial.as<uint8_t>(); g.unfinished = h->lzi_flag.as<uint32_t>();
    hipLaunchKernelGGL(knz_lzi_header_kernel, dim3((nb + 63) / 64), dim3(64), 0, st, g);
    std::vector<uint32_t> geo((size_t)nb * 16), tokBase(nb + 1);
    HIP_OK(hipMemcpyAsync(geo.data(), g.geo, 64 * (size_t)nb, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    uint64_t totalTok = 0;
    uint32_t maxTok = 0, npar = 0;
    for (uint32_t b = 0; b < nb; b++) {
        tokBase[b] = (uint32_t)totalTok;
        if (geo[(size_t)b * 16 + LZI_PAR]) { const uint32_t nt = geo[(size_t)b * 16 + LZI_NTOK]; totalTok += (uint64_t)nt + 2; maxTok = std::max(maxTok, nt); npar++; }
        if (totalTok >= 0xFFFFFFF0ull) break;
    }
    const uint64_t mapStride = (x.stride + 3) & ~(uint64_t)3;
    if (npar == 0 || totalTok >= 0xFFFFFFF0ull || knz_test_switch("KNZ_LZ_INV_CHAIN") != nullptr) {        // nothing for this path (KNZ_LZ_INV_CHAIN: tests run the one-wave kernel alone)
        return KNZ_OK;                                                             // (the header kernel has marked every active block for the one-wave kernel)
    }
    tokBase[nb] = (uint32_t)totalTok;
    const uint32_t segs = (maxTok + KNZ_LZI_SEG - 1) / KNZ_LZI_SEG;
    const size_t tt = (size_t)totalTok + 64;
    if (h->lzi_ta.reserve(4 * tt) || h->lzi_tb.reserve(4 * tt) || h->lzi_tc.reserve(4 * tt) || h->lzi_td.reserve(4 * tt) || h->lzi_lxg.reserve(4 * tt) ||
        h->lzi_lxc.reserve(4 * tt) || h->lzi_ml.reserve(4 * tt) || h->lzi_seg.reserve(32 * (size_t)nb * segs + 64) ||
        h->lzi_map.reserve(4 * mapStride * nb + 64))
        return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed (LZ inverse)");
    HIP_OK(hipMemcpyAsync(h->lzi_tokbase.p, tokBase.data(), 4 * (size_t)(nb + 1), hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));                                          // (tokBase is a local)
    g.segs = segs; g.tok_base = h->lzi_tokbase.as<uint32_t>();
    g.t_a = h->lzi_ta.as<uint32_t>(); g.t_b = h->lzi_tb.as<uint32_t>(); g.t_c = h->lzi_tc.as<uint32_t>(); g.t_d = h->lzi_td.as<uint32_t>();
    g.seg = h->lzi_seg.as<uint32_t>(); g.lx_g = h->lzi_lxg.as<uint32_t>(); g.lx_c = h->lzi_lxc.as<uint32_t>();
    g.ml_val = h->lzi_ml.as<uint32_t>(); g.map = h->lzi_map.as<uint32_t>(); g.map_stride = mapStride;
    const dim3 gtok(segs, nb);
    hipLaunchKernelGGL(knz_lzi_a_count_kernel, gtok, dim3(256), 0, st, g);
    hipLaunchKernelGGL(knz_lzi_a_offsets_kernel, dim3(nb), dim3(64), 0, st, g);
    hipLaunchKernelGGL(knz_lzi_a_apply_kernel, gtok, dim3(256), 0, st, g);
    KNZ_LAUNCH_PROBED(knz_lzi_litext_chain_kernel, dim3(nb), dim3(64), 0, st, g);
    KNZ_LAUNCH_PROBED(knz_lzi_mlen_parse_kernel, dim3(nb), dim3(256), 0, st, g);
    hipLaunchKernelGGL(knz_lzi_b_count_kernel, gtok, dim3(256), 0, st, g);
    hipLaunchKernelGGL(knz_lzi_b_offsets_kernel, dim3(nb), dim3(64), 0, st, g);
    KNZ_LAUNCH_PROBED(knz_lzi_b_apply_kernel, gtok, dim3(256), 0, st, g);
    hipLaunchKernelGGL(knz_lzi_finalize_kernel, dim3((nb + 63) / 64), dim3(64), 0, st, g);
    KNZ_LAUNCH_PROBED(knz_lzi_map_kernel, dim3((maxTok + 255) / 256, nb), dim3(256), 0, st, g);
    const dim3 gout((unsigned)((la.out_cap + 1023) / 1024), nb);
    for (int pass = 0; pass < KNZ_LZI_JUMP_PASSES; pass++) KNZ_LAUNCH_PROBED(knz_lzi_jump_kernel, gout, dim3(256), 0, st, g);   // (the gather finishes what the passes leave open)
    KNZ_LAUNCH_PROBED(knz_lzi_gather_kernel, gout, dim3(256), 0, st, g);
    return KNZ_OK;
}

// ---- PACK / DNA (alias.hip) -------------------------------------------------------------------------------------------------
// Bounded groups of blocks like the UTF stage: the forward stage keeps a 65536-bin pair histogram per block (256 KiB), so the workspace is
// sized to a group of at most 64 blocks (16 MiB), not to the batch.
static int alias_stage(Handle* h, XfBatch& x, uint32_t t, bool forward, hipStream_t st) {
    const uint32_t nb = x.nblocks;
    const uint32_t G = std::min<uint32_t>(nb, 64u);
    if (h->alias_state.reserve((size_t)G * KNZ_ALIAS_STATE_WORDS * 4) || (forward && h->alias_f1.reserve(((size_t)G << 16) * 4)))
        return knz_set_error(h, forward ? KNZ_ERR_CREATE_COMPRESSOR : KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed (PACK)");
    for (uint32_t g0 = 0; g0 < nb; g0 += G) {
        const uint32_t gn = std::min<uint32_t>(G, nb - g0);
        const XfBatch g = x.group(g0, gn);
        AliasArgs a = g.args<AliasArgs>();
        a.blk_dt = forward ? g.blk_dt : nullptr;
        a.state = h->alias_state.as<uint32_t>(); a.f1 = h->alias_f1.as<uint32_t>(); a.seg = h->xf_sega.as<uint32_t>() + (size_t)g0 * x.spb * 4;
        a.only_dna = t == KNZ_T_DNA ? 1u : 0u;
        a.h1_chunks = (uint32_t)std::max<uint64_t>(1, ((uint64_t)a.out_cap + KNZ_ALIAS_H1_CHUNK - 1) / KNZ_ALIAS_H1_CHUNK);
        HIP_OK(hipMemsetAsync(h->alias_state.p, 0, (size_t)gn * KNZ_ALIAS_STATE_WORDS * 4, st));
        const dim3 gseg(x.spb, gn);
        if (forward) {
            HIP_OK(hipMemsetAsync(h->alias_f1.p, 0, ((size_t)gn << 16) * 4, st));
            KNZ_LAUNCH_PROBED(knz_alias_hist0_kernel, gseg, dim3(256), 0, st, a);
            hipLaunchKernelGGL(knz_alias_plan_kernel, dim3(gn), dim3(256), 0, st, a);
            KNZ_LAUNCH_PROBED(knz_alias_hist1_kernel, dim3(KNZ_ALIAS_SLICES * a.h1_chunks, gn), dim3(KNZ_ALIAS_H1_THREADS), 0, st, a);
            KNZ_LAUNCH_PROBED(knz_alias_select_kernel, dim3(gn), dim3(1024), 0, st, a);
            KNZ_LAUNCH_PROBED(knz_alias_pack_kernel, gseg, dim3(256), 0, st, a);
            KNZ_LAUNCH_PROBED(knz_alias_parse_kernel<false>, gseg, dim3(256), 0, st, a);
            hipLaunchKernelGGL(knz_alias_offsets_kernel, dim3(gn), dim3(64), 0, st, a);
            KNZ_LAUNCH_PROBED(knz_alias_parse_kernel<true>, gseg, dim3(256), 0, st, a);
        } else {
            hipLaunchKernelGGL(knz_alias_inv_header_kernel, dim3(gn), dim3(64), 0, st, a);
            KNZ_LAUNCH_PROBED(knz_alias_inv_seg_kernel<false>, gseg, dim3(256), 0, st, a);
            hipLaunchKernelGGL(knz_alias_inv_offsets_kernel, dim3(gn), dim3(64), 0, st, a);
            KNZ_LAUNCH_PROBED(knz_alias_inv_seg_kernel<true>, gseg, dim3(256), 0, st, a);
        }
    }
    return KNZ_OK;
}

// ---- the stages whose kernels need no host code of their own: RANK / MTFT, ZRLT, LZ / LZX, SRT, LZP, UTF ------------------------
static int sbrt_stage(Handle* h, XfBatch& x, uint32_t t, bool forward, hipStream_t st) {
    const uint32_t nb = x.nblocks, gseg = nb * x.spb;
    XfArgs a = xf_args(h, x, t == KNZ_T_RANK ? 2 : 1);
    if (forward) {
        hipLaunchKernelGGL(knz_sbrt_seg_last2_kernel, dim3(gseg), dim3(64), 0, st, a);
        hipLaunchKernelGGL(knz_sbrt_carry_kernel, dim3(nb), dim3(256), 0, st, a);
        if (t == KNZ_T_RANK) KNZ_LAUNCH_PROBED(knz_sbrt_apply_kernel<2>, dim3(gseg), dim3(64), 0, st, a);
        else hipLaunchKernelGGL(knz_sbrt_apply_kernel<1>, dim3(gseg), dim3(64), 0, st, a);
    } else {
        if (t == KNZ_T_RANK) {
            const char* v = knz_test_switch("KNZ_RANK_VARIANT");                                         // (tests: 0 = the round-1 kernel as a cross-check; -DKNZ_MEASURE builds: the earlier forms)
            const int vi = v ? atoi(v) : 5;
            if (knz_test_switch("KNZ_RANK_UNPACKED") != nullptr) a.mode |= 0x100;                   // (tests: the form for blocks > 8 MiB on small inputs)
            if (const char* cv = knz_test_switch("KNZ_RANK_CUT")) a.mode |= ((uint32_t)atoi(cv) / 64u) << 12;   // (tests: where the packed form hands over to the three-register form, ranks)
            if (vi == 0) KNZ_LAUNCH_PROBED(knz_sbrt_inverse_kernel<2>, dim3(nb), dim3(64), 0, st, a);   // the round-1 form (tests: cross-check of the chain kernel)
#ifdef KNZ_MEASURE                                                                             // earlier and measurement forms of the step (docs/HISTORY.md "Tried and dropped")
            else if (vi == 3) KNZ_LAUNCH_PROBED((knz_rank_inverse_chain_kernel<2, 2>), dim3(nb), dim3(64), 0, st, a);   // round-2 first form (SALU arithmetic)
            else if (vi == 4) KNZ_LAUNCH_PROBED((knz_rank_inverse_chain_kernel<2, 4>), dim3(nb), dim3(64), 0, st, a);   // round-2 second form: lane-1 copies of (q, e) kept in registers
            else if (vi == 6) KNZ_LAUNCH_PROBED((knz_rank_inverse_chain_kernel<2, 12 | 64>), dim3(nb), dim3(64), 0, st, a);   // (measured, slower) words with ranks >= 64 as straight-line bodies over 2 / 4 registers
            else if (vi == 7) KNZ_LAUNCH_PROBED((knz_rank_inverse_chain_kernel<2, 4 | 16>), dim3(nb), dim3(64), 0, st, a);   // (measurement: 4 instructions beside the chain in every low step)
            else if (vi == 8) KNZ_LAUNCH_PROBED((knz_rank_inverse_chain_kernel<2, 4 | 32>), dim3(nb), dim3(64), 0, st, a);   // (measurement: 4 instructions on the chain in every low step)
#endif
            else KNZ_LAUNCH_PROBED((knz_rank_inverse_chain_kernel<2, 4 | 64>), dim3(nb), dim3(64), 0, st, a);           // default: the lane-1 copies are DPP operands of the step's own instructions
#if !defined(KNZ_HIP_EMU)
            if (vi != 0 && vi != 3 && knz_measure_switch("KNZ_RANK_PROF") != nullptr) {                  // diagnostics: time of every block's chain
                std::vector<unsigned long long> tk(std::min<size_t>(nb, 1024));
                if (hipStreamSynchronize(st) == hipSuccess && hipMemcpyFromSymbol(tk.data(), HIP_SYMBOL(g_knz_rank_ticks), tk.size() * 8) == hipSuccess) {
                    fprintf(stderr, "inverse RANK chain, ms per block:");
                    for (size_t q = 0; q < tk.size(); q++) fprintf(stderr, " %.0f", (double)tk[q] / 1e5);
                    fprintf(stderr, "\n");
                }
            }
#endif
        }
        else if (knz_test_switch("KNZ_MTFT_CHAIN") != nullptr) KNZ_LAUNCH_PROBED(knz_sbrt_inverse_kernel<1>, dim3(nb), dim3(64), 0, st, a);   // (tests: the one-wave form)
        else {   // move-to-front permutes positions independently of the content: per-segment permutations, composed per block
            hipLaunchKernelGGL(knz_mtft_inv_perm_kernel, dim3(gseg), dim3(64), 0, st, a);
            hipLaunchKernelGGL(knz_mtft_inv_compose_kernel, dim3(nb), dim3(256), 0, st, a);
            hipLaunchKernelGGL(knz_mtft_inv_apply_kernel, dim3(gseg), dim3(64), 0, st, a);
        }
    }
    return KNZ_OK;
}

static int zrlt_stage(Handle* h, XfBatch& x, uint32_t, bool forward, hipStream_t st) {
    const uint32_t nb = x.nblocks, gseg = nb * x.spb;
    XfArgs a = xf_args(h, x, 0);
    if (forward) {
        hipLaunchKernelGGL(knz_zrlt_seg_lastnz_kernel, dim3(gseg), dim3(256), 0, st, a);
        hipLaunchKernelGGL(knz_zrlt_carry_kernel, dim3(nb), dim3(64), 0, st, a);
        hipLaunchKernelGGL(knz_zrlt_seg_kernel<false>, dim3(gseg), dim3(256), 0, st, a);
        hipLaunchKernelGGL(knz_zrlt_offsets_kernel, dim3(nb), dim3(64), 0, st, a);
        hipLaunchKernelGGL(knz_zrlt_seg_kernel<true>, dim3(gseg), dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL(knz_zrlti_seg_lastnd_kernel, dim3(gseg), dim3(256), 0, st, a);
        hipLaunchKernelGGL(knz_zrlt_carry_kernel, dim3(nb), dim3(64), 0, st, a);
        hipLaunchKernelGGL(knz_zrlti_seg_kernel<false>, dim3(gseg), dim3(256), 0, st, a);
        hipLaunchKernelGGL(knz_zrlti_offsets_kernel, dim3(nb), dim3(64), 0, st, a);
        hipLaunchKernelGGL(knz_zrlti_zero_kernel, dim3(64, nb), dim3(256), 0, st, a);
        hipLaunchKernelGGL(knz_zrlti_seg_kernel<true>, dim3(gseg), dim3(256), 0, st, a);
    }
    return KNZ_OK;
}

static int lz_stage(Handle* h, XfBatch& x, uint32_t t, bool forward, hipStream_t st) {
    const uint32_t nb = x.nblocks;
    const unsigned hashLog = t == KNZ_T_LZX ? 19 : 16;
    const uint64_t bstride = ((x.stride + 1024 + 63) & ~(uint64_t)63);
    if (forward && (h->lz_hash.reserve(((size_t)nb << hashLog) * 4) || h->lz_tk.reserve(bstride * nb) || h->lz_mb.reserve(bstride * nb) || h->lz_ml.reserve(bstride * nb)))
        return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed (LZ)");
    LzArgs a = x.args<LzArgs>();
    a.hashes = h->lz_hash.as<int32_t>(); a.tk = h->lz_tk.as<uint8_t>(); a.mb = h->lz_mb.as<uint8_t>(); a.ml = h->lz_ml.as<uint8_t>(); a.buf_stride = bstride; a.extra = t == KNZ_T_LZX ? 1 : 0; a.blk_dt = forward ? x.blk_dt : nullptr;
    if (forward && knz_test_switch("KNZ_LZ_CHAIN") == nullptr) {
        const int rc = lz_forward_par(h, x, a, hashLog, st);
        if (rc == 0) return KNZ_OK;
        if (rc != 1) return knz_set_error(h, KNZ_ERR_UNKNOWN, "LZ forward: HIP error in the table-free forms");   // (1 = does not fit: first form below)
    }
    if (forward) {                                                               // first form: the parse keeps its own hash table (KNZ_LZ_CHAIN, or a batch beyond one sort)
        HIP_OK(hipMemsetAsync(h->lz_hash.p, 0, ((size_t)nb << hashLog) * 4, st));        // hash tables start empty (:265-271)
        KNZ_LAUNCH_PROBED(knz_lz_forward_kernel, dim3(nb), dim3(64), 0, st, a);
    } else {
        // parallel form first; the one-wave kernel takes the blocks it leaves (damaged or unusual streams)
        const int rc = lz_inverse_par(h, x, a, st);
        if (rc) return rc;
        a.active = h->lzi_serial.as<uint8_t>();
        KNZ_LAUNCH_PROBED(knz_lz_inverse_kernel, dim3(nb), dim3(64), 0, st, a);
    }
    return KNZ_OK;
}

static int srt_stage(Handle* h, XfBatch& x, uint32_t, bool forward, hipStream_t st) {
    const uint32_t nb = x.nblocks, gseg = nb * x.spb;
    XfArgs a = xf_args(h, x, 0);
    if (!forward) { KNZ_LAUNCH_PROBED(knz_srt_inverse_kernel, dim3(nb), dim3(64), 0, st, a); return KNZ_OK; }
    if (knz_test_switch("KNZ_SRT_CHAIN") != nullptr) { hipLaunchKernelGGL(knz_srt_forward_kernel, dim3(nb), dim3(64), 0, st, a); return KNZ_OK; }   // (tests: the one-wave form)
    // forward = MTFT ranks (segment-parallel) + first occurrences + a stable partition by symbol (srt_lzp.hip)
    const uint64_t tstride = (x.stride + 63) & ~(uint64_t)63;
    if (h->srt_tab.reserve((size_t)nb * KNZ_SRT_TAB * 4 + 64) || h->srt_tmp.reserve((size_t)nb * tstride + 64) || h->srt_ptrs.reserve((size_t)nb * 24 + 64))
        return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed (SRT)");
    uint64_t* ptrs = h->srt_ptrs.as<uint64_t>();
    uint32_t* dummyLen = (uint32_t*)(ptrs + nb);
    int32_t* dummyOk = (int32_t*)(ptrs + 2 * (size_t)nb);
    hipLaunchKernelGGL(knz_fill_ptrs_kernel, dim3((nb + 63) / 64), dim3(64), 0, st, nb, (uint64_t)h->srt_tmp.p, tstride, ptrs);
    SrtParArgs pa = x.args<SrtParArgs>();
    pa.tab = h->srt_tab.as<uint32_t>(); pa.rank_ptr = ptrs; pa.seg_cnt = h->xf_sega.as<int32_t>();
    hipLaunchKernelGGL(knz_srt_stats_kernel, dim3(nb), dim3(256), 0, st, pa);
    XfArgs m = xf_args(h, x, 1);                                  // MTFT ranks of every position into the scratch blocks
    m.out_ptr = ptrs; m.out_cap = 0xFFFFFFFFu; m.out_len = dummyLen; m.ok = dummyOk;
    hipLaunchKernelGGL(knz_sbrt_seg_last2_kernel, dim3(gseg), dim3(64), 0, st, m);
    hipLaunchKernelGGL(knz_sbrt_carry_kernel, dim3(nb), dim3(256), 0, st, m);
    hipLaunchKernelGGL(knz_sbrt_apply_kernel<1>, dim3(gseg), dim3(64), 0, st, m);
    hipLaunchKernelGGL(knz_srt_seg_count_kernel, dim3(gseg), dim3(64), 0, st, pa);
    hipLaunchKernelGGL(knz_srt_seg_scan_kernel, dim3(nb), dim3(256), 0, st, pa);
    hipLaunchKernelGGL(knz_srt_scatter_kernel, dim3(gseg), dim3(64), 0, st, pa);
    return KNZ_OK;
}

static int lzp_stage(Handle* h, XfBatch& x, uint32_t, bool forward, hipStream_t st) {
    const uint32_t nb = x.nblocks;
    if (h->lz_hash.reserve(((size_t)nb << 16) * 4)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed (LZP)");
    LzArgs a = x.args<LzArgs>();
    a.hashes = h->lz_hash.as<int32_t>(); a.tk = nullptr; a.mb = nullptr; a.ml = nullptr; a.buf_stride = 0; a.extra = 0; a.blk_dt = nullptr;
    HIP_OK(hipMemsetAsync(h->lz_hash.p, 0, ((size_t)nb << 16) * 4, st));                   // both directions start from an empty table (:1001-1005, :1100-1104)
    if (forward) KNZ_LAUNCH_PROBED(knz_lzp_forward_kernel, dim3(nb), dim3(64), 0, st, a);
    else KNZ_LAUNCH_PROBED(knz_lzp_inverse_kernel, dim3(nb), dim3(64), 0, st, a);
    return KNZ_OK;
}

static int utf_stage(Handle* h, XfBatch& x, uint32_t, bool forward, hipStream_t st) {
    const uint32_t nb = x.nblocks;
    // bounded groups of blocks (like the suffix sort): the forward stage keeps a 2^22-entry alias map per block (16 MiB), so the
    // workspace is sized to a group of at most 64 blocks (1 GiB), not to the batch: a stream of 15 000 64-KiB blocks still fits
    const uint32_t G = std::min<uint32_t>(nb, 64u);
    const uint64_t bitsStride = ((x.stride >> 3) + 64) & ~(uint64_t)15;
    if (forward ? (h->utf_map.reserve(((size_t)G << 22) * 4) || h->utf_syms.reserve((size_t)G * 32768 * 4) || h->utf_ranks.reserve((size_t)G * 32768 * 4) ||
                   h->utf_bits.reserve((size_t)G * bitsStride + 64))
                : h->utf_inv.reserve((size_t)G * 32768 * 8))
        return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed (UTF)");
    for (uint32_t g0 = 0; g0 < nb; g0 += G) {
        const uint32_t gn = std::min<uint32_t>(G, nb - g0);
        const XfBatch g = x.group(g0, gn);
        UtfArgs a = g.args<UtfArgs>();
        a.alias_map = h->utf_map.as<int32_t>(); a.symlist = h->utf_syms.as<uint32_t>(); a.ranks = h->utf_ranks.as<uint32_t>();
        a.inv_map = h->utf_inv.as<uint64_t>(); a.chain_bits = h->utf_bits.as<uint8_t>(); a.bits_stride = bitsStride; a.blk_dt = g.blk_dt;
        if (forward) {
            HIP_OK(hipMemsetAsync(h->utf_map.p, 0, ((size_t)gn << 22) * 4, st));
            KNZ_LAUNCH_PROBED(knz_utf_forward_kernel, dim3(gn), dim3(KNZ_UTF_FWD_THREADS), 0, st, a);
        } else KNZ_LAUNCH_PROBED(knz_utf_inverse_kernel, dim3(gn), dim3(64), 0, st, a);
    }
    return KNZ_OK;
}

// ---- the transforms of this build: THE list of ids. knz_supports, knz_max_encoded_len, the ctx["dataType"] decision of encode_batch and run_stage read it ----
struct XfCodec {
    uint32_t id; const char* name;
    uint32_t grow, grow_div;        // MaxEncodedLen(n) = n + grow, or n + n / grow_div where grow_div != 0 and n > 1024 (Sequence.go:189-205 over each transform's own rule)
    bool data_type;                 // the stage reads or writes ctx["dataType"]
    int (*stage)(Handle*, XfBatch&, uint32_t id, bool forward, hipStream_t);   // null: NullTransform, nothing to run
};
static const XfCodec kXfCodecs[] = {
    {KNZ_T_NONE, "NONE", 0, 0, false, nullptr},
    {KNZ_T_BWT, "BWT", 33, 0, false, bwt_stage},
    {KNZ_T_LZ, "LZ", 16, 64, false, lz_stage},
    {KNZ_T_ZRLT, "ZRLT", 0, 0, false, zrlt_stage},
    {KNZ_T_MTFT, "MTFT", 33, 0, false, sbrt_stage},
    {KNZ_T_RANK, "RANK", 33, 0, false, sbrt_stage},
    {KNZ_T_TEXT, "TEXT", 0, 0, true, text_stage},
    {KNZ_T_SRT, "SRT", 4 * 256, 0, false, srt_stage},
    {KNZ_T_LZP, "LZP", 16, 64, false, lzp_stage},
    {KNZ_T_LZX, "LZX", 16, 64, false, lz_stage},
    {KNZ_T_UTF, "UTF", 8192, 0, true, utf_stage},
    {KNZ_T_PACK, "PACK", 1024, 0, true, alias_stage},      // AliasCodec.go:439
    {KNZ_T_DNA, "DNA", 1024, 0, true, alias_stage},
};
static const XfCodec* xf_codec(uint32_t id) {
    for (const XfCodec& c : kXfCodecs) if (c.id == id) return &c;
    return nullptr;
}

static int run_stage(Handle* h, XfBatch& x, uint32_t t, bool forward, hipStream_t st) {
    const XfCodec* c = xf_codec(t);
    if (!c) return knz_set_error(h, KNZ_ERR_INVALID_CODEC, "transform has no device implementation in this build");
    return c->stage ? c->stage(h, x, t, forward, st) : KNZ_OK;
}

// bytes that enter a stage, summed over the live blocks (diagnostics: bench.py prices every kernel on the bytes its stage really saw)
__global__ __launch_bounds__(256) void knz_xf_sum_len_kernel(uint32_t nblocks, const uint32_t* len, const uint8_t* active, unsigned long long* out) {
    __shared__ unsigned long long s_part[256];
    unsigned long long acc = 0;
    for (uint32_t b = threadIdx.x; b < nblocks; b += 256) if (active[b]) acc += len[b];
    s_part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) { unsigned long long t = 0; for (int i = 0; i < 256; i++) t += s_part[i]; *out = t; }
}

// Forward sequence. On entry x.cur_ptr/cur_len describe the source blocks, skip[] = 0xFF for active blocks.
static int forward_sequence(Handle* h, XfBatch& x, uint64_t transformType, hipStream_t st) {
    uint32_t toks[8];
    const int nt = seq_tokens(transformType, toks);
    if (h->stage_sum.reserve(8 * 8)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
    HIP_OK(hipMemsetAsync(h->stage_sum.p, 0, 64, st));
    for (int i = 0; i < nt; i++) {
        CommitArgs c = xf_commit_args(h, x, (uint32_t)i);
        const unsigned gb = (x.nblocks + 63) / 64;
        hipLaunchKernelGGL(knz_xf_sum_len_kernel, dim3(1), dim3(256), 0, st, x.nblocks, (const uint32_t*)x.cur_len, (const uint8_t*)x.active, h->stage_sum.as<unsigned long long>() + i);
        if (toks[i] == KNZ_T_NONE) {   // NullTransform: a copy that always applies; bytes stay where they are
            hipLaunchKernelGGL(knz_xf_none_kernel, dim3(gb), dim3(64), 0, st, x.nblocks, x.active, x.skip, (uint32_t)i);
            continue;
        }
        hipLaunchKernelGGL(knz_xf_prepare_kernel, dim3(gb), dim3(64), 0, st, c, x.out_ptr, x.ok);
        int rc = run_stage(h, x, toks[i], true, st);
        if (rc) return rc;
        hipLaunchKernelGGL(knz_xf_commit_kernel, dim3(gb), dim3(64), 0, st, c);
    }
    HIP_OK(hipMemcpyAsync((uint8_t*)h->pinned + 3072, h->stage_sum.p, 64, hipMemcpyDeviceToHost, st));   // (read behind the batch's synchronisation)
    return KNZ_OK;
}

// Inverse sequence (Sequence.go:131-186): stages in reverse order, skipped ones omitted, any failure is fatal for the block
static int inverse_sequence(Handle* h, XfBatch& x, uint64_t transformType, hipStream_t st) {
    uint32_t toks[8];
    const int nt = seq_tokens(transformType, toks);
    const unsigned gb = (x.nblocks + 63) / 64;
    for (int i = nt - 1; i >= 0; i--) {
        if (toks[i] == KNZ_T_NONE) continue;
        CommitArgs c = xf_commit_args(h, x, (uint32_t)i);
        // active = block is live and its skip bit for this stage is clear
        hipLaunchKernelGGL(knz_xf_inv_select_kernel, dim3(gb), dim3(64), 0, st, x.nblocks, x.skip, x.take, x.active, (uint32_t)i, x.blk_status,
                           (i == x.piped_zrlt || i == x.piped_rank) ? x.piped : (const uint8_t*)nullptr);
        hipLaunchKernelGGL(knz_xf_prepare_kernel, dim3(gb), dim3(64), 0, st, c, x.out_ptr, x.ok);
        int rc = run_stage(h, x, toks[i], false, st);
        if (rc) return rc;
        hipLaunchKernelGGL(knz_xf_commit_kernel, dim3(gb), dim3(64), 0, st, c);
    }
    return KNZ_OK;
}
