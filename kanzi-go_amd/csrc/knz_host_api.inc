// Remaining C-ABI entry points (included by knz_gpu.hip): decode batches, host-pointer batch calls,
// multi-GPU segment assembly, single-codec objects.

// ---- decode batch ---------------------------------------------------------------------------------------------------
struct DecodeBatch {
    const uint8_t* d_stream; uint64_t nbytes;     // device buffer holding either a whole .knz stream or staged payloads
    int framed;                                   // 1: walk the stream from first_bit ; 0: blk_bit/blk_bits already on device
    uint64_t first_bit;
    uint64_t seg_bits;                            // framed == 1: != 0 => segment without end marker
    uint32_t nblocks;                             // framed == 0: given ; framed == 1: result
    uint8_t* d_out; uint64_t out_cap;
    uint64_t out_stride;                          // byte distance between block outputs
    int payload_only; uint32_t given_len;
    uint32_t entropy, checksum_bits, block_size; uint64_t transform;
    std::vector<uint32_t> pre_len;                // results
    std::vector<uint64_t> end_bit;
    std::vector<int32_t> status;
    uint64_t total_out;
};

// The fused ZRLT / RANK chain (rank_pipe.hip) keeps two waves per block resident, polling another kernel's progress words. Their number is bounded
// per DEVICE, over all handles of the process: beyond KNZ_PIPE_DEVICE_BLOCKS blocks in flight a batch takes the regular stage kernels, so that the
// spinning waves can never hold the wave slots the decoders they wait for need (8 handles x EnableGPUDepth(1024) would otherwise ask for 16 K of them).
#define KNZ_PIPE_DEVICE_BLOCKS 1024
#include <atomic>
static std::atomic<int> g_pipe_blocks[64];
// what a decode batch that entered the fused path owes on EVERY way out: nothing of this handle may still run on the side streams when the
// workspace is reused or freed, and its share of the device budget goes back
struct PipeScope {
    Handle* h;
    int blocks = 0;
    bool launched = false;
    explicit PipeScope(Handle* hh) : h(hh) {}
    bool take(int n) {
        const int dev = h->device & 63;
        if (g_pipe_blocks[dev].fetch_add(n) + n > KNZ_PIPE_DEVICE_BLOCKS) { g_pipe_blocks[dev].fetch_sub(n); return false; }
        blocks = n;
        return true;
    }
    ~PipeScope() {
        if (launched) { hipStreamSynchronize(h->stream2); hipStreamSynchronize(h->stream3); }
        if (blocks) g_pipe_blocks[h->device & 63].fetch_sub(blocks);
    }
};

static int decode_batch(Handle* h, DecodeBatch& db, hipStream_t st) {
    h->nprobes = 0;
    if (!knz_supports(db.transform, db.entropy))
        return knz_set_error(h, KNZ_ERR_INVALID_CODEC, "transform/entropy combination has no device implementation in this build");
    uint32_t maxBlocks = db.nblocks;
    if (db.framed) {
        // every block costs at least 8 framing bits + 16 payload bits
        uint64_t bound = db.nbytes / 3 + 1;
        maxBlocks = (uint32_t)std::min<uint64_t>(bound, 1u << 24);
    }
    DevBuf& blkBit = h->blk_dst_bit;      // reuse of the encode-side tables: [maxBlocks] u64 each
    DevBuf& blkBits = h->blk_written;
    if (blkBit.reserve(8 * ((size_t)maxBlocks + 1)) || blkBits.reserve(8 * ((size_t)maxBlocks + 1)) || h->total_bits.reserve(64))
        return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
    uint32_t nblocks = db.nblocks;
    if (db.framed) {
        WalkStreamArgs ws;
        ws.stream = db.d_stream; ws.nbytes = db.nbytes; ws.first_bit = db.first_bit; ws.seg_bits = db.seg_bits; ws.max_blocks = maxBlocks;
        ws.blk_bit = blkBit.as<uint64_t>(); ws.blk_bits = blkBits.as<uint64_t>(); ws.result = h->total_bits.as<uint32_t>();
        hipLaunchKernelGGL(knz_dec_walk_stream_kernel, dim3(1), dim3(1), 0, st, ws);
        uint32_t* res = (uint32_t*)h->pinned;
        HIP_OK(hipMemcpyAsync(res, h->total_bits.p, 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (res[1]) return knz_set_error(h, (int)res[1], "invalid block framing in stream");
        nblocks = res[0];
    }
    db.nblocks = nblocks;
    db.total_out = 0;
    db.pre_len.assign(nblocks, 0); db.end_bit.assign(nblocks, 0); db.status.assign(nblocks, 0);
    if (nblocks == 0) return KNZ_OK;
    const uint32_t maxPre = db.payload_only ? db.given_len : knz_max_encoded_len(db.transform, db.block_size);
    const uint32_t dchunk = entropy_codec(db.entropy)->chunk;
    const uint32_t cpb = std::max<uint32_t>(1, (maxPre + dchunk - 1) / dchunk);
    const size_t nslots = (size_t)nblocks * cpb;
    if (h->blk_len.reserve(4 * (size_t)nblocks) || h->blk_skip.reserve(2 * (size_t)nblocks + 16) || h->blk_cksum.reserve(8 * (size_t)nblocks) ||
        h->chunk_rel.reserve(8 * nslots) || h->blk_status.reserve(4 * (size_t)nblocks) || h->blk_off.reserve(8 * (size_t)nblocks) ||
        h->dec_tables.reserve(8 * (size_t)nblocks))
        return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
    hipEventRecord(h->ev[0], st);
    WalkBlocksArgs wb;
    wb.stream = db.d_stream; wb.nbytes = db.nbytes; wb.blk_bit = blkBit.as<uint64_t>(); wb.blk_bits = blkBits.as<uint64_t>();
    wb.nblocks = nblocks;
    // blockLength handed to decodingTask is padded (v2/io/CompressedStream.go:1620-1626)
    wb.block_size = db.block_size + std::max<uint32_t>(512, db.block_size >> 4);
    wb.checksum_bits = db.checksum_bits; wb.entropy = db.entropy; wb.chunks_per_block = cpb;
    wb.payload_only = db.payload_only; wb.given_len = db.given_len;
    wb.blk_pre_len = h->blk_len.as<uint32_t>(); wb.blk_mode = h->blk_skip.as<uint8_t>(); wb.blk_skip = h->blk_skip.as<uint8_t>() + nblocks;
    wb.blk_cksum = h->blk_cksum.as<uint64_t>(); wb.chunk_bit = h->chunk_rel.as<uint64_t>(); wb.blk_status = h->blk_status.as<int32_t>();
    wb.blk_end_bit = h->dec_tables.as<uint64_t>();
    // Huffman: only the block headers now, the chunk walk shares a launch with the chunk decoders (below)
    const bool fusedWalk = (db.entropy == KNZ_E_HUFFMAN || db.entropy == KNZ_E_ANS0) && knz_test_switch("KNZ_HUF_SPLIT_WALK") == nullptr;   // (the variable lets the tests reach the two-launch path)
    // no transform stage behind the decode: the header pass also places the blocks and makes the host's checks, so nothing is
    // copied or synchronised between it and the walk+decode launch (a refused block shows up in its status at the end)
    const bool direct = fusedWalk && !(db.transform != 0 && !db.payload_only);
    wb.check_out = direct ? 1 : 0; wb.out_off = h->blk_off.as<uint64_t>(); wb.out_base = (uint64_t)db.d_out; wb.out_stride = db.out_stride;
    wb.out_cap = db.out_cap; wb.stream_block_size = db.block_size;
    wb.ans1_ctx_bit = nullptr;
    if (db.entropy == KNZ_E_ANS1) {                                           // the walk leaves every context header's position for the table kernel
        if (h->a1_ctxpos.reserve((size_t)nslots * 257 * 8 + 64)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
        wb.ans1_ctx_bit = h->a1_ctxpos.as<uint64_t>();
    }
    if (fusedWalk) hipLaunchKernelGGL(knz_dec_block_headers_kernel, dim3(nblocks), dim3(64), 0, st, wb);
    else hipLaunchKernelGGL(knz_dec_walk_blocks_kernel, dim3(nblocks), dim3(128), 0, st, wb);
    hipEventRecord(h->ev[1], st);
    const bool xf = db.transform != 0 && !db.payload_only;
    XfBatch xb;
    bool pipeOn = false, pipeGroups = false;
    PipeScope pipeScope(h);
    RankPipeArgs pipeArgs{};
    h->pipe_n = 0;
    uint64_t xstride = 0;
    if (!direct) {   // output placement: transform NONE decodes straight to block b at b*out_stride; otherwise into region 1 of the
        // transform pipeline, the inverse sequence follows
        if (xf) {
            const uint64_t padded = (uint64_t)db.block_size + std::max<uint32_t>(512, db.block_size >> 4);   // decodingTask buffers (:1649-1653)
            xstride = (std::max<uint64_t>(knz_max_encoded_len(db.transform, db.block_size), padded) + 64 + 15) & ~(uint64_t)15;
            if (xf_alloc(h, xb, nblocks, xstride)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
            xb.ctx_entropy = db.entropy; xb.ctx_block_size = db.block_size;      // what the stream's header says, whatever the handle was opened with
        }
        std::vector<uint64_t> off(nblocks);
        for (uint32_t b = 0; b < nblocks; b++) off[b] = xf ? (uint64_t)h->xf_r1.p + (uint64_t)b * xstride : (uint64_t)db.d_out + (uint64_t)b * db.out_stride;
        HIP_OK(hipMemcpyAsync(h->blk_off.p, off.data(), 8 * (size_t)nblocks, hipMemcpyHostToDevice, st));
        // pre-transform lengths decide whether the output fits: check before writing anything
        HIP_OK(hipMemcpyAsync(db.pre_len.data(), h->blk_len.p, 4 * (size_t)nblocks, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(db.status.data(), h->blk_status.p, 4 * (size_t)nblocks, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
    }
    for (uint32_t b = 0; b < nblocks && !direct; b++) {
        if (db.status[b]) return knz_set_error(h, db.status[b], "invalid block in stream");
        if (xf) { if (db.pre_len[b] > xstride) return knz_set_error(h, KNZ_ERR_BLOCK_SIZE, "block larger than the decoder buffers"); continue; }
        if (db.pre_len[b] > db.block_size || (db.pre_len[b] > db.out_stride && b + 1 < nblocks))   // Reader.processBlock :1707-1710
                return knz_set_error(h, KNZ_ERR_PROCESS_BLOCK, "block decodes to more than the stream block size");
        if ((uint64_t)b * db.out_stride + db.pre_len[b] > db.out_cap) return knz_set_error(h, KNZ_ERR_WRITE_FILE, "destination buffer too small");
    }
    if (db.entropy == KNZ_E_FPAQ) {
        FpaqDecArgs da;
        da.stream = db.d_stream; da.nbytes = db.nbytes; da.blk_pre_len = h->blk_len.as<uint32_t>(); da.blk_mode = h->blk_skip.as<uint8_t>();
        da.chunk_bit = h->chunk_rel.as<uint64_t>(); da.blk_out_off = h->blk_off.as<uint64_t>(); da.chunks_per_block = cpb;
        da.blk_status = h->blk_status.as<int32_t>();
        KNZ_LAUNCH_PROBED(knz_fpaq_decode_kernel, dim3(nblocks), dim3(64), 0, st, da);
    } else if (db.entropy == KNZ_E_ANS1) {
        const uint32_t ns = nblocks * cpb;
        const bool wantTable = ns > KNZ_ANS1_LDS_MAX_CHUNKS || knz_test_switch("KNZ_ANS1_TABLE_DECODER") != nullptr;
        if ((wantTable && h->a1_dtab.reserve((size_t)ns * 256 * KNZ_ANS1_SCALE * 4)) || h->a1_info.reserve((size_t)ns * 32) || h->a1_paybit.reserve((size_t)ns * 8) ||
            h->a1_f16.reserve((size_t)ns * 65536 * 2))
            return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
        Ans1DecArgs da;
        da.stream = db.d_stream; da.nbytes = db.nbytes; da.blk_pre_len = h->blk_len.as<uint32_t>(); da.blk_mode = h->blk_skip.as<uint8_t>();
        da.chunk_bit = h->chunk_rel.as<uint64_t>(); da.blk_out_off = h->blk_off.as<uint64_t>(); da.chunks_per_block = cpb; da.nslots = ns;
        da.dtab = h->a1_dtab.as<uint32_t>(); da.info = h->a1_info.as<uint32_t>(); da.paybit = h->a1_paybit.as<uint64_t>();
        da.blk_status = h->blk_status.as<int32_t>();
        da.plain_loop = knz_test_switch("KNZ_ANS1_PLAIN") != nullptr ? 1u : (knz_test_switch("KNZ_ANS1_LOHI_LDS") != nullptr ? 2u : 0u);
        // The LDS decoder (cumulated frequencies of a chunk's 256 contexts in 129 KiB of LDS: one chunk per CU at a time, ~100-165 ms per 4 MiB chunk)
        // takes a batch of any size in ONE launch: the hardware hands a CU the next chunk as soon as one ends. The HBM-table decoder (2 MiB of slot
        // tables per chunk, 16 chunks per wave) is flat at ~830-880 ms up to thousands of chunks: measured crossover (profiles/r04_saturation_*.json,
        // r04_kernel_stats_bwt_copies8.md: 609 chunks, table decoder 824 ms against 2-3 rounds of the LDS decoder) at about five rounds of 256 chunks.
        // (Round 3 switched at 512 chunks: a batch of 203 blocks of 8 MiB decoded slower than one of 102.)
        const bool ldsDecoder = ns <= KNZ_ANS1_LDS_MAX_CHUNKS && knz_test_switch("KNZ_ANS1_TABLE_DECODER") == nullptr;   // (the variable lets the tests reach the other path)
        if (ldsDecoder && h->a1_cum.reserve((size_t)ns * 256 * KNZ_ANS1_CUM_STRIDE * 2 + 64))
            return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
        da.progress = nullptr;
        hipLaunchKernelGGL(knz_ans1_dec_tables_kernel, dim3(ns), dim3(256), 0, st, da, h->a1_f16.as<uint16_t>(), ldsDecoder ? h->a1_cum.as<uint16_t>() : (uint16_t*)nullptr,
                           (const uint64_t*)h->a1_ctxpos.as<uint64_t>());
        hipLaunchKernelGGL(knz_ans1_raw_kernel, dim3(ns), dim3(256), 0, st, da);
        // ... RANK+ZRLT behind the decoder: their inverses start under it, on a second stream, as one chain per block (rank_pipe.hip). The chain
        // takes the blocks it can (coded chunks, both stages applied); the regular stage kernels of inverse_sequence() take the others.
        uint32_t ptoks[8];
        const int pnt = xf ? seq_tokens(db.transform, ptoks) : 0;
        // (the fused path is an option: beyond the device's budget of spinning waves - a device that full gains nothing from the overlap - or without room
        // for its third region the batch takes the regular stage kernels)
        bool pipeWanted = ldsDecoder && h->pipe_ready && nblocks <= KNZ_PIPE_DEVICE_BLOCKS && pnt >= 2 && ptoks[pnt - 1] == KNZ_T_ZRLT && ptoks[pnt - 2] == KNZ_T_RANK && knz_test_switch("KNZ_NO_RANK_PIPE") == nullptr;
        if (pipeWanted && (h->xf_r3.reserve(xstride * nblocks + 256) || h->pipe_prog.reserve(8 * (size_t)ns + 64) || h->pipe_flag.reserve((size_t)nblocks + 64) || h->pipe_group.reserve(3 * (size_t)nblocks + 64))) {
            pipeWanted = false;
            g_alloc_refused = false;                                                  // (nothing to retry in halves: the regular path needs none of these)
        }
        if (pipeWanted && !pipeScope.take((int)nblocks)) pipeWanted = false;
        if (pipeWanted) {
            std::vector<uint8_t> ones(nblocks, 1);
            // Two launches of the chain: the blocks with the longest ZRLT streams (the long chains: stream length is what the chain's time follows) in one,
            // the others in the other. The stages behind the chain (inverse BWT ...) then run for the short blocks while the long chains are still
            // going, and only the few long blocks' stages are left when those end. One group when the lengths do not split that way.
            std::vector<uint8_t> grp(3 * (size_t)nblocks, 0);                        // [group | take of pass A | take of pass B]
            {
                uint32_t maxm = 0, nLong = 0;
                for (uint32_t b = 0; b < nblocks; b++) maxm = std::max(maxm, db.pre_len[b]);
                for (uint32_t b = 0; b < nblocks; b++) { grp[b] = (uint64_t)db.pre_len[b] * 100 > (uint64_t)maxm * 85 ? 1 : 0; nLong += grp[b]; }
                pipeGroups = nLong * 8 >= nblocks && (nblocks - nLong) * 4 >= nblocks && knz_test_switch("KNZ_RANK_PIPE_ONE_GROUP") == nullptr;
                if (knz_test_switch("KNZ_RANK_PIPE_TWO_GROUPS") != nullptr && nblocks >= 2) {            // (tests: small batches through the two-pass schedule)
                    pipeGroups = true;
                    for (uint32_t b = 0; b < nblocks; b++) grp[b] = (uint8_t)(b & 1);
                }
                if (!pipeGroups) for (uint32_t b = 0; b < nblocks; b++) grp[b] = 0;
                for (uint32_t b = 0; b < nblocks; b++) { grp[nblocks + b] = grp[b] == 0; grp[2 * (size_t)nblocks + b] = grp[b] == 1; }
            }
            HIP_OK(hipMemcpyAsync(h->pipe_group.p, grp.data(), grp.size(), hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(xb.side, ones.data(), nblocks, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(xb.take, ones.data(), nblocks, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemsetAsync(h->pipe_prog.p, 0, 8 * (size_t)ns, st));
            HIP_OK(hipMemsetAsync(h->pipe_flag.p, 0, nblocks, st));
            HIP_OK(hipStreamSynchronize(st));                                         // (`ones` is a local; the walk before is long done)
            pipeOn = true;
            h->pipe_n = nblocks;
            da.progress = h->pipe_prog.as<uint64_t>();
            RankPipeArgs pa;
            pa.nblocks = nblocks; pa.chunks_per_block = cpb; pa.info = h->a1_info.as<uint32_t>(); pa.progress = h->pipe_prog.as<uint64_t>();
            pa.cur_ptr = h->blk_off.as<uint64_t>(); pa.cur_len = h->blk_len.as<uint32_t>(); pa.skip = h->blk_skip.as<uint8_t>() + nblocks; pa.side = xb.side;
            pa.blk_status = h->blk_status.as<int32_t>(); pa.piped = h->pipe_flag.as<uint8_t>();
            pa.ranks_base = (uint64_t)h->xf_r3.p; pa.out_base = (uint64_t)h->xf_r2.p; pa.stride = xstride; pa.out_cap = xb.cap();
            pa.zrlt_stage = (uint32_t)(pnt - 1); pa.rank_stage = (uint32_t)(pnt - 2);
            pa.mode = 2;
            pa.group = pipeGroups ? h->pipe_group.as<uint8_t>() : (const uint8_t*)nullptr; pa.group_sel = 0;
            if (knz_test_switch("KNZ_RANK_UNPACKED") != nullptr) pa.mode |= 0x100;
            if (const char* cv = knz_test_switch("KNZ_RANK_CUT")) pa.mode |= ((uint32_t)atoi(cv) / 64u) << 12;
            hipEventRecord(h->ev_pipe[0], st);                                        // behind the table kernels: the chunk headers are parsed
            hipStreamWaitEvent(h->stream2, h->ev_pipe[0], 0);
            pipeScope.launched = true;
            HIP_OK(hipMemsetAsync(h->xf_r3.p, 0, xstride * nblocks, h->stream2));     // zero runs are not written, only the literals between them
            if (pipeGroups) { hipEventRecord(h->ev_pipe[2], h->stream2); hipStreamWaitEvent(h->stream3, h->ev_pipe[2], 0); }   // (the other launch starts behind the zero fill too)
            pipeArgs = pa;
        }
#ifdef KNZ_MEASURE
        if (ldsDecoder && knz_measure_switch("KNZ_ANS1_LDS1") != nullptr) KNZ_LAUNCH_PROBED(knz_ans1_decode_lds_kernel, dim3(ns), dim3(64), 0, st, da, (const uint16_t*)h->a1_cum.as<uint16_t>());   // (round-2 loop)
        else
#endif
        if (ldsDecoder) KNZ_LAUNCH_PROBED(knz_ans1_decode_lds2_kernel, dim3(ns), dim3(64), 0, st, da, (const uint16_t*)h->a1_cum.as<uint16_t>());
        else KNZ_LAUNCH_PROBED(knz_ans1_decode_kernel, dim3((ns + 15) / 16), dim3(64), 0, st, da);
        if (pipeOn) {                                                                 // the consumer goes in BEHIND the producer's launch: it never holds a CU the producer waits for
            hipStream_t st1 = st;
            if (pipeGroups) {                                                         // the long chains first (their waves start first), in their own stream
                RankPipeArgs pl = pipeArgs;
                pl.group_sel = 1;
                { hipStream_t st = h->stream3; KNZ_LAUNCH_PROBED((knz_zrlti_rank_pipe_kernel<2, 4 | 64>), dim3(nblocks), dim3(128), 0, st, pl); }
                hipEventRecord(h->ev_pipe[2], h->stream3);
            }
            { hipStream_t st = h->stream2; KNZ_LAUNCH_PROBED((knz_zrlti_rank_pipe_kernel<2, 4 | 64>), dim3(nblocks), dim3(128), 0, st, pipeArgs); }
            hipEventRecord(h->ev_pipe[1], h->stream2);
            hipStreamWaitEvent(st1, h->ev_pipe[1], 0);                                // (the long group's event is waited for between the two passes of the inverse sequence)
#if defined(KNZ_MEASURE) && !defined(KNZ_HIP_EMU)
            if (knz_measure_switch("KNZ_RANK_PROF") != nullptr) {                      // diagnostics: where every block's fused chain spent its time
                std::vector<unsigned long long> tk((size_t)std::min<uint32_t>(nblocks, 1024) * 8);
                if (hipStreamSynchronize(h->stream2) == hipSuccess && hipMemcpyFromSymbol(tk.data(), HIP_SYMBOL(g_knz_pipe_ticks), tk.size() * 8) == hipSuccess) {
                    fprintf(stderr, "fused ZRLT/RANK inverse, per block: ms chain waits / expander total / chain / total | first data at, producer done at | stream bytes -> ranks\n");
                    for (size_t q = 0; q * 8 < tk.size(); q++)
                        fprintf(stderr, "  block %2zu: %6.1f %6.1f %6.1f %6.1f | %6.1f %6.1f | %llu -> %llu\n", q, tk[8 * q] / 1e5, tk[8 * q + 1] / 1e5, tk[8 * q + 2] / 1e5,
                                tk[8 * q + 3] / 1e5, tk[8 * q + 4] / 1e5, tk[8 * q + 5] / 1e5, tk[8 * q + 6], tk[8 * q + 7]);
                }
            }
#endif
        }
    } else if (db.entropy == KNZ_E_ANS0) {
        Ans0DecArgs da;
        da.stream = db.d_stream; da.nbytes = db.nbytes; da.blk_pre_len = h->blk_len.as<uint32_t>(); da.blk_mode = h->blk_skip.as<uint8_t>();
        da.chunk_bit = h->chunk_rel.as<uint64_t>(); da.blk_out_off = h->blk_off.as<uint64_t>(); da.chunks_per_block = cpb;
        da.nslots = nblocks * cpb; da.out = nullptr; da.blk_status = h->blk_status.as<int32_t>();
        if (fusedWalk) {
            HIP_OK(hipMemsetAsync(h->chunk_rel.p, 0xFF, 8 * nslots, st));           // KNZ_CHUNK_NOT_READY
            const uint32_t gpb = (cpb + KNZ_ANS0_DEC_CHUNKS - 1) / KNZ_ANS0_DEC_CHUNKS;
            KNZ_LAUNCH_PROBED(knz_ans0_walk_decode_kernel, dim3(nblocks + nblocks * gpb), dim3(64), 0, st, wb, da);
        } else KNZ_LAUNCH_PROBED(knz_ans0_decode_kernel, dim3((nblocks * cpb + KNZ_ANS0_DEC_CHUNKS - 1) / KNZ_ANS0_DEC_CHUNKS), dim3(64), 0, st, da);
    } else {
        HufDecArgs da;
        da.stream = db.d_stream; da.nbytes = db.nbytes; da.blk_pre_len = h->blk_len.as<uint32_t>(); da.blk_mode = h->blk_skip.as<uint8_t>();
        da.chunk_bit = h->chunk_rel.as<uint64_t>(); da.blk_out_off = h->blk_off.as<uint64_t>(); da.chunks_per_block = cpb;
        da.entropy = db.entropy; da.out = nullptr; da.blk_status = h->blk_status.as<int32_t>();
        if (db.entropy == KNZ_E_HUFFMAN) {
            if (h->huf_fallback.reserve((size_t)nblocks * cpb + 64)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
            h->huf_fallback_n = (size_t)nblocks * cpb;
            if (fusedWalk) {
                HIP_OK(hipMemsetAsync(h->chunk_rel.p, 0xFF, 8 * nslots, st));       // KNZ_CHUNK_NOT_READY
                KNZ_LAUNCH_PROBED(knz_huf_walk_decode_kernel, dim3(nblocks + nblocks * cpb), dim3(256), 0, st, wb, da, h->huf_fallback.as<uint8_t>());
            } else KNZ_LAUNCH_PROBED(knz_huf_decode_par_kernel, dim3(nblocks * cpb), dim3(256), 0, st, da, h->huf_fallback.as<uint8_t>());
            hipLaunchKernelGGL(knz_huf_decode_kernel, dim3(nblocks * cpb), dim3(64), 0, st, da, (const uint8_t*)h->huf_fallback.as<uint8_t>());
        } else {
            h->huf_fallback_n = 0;
            hipLaunchKernelGGL(knz_huf_decode_kernel, dim3(nblocks * cpb), dim3(64), 0, st, da, (const uint8_t*)nullptr);
        }
    }
    hipEventRecord(h->ev[2], st);
    if (xf) {
        if (!pipeOn) {
            std::vector<uint8_t> ones(nblocks, 1);
            HIP_OK(hipMemcpyAsync(xb.side, ones.data(), nblocks, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(xb.take, ones.data(), nblocks, hipMemcpyHostToDevice, st));
            HIP_OK(hipStreamSynchronize(st));
        } else {
            xb.piped = h->pipe_flag.as<uint8_t>(); xb.piped_zrlt = (int)pipeArgs.zrlt_stage; xb.piped_rank = (int)pipeArgs.rank_stage;
        }
        xb.cur_ptr = h->blk_off.as<uint64_t>(); xb.cur_len = h->blk_len.as<uint32_t>(); xb.skip = h->blk_skip.as<uint8_t>() + nblocks;
        xb.blk_status = h->blk_status.as<int32_t>();
        int rc;
        if (pipeOn && pipeGroups) {
            uint8_t* takeAll = xb.take;
            xb.take = h->pipe_group.as<uint8_t>() + nblocks;                          // pass A: the blocks of the short chains, while the long ones run
            rc = inverse_sequence(h, xb, db.transform, st);
            if (rc) return rc;
            hipStreamWaitEvent(st, h->ev_pipe[2], 0);
            xb.take = h->pipe_group.as<uint8_t>() + 2 * (size_t)nblocks;              // pass B: the blocks of the long chains
            rc = inverse_sequence(h, xb, db.transform, st);
            xb.take = takeAll;
        } else rc = inverse_sequence(h, xb, db.transform, st);
        if (rc) return rc;
        HIP_OK(hipMemcpyAsync(db.pre_len.data(), h->blk_len.p, 4 * (size_t)nblocks, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(db.status.data(), h->blk_status.p, 4 * (size_t)nblocks, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        std::vector<uint64_t> dstp(nblocks);
        for (uint32_t b = 0; b < nblocks; b++) {
            if (db.status[b]) return knz_set_error(h, db.status[b], "inverse transform failed");
            if (db.pre_len[b] > db.block_size || (db.pre_len[b] > db.out_stride && b + 1 < nblocks))   // Reader.processBlock :1707-1710
                return knz_set_error(h, KNZ_ERR_PROCESS_BLOCK, "block decodes to more than the stream block size");
            if ((uint64_t)b * db.out_stride + db.pre_len[b] > db.out_cap) return knz_set_error(h, KNZ_ERR_WRITE_FILE, "destination buffer too small");
            dstp[b] = (uint64_t)db.d_out + (uint64_t)b * db.out_stride;
        }
        HIP_OK(hipMemcpyAsync(xb.out_ptr, dstp.data(), 8 * (size_t)nblocks, hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));
        hipLaunchKernelGGL(knz_copy_blocks_kernel, dim3(64, nblocks), dim3(256), 0, st, nblocks, xb.cur_ptr, xb.cur_len, xb.out_ptr, (const uint8_t*)nullptr);
    }
    if (db.checksum_bits != 0 && !db.payload_only) {   // decodingTask.decode :1992-2007: hash of the decoded block vs the header field
        XxhArgs xa;
        xa.nblocks = nblocks; xa.len = h->blk_len.as<uint32_t>(); xa.cksum = h->blk_cksum.as<uint64_t>(); xa.status = h->blk_status.as<int32_t>();
        xa.ptr = xf ? xb.out_ptr : h->blk_off.as<uint64_t>();
        xa.mode = nullptr; xa.bits = db.checksum_bits; xa.verify = 1;
        hipLaunchKernelGGL(knz_xxhash_kernel, dim3(nblocks), dim3(64), 0, st, xa);
    }
    hipEventRecord(h->ev[3], st);
    hipEventRecord(h->ev[4], st);
    h->ev_valid = true;
    HIP_OK(hipMemcpyAsync(db.status.data(), h->blk_status.p, 4 * (size_t)nblocks, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(db.end_bit.data(), h->dec_tables.p, 8 * (size_t)nblocks, hipMemcpyDeviceToHost, st));
    if (direct) HIP_OK(hipMemcpyAsync(db.pre_len.data(), h->blk_len.p, 4 * (size_t)nblocks, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    for (uint32_t b = 0; b < nblocks; b++) {
        if (db.status[b]) return knz_set_error(h, db.status[b], db.status[b] == KNZ_ERR_CRC_CHECK ? "Corrupted bitstream: checksum mismatch" : "invalid entropy payload");
        db.total_out += db.pre_len[b];
    }
    return KNZ_OK;
}

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

extern "C" int knz_dev_decompress(void* handle, const void* d_src, uint64_t n_bytes, void* d_dst, uint64_t dst_cap,
                                  uint64_t* out_bytes, void* hip_stream) {
    Handle* h = lane_of_pointer((Handle*)handle, d_dst);
    if (!h || !d_src || !d_dst || !out_bytes) return KNZ_ERR_MISSING_PARAM;
    DeviceGuard dg(h);
    if ((uintptr_t)d_src & 3) return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "d_src must be 4-byte aligned");
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->stream;
    uint8_t hdr[32] = {0};
    HIP_OK(hipMemcpyAsync(hdr, d_src, std::min<uint64_t>(32, n_bytes), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    knz_cfg sc = h->cfg;
    int64_t outputSize = 0;
    uint32_t hbits = 0;
    int rc = parse_stream_header(h, hdr, n_bytes, sc, outputSize, hbits);
    if (rc) return rc;
    DecodeBatch db;
    db.d_stream = (const uint8_t*)d_src; db.nbytes = n_bytes; db.framed = 1; db.first_bit = hbits; db.seg_bits = 0; db.nblocks = 0;
    db.d_out = (uint8_t*)d_dst; db.out_cap = dst_cap; db.out_stride = sc.block_size; db.payload_only = 0; db.given_len = 0;
    db.entropy = sc.entropy; db.checksum_bits = sc.checksum_bits; db.block_size = sc.block_size; db.transform = sc.transform;
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

extern "C" int knz_dev_decompress_blocks(void* handle, const void* d_src, uint64_t n_bits, void* d_dst, uint64_t dst_cap,
                                         uint64_t* out_bytes, void* hip_stream) {
    Handle* h = lane_of_pointer((Handle*)handle, d_dst);
    if (!h || !d_src || !d_dst || !out_bytes) return KNZ_ERR_MISSING_PARAM;
    DeviceGuard dg(h);
    if ((uintptr_t)d_src & 3) return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "d_src must be 4-byte aligned");
    *out_bytes = 0;
    if (n_bits == 0) return KNZ_OK;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->stream;
    DecodeBatch db;
    db.d_stream = (const uint8_t*)d_src; db.nbytes = (n_bits + 7) >> 3; db.framed = 1; db.first_bit = 0; db.seg_bits = n_bits; db.nblocks = 0;
    db.d_out = (uint8_t*)d_dst; db.out_cap = dst_cap; db.out_stride = h->cfg.block_size; db.payload_only = 0; db.given_len = 0;
    db.entropy = h->cfg.entropy; db.checksum_bits = h->cfg.checksum_bits; db.block_size = h->cfg.block_size; db.transform = h->cfg.transform;
    int rc = decode_batch(h, db, st);
    if (rc) return rc;
    *out_bytes = db.total_out;
    return KNZ_OK;
}

// ---- host-pointer batch entry points ------------------------------------------------------------------------------------
static int encode_blocks_once(Handle* h, knz_block* blocks, int n);
static int decode_blocks_once(Handle* h, knz_block* blocks, int n);
// A batch whose workspace the device cannot hold any more (other handles, other tenants) is taken in halves after the handle's own workspace
// has been given back: blocks are independent (Definitions.go:73-77), so the result is the same, with fewer of them side by side.
template <typename F>
static int blocks_split_retry(Handle* h, knz_block* blocks, int n, F once) {
    g_alloc_refused = false;
    int rc = once(h, blocks, n);
    if (rc == KNZ_OK || !g_alloc_refused) return rc;
    knz_release_workspace(h);
    g_alloc_refused = false;
    if (n == 1) return once(h, blocks, n);                    // (once more with nothing else of this handle resident)
    const int half = n / 2;
    rc = blocks_split_retry(h, blocks, half, once);
    if (rc) return rc;
    return blocks_split_retry(h, blocks + half, n - half, once);
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
    hipStream_t st = h->hstream ? h->hstream : h->stream;
    const uint64_t bs = h->cfg.block_size;
    // stage the blocks at block_size stride; all but the last must be full for the shared block table
    for (int i = 0; i < n; i++) {
        blocks[i].status = 0;
        if (!blocks[i].src || !blocks[i].dst || blocks[i].src_len == 0 || blocks[i].src_len > bs) return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "invalid block descriptor");
        if (i + 1 < n && blocks[i].src_len != bs) return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "only the last block of a batch may be short");
    }
    const uint64_t total = (uint64_t)(n - 1) * bs + blocks[n - 1].src_len;
    const uint64_t ostride = ((uint64_t)knz_max_encoded_len(h->cfg.transform, (uint32_t)bs) * 12 / 8 + 1024 + (h->cfg.entropy == KNZ_E_ANS1 ? 131072ull * (bs / (4u << 20) + 2) : 0) + 63) & ~(uint64_t)63;
    if (h->stage_in.reserve(total + 64) || h->stage_out.reserve(ostride * n + 64)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
    for (int i = 0; i < n; i++)
        HIP_OK(hipMemcpyAsync(h->stage_in.as<uint8_t>() + (uint64_t)i * bs, blocks[i].src, blocks[i].src_len, hipMemcpyHostToDevice, st));
    EncodeBatch eb{h->stage_in.as<uint8_t>(), total, h->stage_out.as<uint8_t>(), ostride * n + 64, 0, 0, 0, 0, ostride, 0, 0};
    int rc = encode_batch(h, eb, st);
    if (rc) { for (int i = 0; i < n; i++) blocks[i].status = rc; return rc; }
    const Handle::ResultRow* rows = h->pinned_rows;   // (filled by encode_batch: nothing more to bring over but the streams themselves)
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
static int decode_blocks_once(Handle* h, knz_block* blocks, int n) {
    hipStream_t st = h->hstream ? h->hstream : h->stream;
    const uint64_t bs = h->cfg.block_size;
    uint64_t total = 0;
    std::vector<uint64_t> bit(n), bits(n);
    for (int i = 0; i < n; i++) {
        blocks[i].status = 0;
        if (!blocks[i].src || !blocks[i].dst || blocks[i].src_len == 0) return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "invalid block descriptor");
        bit[i] = total * 8;
        bits[i] = (uint64_t)blocks[i].src_len * 8;
        total += ((uint64_t)blocks[i].src_len + 7) & ~(uint64_t)7;
    }
    const uint64_t ostride = (bs + 63) & ~(uint64_t)63;
    if (h->stage_in.reserve(total + 64) || h->stage_out.reserve(ostride * n + 64) || h->blk_dst_bit.reserve(8 * (size_t)n + 8) ||
        h->blk_written.reserve(8 * (size_t)n + 8))
        return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
    HIP_OK(hipMemsetAsync(h->stage_in.p, 0, total + 64, st));
    for (int i = 0; i < n; i++)
        HIP_OK(hipMemcpyAsync(h->stage_in.as<uint8_t>() + (bit[i] >> 3), blocks[i].src, blocks[i].src_len, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(h->blk_dst_bit.p, bit.data(), 8 * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(h->blk_written.p, bits.data(), 8 * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
    DecodeBatch db;
    db.d_stream = h->stage_in.as<uint8_t>(); db.nbytes = total; db.framed = 0; db.first_bit = 0; db.seg_bits = 0; db.nblocks = (uint32_t)n;
    db.d_out = h->stage_out.as<uint8_t>(); db.out_cap = ostride * n; db.out_stride = ostride; db.payload_only = 0; db.given_len = 0;
    db.entropy = h->cfg.entropy; db.checksum_bits = h->cfg.checksum_bits; db.block_size = (uint32_t)bs; db.transform = h->cfg.transform;
    int rc = decode_batch(h, db, st);
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
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->stream;
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
static int transform_single(Handle* h, uint64_t type1, bool forward, const uint8_t* src, uint32_t n, uint8_t* dst, uint32_t cap, uint32_t* out_n) {
    if (!xf_codec((uint32_t)type1)) return knz_set_error(h, KNZ_ERR_INVALID_CODEC, "transform has no device implementation in this build");
    *out_n = 0;
    if (n == 0 || cap == 0) return KNZ_OK;                                  // every Forward/Inverse returns (0,0,nil) on empty input
    if (type1 == KNZ_T_NONE) {
        if (cap < n) return forward ? KNZ_SKIP : knz_set_error(h, KNZ_ERR_PROCESS_BLOCK, "Destination buffer too small");
        memcpy(dst, src, n);                                                // NullTransform: nothing for the device to do
        *out_n = n;
        return KNZ_OK;
    }
    hipStream_t st = h->hstream ? h->hstream : h->stream;
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
    Handle* h = lane0((Handle*)handle);
    if (!h || !src || !dst || !out_n) return KNZ_ERR_MISSING_PARAM;
    DeviceGuard dg(h);
    return transform_single(h, type1, true, src, n, dst, cap, out_n);
}

extern "C" int knz_transform_inverse(void* handle, uint64_t type1, const uint8_t* src, uint32_t n, uint8_t* dst, uint32_t cap, uint32_t* out_n) {
    Handle* h = lane0((Handle*)handle);
    if (!h || !src || !dst || !out_n) return KNZ_ERR_MISSING_PARAM;
    DeviceGuard dg(h);
    return transform_single(h, type1, false, src, n, dst, cap, out_n);
}

extern "C" int knz_entropy_encode(void* handle, uint32_t type, const uint8_t* src, uint32_t n, uint8_t* bits, uint64_t cap_bytes, uint64_t* out_bits) {
    Handle* h = lane0((Handle*)handle);
    if (!h || (!src && n) || !bits || !out_bits) return KNZ_ERR_MISSING_PARAM;
    DeviceGuard dg(h);
    if (!entropy_on_device(type)) return knz_set_error(h, KNZ_ERR_INVALID_CODEC, "entropy codec has no device implementation in this build");
    *out_bits = 0;
    if (n == 0) return KNZ_OK;                 // HuffmanEncoder.Write(len 0) writes nothing (:395-397)
    if (n > (1u << 30)) return knz_set_error(h, KNZ_ERR_BLOCK_SIZE, "Invalid block size parameter (max is 1<<30)");   // FPAQCodec.go:128-130 and friends
    hipStream_t st = h->hstream ? h->hstream : h->stream;
    knz_cfg saved = h->cfg;
    h->cfg.entropy = type; h->cfg.transform = 0; h->cfg.checksum_bits = 0;
    h->cfg.block_size = std::max<uint32_t>(1024, (n + 15) & ~15u);
    const uint64_t ocap = (uint64_t)n * 2 + 262144;       // rANS order 1 spends up to 110 KB of headers per 4 MiB chunk
    int rc = KNZ_OK;
    if (h->stage_in.reserve((uint64_t)n + 64) || h->stage_out.reserve(ocap + 64)) rc = knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
    uint64_t written = 0;
    if (!rc) {
        hipMemcpyAsync(h->stage_in.p, src, n, hipMemcpyHostToDevice, st);
        EncodeBatch eb{h->stage_in.as<uint8_t>(), n, h->stage_out.as<uint8_t>(), ocap + 64, 0, 0, 0, 0, ocap, 1, 0};
        rc = encode_batch(h, eb, st);
        if (!rc) written = h->pinned_rows[0].written;       // (the batch's result rows are on the host already)
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
    hipStream_t st = h->hstream ? h->hstream : h->stream;
    const uint64_t padded = (n_bytes + 7) & ~(uint64_t)7;
    if (h->stage_in.reserve(padded + 64) || h->stage_out.reserve((uint64_t)n + 64) || h->blk_dst_bit.reserve(16) || h->blk_written.reserve(16))
        return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
    HIP_OK(hipMemsetAsync(h->stage_in.p, 0, padded + 64, st));
    HIP_OK(hipMemcpyAsync(h->stage_in.p, bits, n_bytes, hipMemcpyHostToDevice, st));
    uint64_t zero = 0, nb = n_bytes * 8;
    HIP_OK(hipMemcpyAsync(h->blk_dst_bit.p, &zero, 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(h->blk_written.p, &nb, 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
    DecodeBatch db;
    db.d_stream = h->stage_in.as<uint8_t>(); db.nbytes = padded; db.framed = 0; db.first_bit = 0; db.seg_bits = 0; db.nblocks = 1;
    db.d_out = h->stage_out.as<uint8_t>(); db.out_cap = n; db.out_stride = n; db.payload_only = 1; db.given_len = n;
    db.entropy = type; db.checksum_bits = 0; db.block_size = std::max<uint32_t>(1024, n); db.transform = 0;
    int rc = decode_batch(h, db, st);
    if (rc) return rc;
    HIP_OK(hipMemcpyAsync(dst, h->stage_out.p, n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (used_bits) *used_bits = db.end_bit[0];
    return KNZ_OK;
}
