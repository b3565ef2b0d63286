// The batch scheduler (included by knz_gpu.hip behind knz_transforms.inc): encode_batch and decode_batch, the entropy stage between the transform
// pipeline and the stream layout with one function per codec and direction (the rows of kEntropyCodecs), and the host side of the fused
// ZRLT / RANK chain that runs under the rANS-1 decoder.

// ---- encode batch ----------------------------------------------------------------------------------------------------
// d_src: nblocks blocks, block b at b*block_size (last one shorter). Output either the framed .knz body/stream
// (framed=1) or per-block local streams at out_stride bytes (framed=0). Made by one of the four named forms below.
struct EncodeBatch {
    const uint8_t* d_src; uint64_t n;
    uint8_t* d_dst; uint64_t dst_cap;
    int framed = 0, with_header = 0, with_end = 0; int64_t header_input_size = 0;
    uint64_t out_stride = 0; // framed == 0
    int payload_only = 0;    // 1: single EntropyEncoder object, no block header bits
    int keep_probes = 0;     // 1: the kernel probes of the call so far stay, this batch's follow them (knz_dev_write_many: its overlay runs in front)
    uint64_t total_bits = 0; // result
    // several streams in one batch (knz_many.inc; on block_streams): the blocks are those of a table of streams, `blocks` of them, none longer than
    // max_len; a block that fails leaves its status in blk_status for the caller instead of failing the batch
    struct Many { const ManyStream* streams = nullptr; uint32_t n_streams = 0, blocks = 0, max_len = 0; uint32_t* blk_stream = nullptr; } many;
    // a whole .knz stream (header, framed blocks, end marker) ; a segment of one (framed blocks only) ; block-local streams, block b's at dst + b * stride
    // (count of them, 64 bytes of slack behind the last) ; the bare payload of a single EntropyEncoder object (one block-local stream, no block header)
    static EncodeBatch stream(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t cap, int64_t header_input_size) {
        EncodeBatch eb = segment(src, n, dst, cap); eb.with_header = eb.with_end = 1; eb.header_input_size = header_input_size; return eb;
    }
    static EncodeBatch segment(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t cap) { EncodeBatch eb(src, n, dst, cap); eb.framed = 1; return eb; }
    static EncodeBatch block_streams(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t stride, uint64_t count) {
        EncodeBatch eb(src, n, dst, stride * count + 64); eb.out_stride = stride; return eb;
    }
    static EncodeBatch payload(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t cap) { EncodeBatch eb = block_streams(src, n, dst, cap, 1); eb.payload_only = 1; return eb; }
private:
    EncodeBatch(const uint8_t* src, uint64_t nn, uint8_t* dst, uint64_t cap) : d_src(src), n(nn), d_dst(dst), dst_cap(cap) {}
};

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
    // several streams in one batch (knz_many.inc): every failing block is marked in `status`, not only the first ; done: the batch ran to its end
    // (a block that failed then leaves the others as they are)
    bool many = false, done = false;
    // a framed stream with the codec parameters of `c` (the handle's, or a stream header's), blocks placed at block_size: call sites state what differs
    DecodeBatch(const knz_cfg& c, const uint8_t* stream, uint64_t n, uint8_t* out, uint64_t cap)
        : d_stream(stream), nbytes(n), framed(1), first_bit(0), seg_bits(0), nblocks(0), d_out(out), out_cap(cap), out_stride(c.block_size),
          payload_only(0), given_len(0), entropy(c.entropy), checksum_bits(c.checksum_bits), block_size(c.block_size), transform(c.transform), total_out(0) {}
    // ... staged payloads instead of a stream: n of them, their bit positions already on the device (dec_stage_payloads, many.hip), block b decoded to out + b * stride
    void unframed(uint32_t n, uint64_t stride) { framed = 0; nblocks = n; out_stride = stride; }
    // ... a range of the stream's blocks instead of all of them: the walk starts at `bit` as block first_id (the first block of a stream is 1), skips the
    // frames in front of `from`, stops behind block to - 1 (~0: the last). Everything behind the walk is sized by the blocks it found: those of the range.
    // hinted: `bit` is a caller's word, not the header's: the frame there has to be a block
    bool ranged = false, rg_hinted = false; uint64_t rg_first_id = 1, rg_from = 1, rg_to = ~(uint64_t)0;
    void range(uint64_t bit, uint64_t first_id, uint64_t from, uint64_t to, bool hinted) {
        ranged = true; rg_hinted = hinted; first_bit = bit; rg_first_id = first_id; rg_from = from; rg_to = to;
    }
    // block b failed with rc: true = stop at this first one ; with `many` it is marked, `first` keeps the first code and the batch goes on
    bool block_failed(uint32_t b, int rc, int& first) { status[b] = rc; if (!first) first = rc; return !many; }
};

// ---- entropy stage, encode side: one function per codec ----------------------------------------------------------------
// what an arm reads from encode_batch, and what the Huffman arm hands back to it
struct EncStage {
    uint32_t nblocks, cpb, slotStride; size_t nslots; bool skipOpt;
    bool hufDirect = false;                                              // Huffman units encoded at their final bit positions (encode_batch, behind the layout)
    HufEncArgs hufArgs;
};

// the fields every encoder's argument struct has (and CopyUnitsArgs), assigned by name: the structs share no base, their layouts are the kernels' ABI
template <class A> static void enc_io(A& a, Handle* h, uint32_t cpb) {
    a.blk_off = h->blk_off.as<uint64_t>(); a.blk_len = h->blk_len.as<uint32_t>(); a.chunks_per_block = cpb;
    a.scratch = h->scratch.as<uint8_t>(); a.unit_bits = h->unit_bits.as<uint32_t>(); a.unit_src = h->unit_src.as<uint32_t>();
    a.blk_status = h->blk_status.as<int32_t>();
}
// ... restricted to the blocks from b0 on (slots from s0 on): the slice of every per-block / per-slot table
template <class A> static void enc_group(A& a, uint32_t b0, size_t s0, uint32_t slotStride) {
    a.blk_off += b0; a.blk_len += b0; a.blk_status += b0;
    a.scratch += s0 * slotStride; a.unit_bits += s0 * KNZ_UNITS_PER_CHUNK; a.unit_src += s0 * KNZ_UNITS_PER_CHUNK;
}

static int huf_encode_stage(Handle* h, EncStage& s, hipStream_t st) {      // HUFFMAN, and NONE (raw units)
    const uint32_t nblocks = s.nblocks, cpb = s.cpb;
    HufEncArgs a;
    enc_io(a, h, cpb); a.data = nullptr;
    if (h->cfg.entropy == KNZ_E_HUFFMAN) {
        const uint32_t nc = nblocks * cpb, groups = (nc + 63) / 64;
        if (h->huf_stfreq.reserve((size_t)groups * 256 * 64 * 2) || h->huf_stsym.reserve((size_t)groups * 256 * 64) ||
            h->huf_stlen.reserve((size_t)groups * 256 * 64) || h->huf_stcnt.reserve((size_t)groups * 64 * 2) || h->huf_stmax.reserve((size_t)groups * 64))
            return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
        a.st_freq = h->huf_stfreq.as<uint16_t>(); a.st_sym = h->huf_stsym.as<uint8_t>(); a.st_len = h->huf_stlen.as<uint8_t>();
        a.st_count = h->huf_stcnt.as<uint16_t>(); a.st_maxlen = h->huf_stmax.as<uint8_t>(); a.nchunks = nc;
        // The units are encoded at their final bit positions (sizes pass -> layout scans -> encoder, further down) unless copy blocks of -s
        // have to overwrite chunks afterwards or the test switch asks for the scratch-slot form (units to slots, knz_gather_kernel).
        s.hufDirect = !s.skipOpt && knz_test_switch("KNZ_HUF_SCRATCH") == nullptr;
        a.st_fhist = nullptr; a.dst_words = nullptr; a.chunk_rel = nullptr; a.blk_dst_bit = nullptr; a.total_bits = nullptr;
        if (s.hufDirect) {
            if (h->huf_fhist.reserve((size_t)nc * 4 * 256 * 2 + 64)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
            a.st_fhist = h->huf_fhist.as<uint16_t>();
        }
        KNZ_LAUNCH_PROBED(knz_huf_hist_kernel, dim3(nc), dim3(256), 0, st, a);
        KNZ_LAUNCH_PROBED(knz_huf_lengths_kernel, dim3(groups), dim3(64), 0, st, a);
        if (s.hufDirect) { KNZ_LAUNCH_PROBED(knz_huf_encode_kernel<true>, dim3(nc), dim3(256), 0, st, a); s.hufArgs = a; }
        else KNZ_LAUNCH_PROBED(knz_huf_encode_kernel<false>, dim3(nc), dim3(256), 0, st, a);
    }
    else hipLaunchKernelGGL(knz_raw_units_kernel, dim3(nblocks * cpb), dim3(256), 0, st, a);
    return KNZ_OK;
}

static int fpaq_encode_stage(Handle* h, EncStage& s, hipStream_t st) {
    FpaqArgs a;
    enc_io(a, h, s.cpb); a.blk_src_len = h->blk_src_len.as<uint32_t>();
    KNZ_LAUNCH_PROBED(knz_fpaq_encode_kernel, dim3(s.nblocks), dim3(64), 0, st, a);
    return KNZ_OK;
}

static int ans1_encode_stage(Handle* h, EncStage& s, hipStream_t st) {
    const uint32_t nblocks = s.nblocks, cpb = s.cpb;
    // bounded groups of blocks (like the UTF stage and the suffix sort): a chunk slot takes 768 KiB of count / coder tables, 112 KiB of
    // context headers and the 64 MiB expanded-step stream; the workspace is sized to at most ~64 GiB of them (up to ~960 chunks side by side: the chains of a group run as one wave each, 25 ms whatever their number), not to the batch
    const size_t perSlot = (size_t)65536 * 12 + (size_t)256 * KNZ_ANS1_CTXHDR_BYTES + 1024 + KNZ_ANS1_ENT_STRIDE * 16;
    const uint32_t slotsPerGroup = (uint32_t)std::max<size_t>(cpb, std::min<size_t>((size_t)nblocks * cpb, ((size_t)64 << 30) / perSlot));
    uint32_t GB = std::max<uint32_t>(1, slotsPerGroup / cpb);                   // whole blocks per group
    if (const char* e = knz_test_switch("KNZ_ANS1_GROUP_BLOCKS")) GB = std::max(1, atoi(e));   // (tests: several groups on small inputs)
    const bool ans1EncPlain = knz_test_switch("KNZ_ANS1_ENC_PLAIN") != nullptr;   // (A/B and cross-check: the compiler's loop instead of the hand-written one)
    const bool ans1EncOneWave = knz_test_switch("KNZ_ANS1_ENC_ONE_WAVE") != nullptr;   // (A/B and cross-check: the one-wave kernel, which places its words itself)
    // a group the device has no room for (other handles, a smaller device) is halved until it fits: fewer chains side by side, same bytes
    uint32_t gs = GB * cpb;
    for (;;) {
        gs = GB * cpb;
        if (!(h->a1_freqs.reserve((size_t)gs * 65536 * 4) || h->a1_tab.reserve((size_t)gs * 65536 * 8) ||
              h->a1_ctxhdr.reserve((size_t)gs * 256 * KNZ_ANS1_CTXHDR_BYTES + 64) || h->a1_ctxbits.reserve((size_t)gs * 256 * 4) ||
              h->a1_ent.reserve((size_t)gs * KNZ_ANS1_ENT_STRIDE * 16)))
            break;
        if (GB == 1) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
        h->a1_freqs.release(); h->a1_tab.release(); h->a1_ctxhdr.release(); h->a1_ctxbits.release(); h->a1_ent.release();
        GB = (GB + 1) / 2;
    }
    for (uint32_t b0 = 0; b0 < nblocks; b0 += GB) {
        const uint32_t gb = std::min<uint32_t>(GB, nblocks - b0), ns = gb * cpb;
        const size_t s0 = (size_t)b0 * cpb;
        Ans1Args a;                                                                // the group's slice of every per-block / per-slot table
        enc_io(a, h, cpb); enc_group(a, b0, s0, s.slotStride); a.nslots = ns;
        a.freqs = h->a1_freqs.as<uint32_t>(); a.tab = h->a1_tab.as<uint2>(); a.ctx_hdr = h->a1_ctxhdr.as<uint8_t>();
        a.ctx_bits = h->a1_ctxbits.as<uint32_t>();
        hipMemsetAsync(h->a1_freqs.p, 0, (size_t)ns * 65536 * 4, st);
        KNZ_LAUNCH_PROBED(knz_ans1_hist_kernel, dim3(ns * KNZ_ANS1_HIST_WGS * KNZ_ANS1_HIST_SLICES), dim3(256), 0, st, a);
        hipLaunchKernelGGL(knz_ans1_stats_kernel, dim3(ns * 256), dim3(64), 0, st, a);
        hipLaunchKernelGGL(knz_ans1_merge_kernel, dim3(ns), dim3(256), 0, st, a);
        KNZ_LAUNCH_PROBED(knz_ans1_expand_kernel, dim3(ns, 128), dim3(256), 0, st, a, h->a1_ent.as<uint4>());
        // two waves a chunk: one codes, one places the renormalisation words (ans1.hip); the emulator has the same two waves around the C++ step
        if (!ans1EncPlain && !ans1EncOneWave) KNZ_LAUNCH_PROBED(knz_ans1_encode_asm_kernel, dim3(ns), dim3(128), 0, st, a, (const uint4*)h->a1_ent.as<uint4>());
#ifndef KNZ_HIP_EMU
        else if (!ans1EncPlain) KNZ_LAUNCH_PROBED(knz_ans1_encode_asm1_kernel, dim3(ns), dim3(64), 0, st, a, (const uint4*)h->a1_ent.as<uint4>());
#endif
        else KNZ_LAUNCH_PROBED(knz_ans1_encode_kernel, dim3(ns), dim3(64), 0, st, a, (const uint4*)h->a1_ent.as<uint4>());
    }
    return KNZ_OK;
}

static int ans0_encode_stage(Handle* h, EncStage& s, hipStream_t st) {
    Ans0Args a;
    enc_io(a, h, s.cpb); a.data = nullptr;
    a.tab = h->ans_tab.as<uint2>(); a.chunk_info = (uint32_t*)(h->ans_tab.as<uint8_t>() + s.nslots * 2048);   // (kEntropyCodecs: 2048 + 4 bytes of ans_tab per slot)
    const uint32_t ns = s.nblocks * s.cpb;
    hipLaunchKernelGGL(knz_ans0_stats_kernel, dim3(ns), dim3(256), 0, st, a);
    KNZ_LAUNCH_PROBED(knz_ans0_encode_kernel, dim3((ns + KNZ_ANS0_CHUNKS_PER_WG - 1) / KNZ_ANS0_CHUNKS_PER_WG), dim3(128), 0, st, a, ns);
    return KNZ_OK;
}

// ---- the fused ZRLT / RANK chain under the rANS-1 decoder, host side ------------------------------------------------------------------
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

struct RankPipe {
    PipeScope scope;
    bool on = false, groups = false;                 // the chain runs ; in two launches (the long chains, the short ones), the stages behind it in two passes
    RankPipeArgs args{};
    uint8_t* take[2] = {nullptr, nullptr};           // groups: the blocks of pass A (short chains) and of pass B (long chains) of the inverse sequence
    explicit RankPipe(Handle* h) : scope(h) {}
};

// ---- entropy stage, decode side: one function per codec ----------------------------------------------------------------
// what the phases of decode_batch share; the arms read nblocks, cpb, nslots, fusedWalk, wb, and the rANS-1 arm hands back the state of the fused chain
struct DecStage {
    DecodeBatch& db;
    uint32_t nblocks, cpb; size_t nslots;
    WalkBlocksArgs wb;                               // the header pass's arguments: the fused walk + decode launches take them again
    bool fusedWalk, direct, xf;                      // chunk walk inside the decoders' launch ; ... and nothing behind the decode ; a transform stage follows
    XfBatch xb; uint64_t xstride = 0;                // xf: the batch in the transform pipeline's regions
    RankPipe pipe;
    DecStage(Handle* h, DecodeBatch& b) : db(b), pipe(h) {}
};

// the fields every decoder's argument struct begins with, assigned by name: the structs share no base (they diverge behind a 52-byte head, and their
// layouts are the kernels' ABI)
template <class A> static void dec_io(A& a, const DecodeBatch& db, Handle* h, uint32_t cpb) {
    a.stream = db.d_stream; a.nbytes = db.nbytes; a.blk_pre_len = h->blk_len.as<uint32_t>(); a.blk_mode = h->blk_skip.as<uint8_t>();
    a.chunk_bit = h->chunk_rel.as<uint64_t>(); a.blk_out_off = h->blk_off.as<uint64_t>(); a.chunks_per_block = cpb;
    a.blk_status = h->blk_status.as<int32_t>();
}

// Plan, in front of the decoder's launch (behind its table kernels): is the batch eligible, is there room (workspace, the device's budget), which blocks go
// in which launch; then the uploads, the zero fills and the wiring of the side streams. Leaves d.pipe.on == false where the regular stage kernels take over.
static int rank_pipe_plan(Handle* h, DecStage& d, bool ldsDecoder, hipStream_t st) {
    const DecodeBatch& db = d.db;
    XfBatch& xb = d.xb;
    RankPipe& pipe = d.pipe;
    const uint32_t nblocks = d.nblocks, cpb = d.cpb, ns = nblocks * cpb;
    const uint64_t xstride = d.xstride;
    uint32_t ptoks[8];
    const int pnt = d.xf ? seq_tokens(db.transform, ptoks) : 0;
    // (the fused path is an option: beyond the device's budget of spinning waves - a device that full gains nothing from the overlap - or without room
    // for its third region the batch takes the regular stage kernels)
    bool pipeWanted = ldsDecoder && h->pipe_ready && nblocks <= KNZ_PIPE_DEVICE_BLOCKS && pnt >= 2 && ptoks[pnt - 1] == KNZ_T_ZRLT && ptoks[pnt - 2] == KNZ_T_RANK && knz_test_switch("KNZ_NO_RANK_PIPE") == nullptr;
    if (pipeWanted && (h->xf_r3.reserve(xstride * nblocks + 256) || h->pipe_prog.reserve(8 * (size_t)ns + 64) || h->pipe_flag.reserve((size_t)nblocks + 64) || h->pipe_group.reserve(3 * (size_t)nblocks + 64))) {
        pipeWanted = false;
        g_alloc_refused = false;                                                  // (nothing to retry in halves: the regular path needs none of these)
    }
    if (pipeWanted && !pipe.scope.take((int)nblocks)) pipeWanted = false;
    if (!pipeWanted) return KNZ_OK;
    std::vector<uint8_t> ones(nblocks, 1);
    // Two launches of the chain: the blocks with the longest ZRLT streams (the long chains: stream length is what the chain's time follows) in one,
    // the others in the other. The stages behind the chain (inverse BWT ...) then run for the short blocks while the long chains are still
    // going, and only the few long blocks' stages are left when those end. One group when the lengths do not split that way.
    std::vector<uint8_t> grp(3 * (size_t)nblocks, 0);                        // [group | take of pass A | take of pass B]
    {
        uint32_t maxm = 0, nLong = 0;
        for (uint32_t b = 0; b < nblocks; b++) maxm = std::max(maxm, db.pre_len[b]);
        for (uint32_t b = 0; b < nblocks; b++) { grp[b] = (uint64_t)db.pre_len[b] * 100 > (uint64_t)maxm * 85 ? 1 : 0; nLong += grp[b]; }
        pipe.groups = nLong * 8 >= nblocks && (nblocks - nLong) * 4 >= nblocks && knz_test_switch("KNZ_RANK_PIPE_ONE_GROUP") == nullptr;
        if (knz_test_switch("KNZ_RANK_PIPE_TWO_GROUPS") != nullptr && nblocks >= 2) {            // (tests: small batches through the two-pass schedule)
            pipe.groups = true;
            for (uint32_t b = 0; b < nblocks; b++) grp[b] = (uint8_t)(b & 1);
        }
        if (!pipe.groups) for (uint32_t b = 0; b < nblocks; b++) grp[b] = 0;
        for (uint32_t b = 0; b < nblocks; b++) { grp[nblocks + b] = grp[b] == 0; grp[2 * (size_t)nblocks + b] = grp[b] == 1; }
    }
    HIP_OK(hipMemcpyAsync(h->pipe_group.p, grp.data(), grp.size(), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(xb.side, ones.data(), nblocks, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(xb.take, ones.data(), nblocks, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(h->pipe_prog.p, 0, 8 * (size_t)ns, st));
    HIP_OK(hipMemsetAsync(h->pipe_flag.p, 0, nblocks, st));
    HIP_OK(hipStreamSynchronize(st));                                         // (`ones` is a local; the walk before is long done)
    pipe.on = true;
    h->pipe_n = nblocks;
    if (pipe.groups) { pipe.take[0] = h->pipe_group.as<uint8_t>() + nblocks; pipe.take[1] = h->pipe_group.as<uint8_t>() + 2 * (size_t)nblocks; }
    RankPipeArgs pa;
    pa.nblocks = nblocks; pa.chunks_per_block = cpb; pa.info = h->a1_info.as<uint32_t>(); pa.progress = h->pipe_prog.as<uint64_t>();
    pa.cur_ptr = h->blk_off.as<uint64_t>(); pa.cur_len = h->blk_len.as<uint32_t>(); pa.skip = h->blk_skip.as<uint8_t>() + nblocks; pa.side = xb.side;
    pa.blk_status = h->blk_status.as<int32_t>(); pa.piped = h->pipe_flag.as<uint8_t>();
    pa.ranks_base = (uint64_t)h->xf_r3.p; pa.out_base = (uint64_t)h->xf_r2.p; pa.stride = xstride; pa.out_cap = xb.cap();
    pa.zrlt_stage = (uint32_t)(pnt - 1); pa.rank_stage = (uint32_t)(pnt - 2);
    pa.mode = 2;
    pa.group = pipe.groups ? h->pipe_group.as<uint8_t>() : (const uint8_t*)nullptr; pa.group_sel = 0;
    if (knz_test_switch("KNZ_RANK_UNPACKED") != nullptr) pa.mode |= 0x100;
    if (const char* cv = knz_test_switch("KNZ_RANK_CUT")) pa.mode |= ((uint32_t)atoi(cv) / 64u) << 12;
    hipEventRecord(h->ev_pipe[0], st);                                        // behind the table kernels: the chunk headers are parsed
    hipStreamWaitEvent(h->stream2, h->ev_pipe[0], 0);
    pipe.scope.launched = true;
    HIP_OK(hipMemsetAsync(h->xf_r3.p, 0, xstride * nblocks, h->stream2));     // zero runs are not written, only the literals between them
    if (pipe.groups) { hipEventRecord(h->ev_pipe[2], h->stream2); hipStreamWaitEvent(h->stream3, h->ev_pipe[2], 0); }   // (the other launch starts behind the zero fill too)
    pipe.args = pa;
    return KNZ_OK;
}

// Launch, BEHIND the producer's launch: the consumer never holds a CU the producer waits for
static void rank_pipe_launch(Handle* h, DecStage& d, hipStream_t st) {
    const RankPipe& pipe = d.pipe;
    const uint32_t nblocks = d.nblocks;
    hipStream_t st1 = st;
    if (pipe.groups) {                                                       // the long chains first (their waves start first), in their own stream
        RankPipeArgs pl = pipe.args;
        pl.group_sel = 1;
        { hipStream_t st = h->stream3; KNZ_LAUNCH_PROBED((knz_zrlti_rank_pipe_kernel<2, 4 | 64>), dim3(nblocks), dim3(128), 0, st, pl); }
        hipEventRecord(h->ev_pipe[2], h->stream3);
    }
    { hipStream_t st = h->stream2; KNZ_LAUNCH_PROBED((knz_zrlti_rank_pipe_kernel<2, 4 | 64>), dim3(nblocks), dim3(128), 0, st, pipe.args); }
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

static int fpaq_decode_stage(Handle* h, DecStage& d, hipStream_t st) {
    FpaqDecArgs da;
    dec_io(da, d.db, h, d.cpb);
    KNZ_LAUNCH_PROBED(knz_fpaq_decode_kernel, dim3(d.nblocks), dim3(64), 0, st, da);
    return KNZ_OK;
}

static int ans1_decode_stage(Handle* h, DecStage& d, hipStream_t st) {
    const uint32_t ns = d.nblocks * d.cpb;
    const bool wantTable = ns > KNZ_ANS1_LDS_MAX_CHUNKS || knz_test_switch("KNZ_ANS1_TABLE_DECODER") != nullptr;
    if ((wantTable && h->a1_dtab.reserve((size_t)ns * 256 * KNZ_ANS1_SCALE * 4)) || h->a1_info.reserve((size_t)ns * 32) || h->a1_paybit.reserve((size_t)ns * 8) ||
        h->a1_f16.reserve((size_t)ns * 65536 * 2))
        return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
    Ans1DecArgs da;
    dec_io(da, d.db, h, d.cpb); da.nslots = ns;
    da.dtab = h->a1_dtab.as<uint32_t>(); da.info = h->a1_info.as<uint32_t>(); da.paybit = h->a1_paybit.as<uint64_t>();
    da.plain_loop = knz_test_switch("KNZ_ANS1_PLAIN") != nullptr ? 1u : (knz_test_switch("KNZ_ANS1_LOHI_LDS") != nullptr ? 2u : (knz_test_switch("KNZ_ANS1_R5_LOOP") != nullptr ? 3u : 0u));
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
    int rc = rank_pipe_plan(h, d, ldsDecoder, st);
    if (rc) return rc;
    if (d.pipe.on) da.progress = h->pipe_prog.as<uint64_t>();
#ifdef KNZ_MEASURE
    if (ldsDecoder && knz_measure_switch("KNZ_ANS1_LDS1") != nullptr) KNZ_LAUNCH_PROBED(knz_ans1_decode_lds_kernel, dim3(ns), dim3(64), 0, st, da, (const uint16_t*)h->a1_cum.as<uint16_t>());   // (round-2 loop)
    else
#endif
    if (ldsDecoder) KNZ_LAUNCH_PROBED(knz_ans1_decode_lds2_kernel, dim3(ns), dim3(64), 0, st, da, (const uint16_t*)h->a1_cum.as<uint16_t>());
    else KNZ_LAUNCH_PROBED(knz_ans1_decode_kernel, dim3((ns + 15) / 16), dim3(64), 0, st, da);
    if (d.pipe.on) rank_pipe_launch(h, d, st);
    return KNZ_OK;
}

static int ans0_decode_stage(Handle* h, DecStage& d, hipStream_t st) {
    const uint32_t nblocks = d.nblocks, cpb = d.cpb;
    Ans0DecArgs da;
    dec_io(da, d.db, h, cpb);
    da.nslots = nblocks * cpb; da.out = nullptr;
    if (d.fusedWalk) {
        HIP_OK(hipMemsetAsync(h->chunk_rel.p, 0xFF, 8 * d.nslots, st));         // KNZ_CHUNK_NOT_READY
        const uint32_t gpb = (cpb + KNZ_ANS0_DEC_CHUNKS - 1) / KNZ_ANS0_DEC_CHUNKS;
        KNZ_LAUNCH_PROBED(knz_ans0_walk_decode_kernel, dim3(nblocks + nblocks * gpb), dim3(64), 0, st, d.wb, da);
    } else KNZ_LAUNCH_PROBED(knz_ans0_decode_kernel, dim3((nblocks * cpb + KNZ_ANS0_DEC_CHUNKS - 1) / KNZ_ANS0_DEC_CHUNKS), dim3(64), 0, st, da);
    return KNZ_OK;
}

static int huf_decode_stage(Handle* h, DecStage& d, hipStream_t st) {      // HUFFMAN, and NONE (raw chunks)
    const DecodeBatch& db = d.db;
    const uint32_t nblocks = d.nblocks, cpb = d.cpb;
    HufDecArgs da;
    dec_io(da, db, h, cpb);
    da.entropy = db.entropy; da.out = nullptr;
    if (db.entropy == KNZ_E_HUFFMAN) {
        if (h->huf_fallback.reserve((size_t)nblocks * cpb + 64)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
        h->huf_fallback_n = (size_t)nblocks * cpb;
        if (d.fusedWalk) {
            HIP_OK(hipMemsetAsync(h->chunk_rel.p, 0xFF, 8 * d.nslots, st));     // KNZ_CHUNK_NOT_READY
            KNZ_LAUNCH_PROBED(knz_huf_walk_decode_kernel, dim3(nblocks + nblocks * cpb), dim3(256), 0, st, d.wb, da, h->huf_fallback.as<uint8_t>());
        } else KNZ_LAUNCH_PROBED(knz_huf_decode_par_kernel, dim3(nblocks * cpb), dim3(256), 0, st, da, h->huf_fallback.as<uint8_t>());
        hipLaunchKernelGGL(knz_huf_decode_kernel, dim3(nblocks * cpb), dim3(64), 0, st, da, (const uint8_t*)h->huf_fallback.as<uint8_t>());
    } else {
        h->huf_fallback_n = 0;
        hipLaunchKernelGGL(knz_huf_decode_kernel, dim3(nblocks * cpb), dim3(64), 0, st, da, (const uint8_t*)nullptr);
    }
    return KNZ_OK;
}

// ---- the entropy codecs of this build: THE list of ids. knz_supports, encode_batch and decode_batch read it ----------------------------
struct EntropyCodec {
    uint32_t id, chunk, slot_stride, gather_y;       // bytes per chunk, bytes per scratch slot of a chunk, y-dimension of the gather grid
    uint32_t tab_slot;                               // bytes of Handle::ans_tab per slot (encode)
    int (*encode)(Handle*, EncStage&, hipStream_t);  // post-transform blocks -> units in the scratch slots (Huffman: or at their final bit positions)
    int (*decode)(Handle*, DecStage&, hipStream_t);  // chunks of the stream -> blocks at blk_off
};
static const EntropyCodec kEntropyCodecs[] = {
    {KNZ_E_NONE, KNZ_HUF_CHUNK, KNZ_CHUNK_STRIDE, 1, 0, huf_encode_stage, huf_decode_stage},
    {KNZ_E_HUFFMAN, KNZ_HUF_CHUNK, KNZ_CHUNK_STRIDE, 1, 0, huf_encode_stage, huf_decode_stage},
    {KNZ_E_FPAQ, KNZ_ANS1_CHUNK, KNZ_FPAQ_SLOT, 64, 0, fpaq_encode_stage, fpaq_decode_stage},
    {KNZ_E_ANS0, KNZ_HUF_CHUNK, KNZ_ANS_SLOT, 1, 2048 + 4, ans0_encode_stage, ans0_decode_stage},
    {KNZ_E_ANS1, KNZ_ANS1_CHUNK, KNZ_ANS1_SLOT, 64, 0, ans1_encode_stage, ans1_decode_stage},
};
static const EntropyCodec* entropy_codec(uint32_t e) {
    for (const EntropyCodec& c : kEntropyCodecs) if (c.id == e) return &c;
    return nullptr;
}
static bool entropy_on_device(uint32_t e) { return entropy_codec(e) != nullptr; }

// block tables of an encode batch: absolute device addresses; blocks <= 15 bytes are copy blocks (CompressedStream.go:773-776)
struct EncTablesArgs {
    uint32_t nblocks; uint64_t src; uint64_t n; uint64_t bs; int payload_only; int none_only;
    uint64_t* blk_off; uint32_t* blk_len; uint32_t* blk_src_len; uint8_t* blk_skip; uint8_t* blk_copy; int32_t* blk_status;
    uint8_t* active; uint8_t* side;
};
// row b of the tables: a block of len bytes at addr
__device__ __forceinline__ void knz_enc_table_row(const EncTablesArgs& a, uint32_t b, uint64_t addr, uint32_t len, bool payload_only) {
    const bool copy = len <= 15 && !payload_only;
    a.blk_off[b] = addr;
    a.blk_len[b] = len;
    a.blk_src_len[b] = payload_only ? (len > 16 ? len : 16u) : len;     // a bare EntropyEncoder has no copy-block rule
    a.blk_copy[b] = copy ? 1 : 0;
    a.blk_skip[b] = (copy || a.none_only) ? 0x7F : 0xFF;                // NullTransform always applies: slot 0 cleared
    a.blk_status[b] = 0;
    if (a.active) { a.active[b] = (copy || a.none_only) ? 0 : 1; a.side[b] = 0; }
}
__global__ void knz_enc_tables_kernel(EncTablesArgs a) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.nblocks) return;
    const uint64_t rest = a.n - (uint64_t)b * a.bs;
    knz_enc_table_row(a, b, a.src + (uint64_t)b * a.bs, (uint32_t)(rest < a.bs ? rest : a.bs), a.payload_only != 0);
}

// ... of a batch over several streams: block b is block b - first_block of the stream that owns it
__global__ void knz_many_enc_tables_kernel(EncTablesArgs a, const ManyStream* s, uint32_t K, uint32_t* blk_stream) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.nblocks) return;
    const uint32_t k = knz_many_owner(s, K, b);
    const uint64_t at = (uint64_t)(b - s[k].first_block) * a.bs, rest = s[k].n - at;
    blk_stream[b] = k;
    knz_enc_table_row(a, b, s[k].src + at, (uint32_t)(rest < a.bs ? rest : a.bs), false);
}

// the rows of Handle::ResultRow for the blocks of a batch, the totals (bits written, overflow flag) in the row behind the last block
__global__ void knz_pack_results_kernel(uint32_t nblocks, const uint64_t* written, const uint64_t* cksum, const uint32_t* post_len, const int32_t* status,
                                        const uint32_t* hdr, const uint8_t* skip, const uint64_t* totals, Handle::ResultRow* rows) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nblocks) {
        Handle::ResultRow r;
        r.written = written[b]; r.cksum = cksum[b]; r.post_len = post_len[b]; r.status = status[b]; r.mode = hdr[(size_t)b * 6 + 1]; r.skip = skip[b];
        rows[b] = r;
    } else if (b == nblocks) {
        Handle::ResultRow r;
        r.written = totals[0]; r.cksum = totals[1]; r.post_len = 0; r.status = 0; r.mode = 0; r.skip = 0;
        rows[b] = r;
    }
}

static int encode_batch(Handle* h, EncodeBatch& eb, hipStream_t st) {
    const knz_cfg& cfg = h->cfg;
    if (!eb.keep_probes) h->nprobes = 0;
    if (!knz_supports(cfg.transform, cfg.entropy))
        return knz_set_error(h, KNZ_ERR_INVALID_CODEC, "transform/entropy combination has no device implementation in this build");
    const EntropyCodec& ec = *entropy_codec(cfg.entropy);
    const uint64_t bs = cfg.block_size;
    const uint32_t nblocks = eb.many.streams ? eb.many.blocks : (uint32_t)((eb.n + bs - 1) / bs);       // (0: Writer.Close on an empty stream, header + end marker only)
    const uint32_t chunkSize = ec.chunk;
    const uint32_t maxPost = knz_max_encoded_len(cfg.transform, eb.many.streams ? std::max<uint32_t>(eb.many.max_len, 1) : (uint32_t)std::min<uint64_t>(bs, eb.n ? eb.n : 1));
    const uint32_t cpb = std::max<uint32_t>(1, (maxPost + chunkSize - 1) / chunkSize);
    const size_t nslots = (size_t)std::max<uint32_t>(nblocks, 1) * cpb;
    const uint32_t slotStride = ec.slot_stride;

    if (h->blk_off.reserve(sizeof(uint64_t) * (nblocks + 1)) || h->blk_len.reserve(4 * (nblocks + 1)) ||
        h->blk_src_len.reserve(4 * (nblocks + 1)) || h->blk_skip.reserve(nblocks + 16) || h->blk_cksum.reserve(8 * (nblocks + 1)) ||
        h->blk_status.reserve(4 * (nblocks + 1)) || h->unit_bits.reserve(4 * nslots * KNZ_UNITS_PER_CHUNK) || h->unit_src.reserve(4 * nslots * KNZ_UNITS_PER_CHUNK) ||
        h->scratch.reserve(nslots * (size_t)slotStride + 64) || h->ans_tab.reserve(std::max<size_t>(nslots * ec.tab_slot, 16)) || h->chunk_rel.reserve(8 * nslots) ||
        h->blk_written.reserve(8 * (nblocks + 1)) || h->blk_hdr.reserve(4 * 6 * (nblocks + 1)) ||
        h->blk_dst_bit.reserve(8 * (nblocks + 1)) || h->total_bits.reserve(64) || h->blk_copy.reserve(nblocks + 16))
        return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");

    XfBatch xb;
    if (nblocks) {   // block tables, filled on the device: no staging copies, no host synchronisation in front of the first kernel
        const bool noneOnly = cfg.transform == 0;
        const uint64_t stride = ((uint64_t)maxPost + 64 + 15) & ~(uint64_t)15;
        if (!noneOnly && xf_alloc(h, xb, nblocks, stride)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
        EncTablesArgs ta;
        ta.nblocks = nblocks; ta.src = (uint64_t)eb.d_src; ta.n = eb.n; ta.bs = bs; ta.payload_only = eb.payload_only; ta.none_only = noneOnly ? 1 : 0;
        ta.blk_off = h->blk_off.as<uint64_t>(); ta.blk_len = h->blk_len.as<uint32_t>(); ta.blk_src_len = h->blk_src_len.as<uint32_t>();
        ta.blk_skip = h->blk_skip.as<uint8_t>(); ta.blk_copy = h->blk_copy.as<uint8_t>(); ta.blk_status = h->blk_status.as<int32_t>();
        ta.active = noneOnly ? nullptr : xb.active; ta.side = noneOnly ? nullptr : xb.side;
        if (eb.many.streams) hipLaunchKernelGGL(knz_many_enc_tables_kernel, dim3((nblocks + 255) / 256), dim3(256), 0, st, ta, eb.many.streams, eb.many.n_streams, eb.many.blk_stream);
        else hipLaunchKernelGGL(knz_enc_tables_kernel, dim3((nblocks + 255) / 256), dim3(256), 0, st, ta);
    }
    const bool skipOpt = (cfg.flags & KNZ_FLAG_SKIP_BLOCKS) != 0 && !eb.payload_only && nblocks != 0;
    if (skipOpt) {                                                       // -s: incompressible blocks become copy blocks (:778-800)
        SkipArgs ka;
        ka.nblocks = nblocks; ka.blk_off = h->blk_off.as<uint64_t>(); ka.blk_len = h->blk_len.as<uint32_t>();
        ka.blk_copy = h->blk_copy.as<uint8_t>(); ka.blk_skip = h->blk_skip.as<uint8_t>(); ka.active = cfg.transform != 0 ? xb.active : nullptr;
        hipLaunchKernelGGL(knz_skip_detect_kernel, dim3(nblocks), dim3(256), 0, st, ka);
    }
    hipEventRecord(h->ev[0], st);
    if (nblocks && cfg.checksum_bits != 0) {        // checksum of the untransformed block (encodingTask.encode :760-767)
        XxhArgs xa;
        xa.nblocks = nblocks; xa.ptr = h->blk_off.as<uint64_t>(); xa.len = h->blk_len.as<uint32_t>(); xa.cksum = h->blk_cksum.as<uint64_t>();
        xa.status = h->blk_status.as<int32_t>(); xa.mode = nullptr; xa.bits = cfg.checksum_bits; xa.verify = 0;
        hipLaunchKernelGGL(knz_xxhash_kernel, dim3(nblocks), dim3(64), 0, st, xa);
    }
    if (nblocks && cfg.transform != 0) {
        xb.cur_ptr = h->blk_off.as<uint64_t>(); xb.cur_len = h->blk_len.as<uint32_t>(); xb.skip = h->blk_skip.as<uint8_t>();
        xb.blk_status = h->blk_status.as<int32_t>();
        bool hasUtf = false;                                             // (a stage that reads or writes ctx["dataType"])
        for (int sft = 42; sft >= 0; sft -= 6) hasUtf = hasUtf || xf_codec((uint32_t)((cfg.transform >> sft) & 63))->data_type;
        if (hasUtf) {                                                    // ctx["dataType"] from the magic number of the untransformed block (:811-819)
            if (h->blk_dt.reserve(nblocks + 16)) return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "device workspace allocation failed");
            hipLaunchKernelGGL(knz_block_datatype_kernel, dim3((nblocks + 63) / 64), dim3(64), 0, st, nblocks, (const uint64_t*)h->blk_off.as<uint64_t>(),
                               (const uint32_t*)h->blk_len.as<uint32_t>(), h->blk_dt.as<uint8_t>());
            xb.blk_dt = h->blk_dt.as<uint8_t>();
        }
        int rc = forward_sequence(h, xb, cfg.transform, st);
        if (rc) return rc;
    }
    hipEventRecord(h->ev[1], st);
    EncStage es{nblocks, cpb, slotStride, nslots, skipOpt};
    if (nblocks) { int rc = ec.encode(h, es, st); if (rc) return rc; }
    hipEventRecord(h->ev[2], st);
    if (skipOpt && cfg.entropy != KNZ_E_NONE) {
        CopyUnitsArgs ca;
        enc_io(ca, h, cpb); ca.chunk_size = chunkSize; ca.blk_copy = h->blk_copy.as<uint8_t>(); ca.slot_stride = slotStride;
        hipLaunchKernelGGL(knz_copy_units_kernel, dim3(nblocks * cpb), dim3(256), 0, st, ca);
    }
    LayoutArgs la;
    uint32_t toks[8];
    la.nblocks = nblocks; la.chunks_per_block = cpb; la.unit_bits = h->unit_bits.as<uint32_t>();
    la.blk_len = h->blk_len.as<uint32_t>(); la.blk_src_len = h->blk_src_len.as<uint32_t>(); la.blk_skip = h->blk_skip.as<uint8_t>(); la.blk_copy = h->blk_copy.as<uint8_t>();
    la.blk_cksum = h->blk_cksum.as<uint64_t>(); la.checksum_bits = cfg.checksum_bits; la.n_transforms = (uint32_t)seq_tokens(cfg.transform, toks);
    la.chunk_size = chunkSize; la.payload_only = eb.payload_only; la.chunk_rel = h->chunk_rel.as<uint64_t>(); la.blk_written = h->blk_written.as<uint64_t>();
    la.blk_hdr = h->blk_hdr.as<uint32_t>();
    if (nblocks) hipLaunchKernelGGL(knz_layout_blocks_kernel, dim3(nblocks), dim3(256), 0, st, la);

    StreamArgs sa;
    sa.nblocks = nblocks; sa.chunks_per_block = cpb; sa.chunk_size = chunkSize; sa.blk_len = h->blk_len.as<uint32_t>();
    sa.chunk_rel = h->chunk_rel.as<uint64_t>(); sa.blk_written = h->blk_written.as<uint64_t>(); sa.blk_hdr = h->blk_hdr.as<uint32_t>();
    sa.dst_words = (uint32_t*)eb.d_dst;
    const uint64_t usable = eb.dst_cap >= 8 ? ((eb.dst_cap & ~(uint64_t)3) - 4) : 0;   // whole BE words are stored
    sa.dst_cap_bits = usable * 8;
    sa.first_bit = 0; sa.framed = eb.framed; sa.block_stride_bits = eb.out_stride * 8; sa.end_marker = eb.with_end;
    sa.header_bits = 0;
    for (int i = 0; i < 8; i++) sa.header_words[i] = 0;
    if (eb.framed && eb.with_header) sa.header_bits = knz_build_stream_header(cfg, eb.header_input_size, sa.header_words);
    sa.blk_dst_bit = h->blk_dst_bit.as<uint64_t>(); sa.total_bits = h->total_bits.as<uint64_t>();
    sa.blk_status = h->blk_status.as<int32_t>();
    hipLaunchKernelGGL(knz_layout_stream_kernel, dim3(1), dim3(256), 0, st, sa);
    hipEventRecord(h->ev[3], st);
    if (es.hufDirect && nblocks) {                                       // Huffman: the encoder itself places the units (no scratch round trip, no gather)
        HufEncArgs& a = es.hufArgs;
        a.dst_words = (uint32_t*)eb.d_dst; a.chunk_rel = h->chunk_rel.as<uint64_t>(); a.blk_dst_bit = h->blk_dst_bit.as<uint64_t>();
        a.total_bits = h->total_bits.as<uint64_t>();
        KNZ_LAUNCH_PROBED(knz_huf_encode_kernel<false>, dim3(nblocks * cpb), dim3(256), 0, st, a);
    }

    GatherArgs ga;
    ga.chunks_per_block = cpb; ga.chunk_size = chunkSize; ga.blk_len = h->blk_len.as<uint32_t>(); ga.unit_bits = h->unit_bits.as<uint32_t>();
    ga.scratch = h->scratch.as<uint8_t>(); ga.chunk_stride = slotStride;
    ga.unit_src = h->unit_src.as<uint32_t>();
    ga.chunk_rel = h->chunk_rel.as<uint64_t>(); ga.blk_dst_bit = h->blk_dst_bit.as<uint64_t>(); ga.dst_words = (uint32_t*)eb.d_dst;
    ga.total_bits = h->total_bits.as<uint64_t>();
    if (nblocks && !es.hufDirect) KNZ_LAUNCH_PROBED(knz_gather_kernel, dim3(nblocks * cpb, ec.gather_y), dim3(256), 0, st, ga);
    hipEventRecord(h->ev[4], st);
    h->ev_valid = true;

    // results come back packed: one row per block (bit count, checksum, post-transform length, status, mode, skip flags) and the batch totals, gathered
    // by one small kernel and brought over by ONE asynchronous copy into pinned memory, one synchronisation
    if (h->res_rows.reserve(sizeof(Handle::ResultRow) * ((size_t)nblocks + 1)) || h->pinned_rows.reserve(sizeof(Handle::ResultRow) * ((size_t)nblocks + 1)))
        return knz_set_error(h, KNZ_ERR_CREATE_COMPRESSOR, "pinned host allocation failed");
    hipLaunchKernelGGL(knz_pack_results_kernel, dim3((nblocks + 1 + 255) / 256), dim3(256), 0, st, nblocks, (const uint64_t*)h->blk_written.as<uint64_t>(),
                       (const uint64_t*)h->blk_cksum.as<uint64_t>(), (const uint32_t*)h->blk_len.as<uint32_t>(), (const int32_t*)h->blk_status.as<int32_t>(),
                       (const uint32_t*)h->blk_hdr.as<uint32_t>(), (const uint8_t*)h->blk_skip.as<uint8_t>(), (const uint64_t*)h->total_bits.as<uint64_t>(),
                       h->res_rows.as<Handle::ResultRow>());
    Handle::ResultRow* rows = h->pinned_rows.as<Handle::ResultRow>();
    HIP_OK(hipMemcpyAsync(rows, h->res_rows.p, sizeof(Handle::ResultRow) * ((size_t)nblocks + 1), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    if (rows[nblocks].cksum != 0) return knz_set_error(h, KNZ_ERR_WRITE_FILE, "destination buffer too small");     // (the totals row: bits, overflow flag)
    for (uint32_t b = 0; b < nblocks && !eb.many.streams; b++)
        if (rows[b].status != 0) return knz_set_error(h, rows[b].status, "block failed (the reference panics on this input: ERR_PROCESS_BLOCK)");
    eb.total_bits = rows[nblocks].written;
    h->post_bytes = 0;
    for (uint32_t b = 0; b < nblocks; b++) h->post_bytes += rows[b].post_len;
    for (int i = 0; i < 8; i++) h->stage_bytes[i] = (nblocks && cfg.transform != 0) ? ((const uint64_t*)((const uint8_t*)h->pinned + 3072))[i] : 0;
    return KNZ_OK;
}

// ---- decode batch: framing walk, header pass, output placement and pre-checks, entropy stage, inverse transforms and copy-out, checksum, results ----
// Framing walk: the number of blocks and their bit positions (framed: found on the device ; else given, blk_bit / blk_bits uploaded by the caller)
static int dec_walk_framing(Handle* h, DecodeBatch& db, hipStream_t st) {
    uint32_t maxBlocks = db.nblocks;
    if (db.framed) {
        // every block costs at least 8 framing bits + 16 payload bits
        uint64_t bound = db.nbytes / 3 + 1;
        maxBlocks = (uint32_t)std::min<uint64_t>(bound, 1u << 24);
    }
    const uint32_t walkBound = maxBlocks;
    if (db.framed && db.ranged) maxBlocks = (uint32_t)std::min<uint64_t>(maxBlocks, db.rg_to - db.rg_from);   // (the tables hold the range, not the stream)
    DevBuf& blkBit = h->blk_dst_bit;      // reuse of the encode-side tables: [maxBlocks] u64 each
    DevBuf& blkBits = h->blk_written;
    if (blkBit.reserve(8 * ((size_t)maxBlocks + 1)) || blkBits.reserve(8 * ((size_t)maxBlocks + 1)) || h->total_bits.reserve(64))
        return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
    uint32_t nblocks = db.nblocks;
    if (db.framed && db.ranged) {
        WalkRangeArgs wr;
        wr.stream = db.d_stream; wr.nbytes = db.nbytes; wr.first_bit = db.first_bit; wr.first_id = db.rg_first_id; wr.from = db.rg_from; wr.to = db.rg_to;
        wr.max_blocks = walkBound; wr.cap = maxBlocks; wr.frames = 0; wr.stride = 1; wr.hinted = db.rg_hinted ? 1 : 0;
        wr.blk_bit = blkBit.as<uint64_t>(); wr.blk_bits = blkBits.as<uint64_t>(); wr.result = h->total_bits.as<uint64_t>();
        hipLaunchKernelGGL(knz_dec_walk_range_kernel, dim3(1), dim3(1), 0, st, wr);
        uint64_t* res = (uint64_t*)h->pinned;
        HIP_OK(hipMemcpyAsync(res, h->total_bits.p, 24, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (res[1]) return knz_set_error(h, (int)res[1], "invalid block framing in stream");
        nblocks = (uint32_t)res[0];
    } else if (db.framed) {
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
    return KNZ_OK;
}

// Header pass: every block's header fields and (unless the decoders' launch walks them) its chunks' bit positions
static int dec_header_pass(Handle* h, DecStage& d, const EntropyCodec& ec, hipStream_t st) {
    const DecodeBatch& db = d.db;
    const uint32_t nblocks = d.nblocks = db.nblocks;
    WalkBlocksArgs& wb = d.wb;
    const uint32_t maxPre = db.payload_only ? db.given_len : knz_max_encoded_len(db.transform, db.block_size);
    const uint32_t cpb = d.cpb = std::max<uint32_t>(1, (maxPre + ec.chunk - 1) / ec.chunk);
    const size_t nslots = d.nslots = (size_t)nblocks * cpb;
    if (h->blk_len.reserve(4 * (size_t)nblocks) || h->blk_skip.reserve(2 * (size_t)nblocks + 16) || h->blk_cksum.reserve(8 * (size_t)nblocks) ||
        h->chunk_rel.reserve(8 * nslots) || h->blk_status.reserve(4 * (size_t)nblocks) || h->blk_off.reserve(8 * (size_t)nblocks) ||
        h->dec_tables.reserve(8 * (size_t)nblocks))
        return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
    hipEventRecord(h->ev[0], st);
    wb.stream = db.d_stream; wb.nbytes = db.nbytes; wb.blk_bit = h->blk_dst_bit.as<uint64_t>(); wb.blk_bits = h->blk_written.as<uint64_t>();
    wb.nblocks = nblocks;
    // blockLength handed to decodingTask is padded (v2/io/CompressedStream.go:1620-1626)
    wb.block_size = db.block_size + std::max<uint32_t>(512, db.block_size >> 4);
    wb.checksum_bits = db.checksum_bits; wb.entropy = db.entropy; wb.chunks_per_block = cpb;
    wb.payload_only = db.payload_only; wb.given_len = db.given_len;
    wb.blk_pre_len = h->blk_len.as<uint32_t>(); wb.blk_mode = h->blk_skip.as<uint8_t>(); wb.blk_skip = h->blk_skip.as<uint8_t>() + nblocks;
    wb.blk_cksum = h->blk_cksum.as<uint64_t>(); wb.chunk_bit = h->chunk_rel.as<uint64_t>(); wb.blk_status = h->blk_status.as<int32_t>();
    wb.blk_end_bit = h->dec_tables.as<uint64_t>();
    // Huffman: only the block headers now, the chunk walk shares a launch with the chunk decoders (below)
    const bool fusedWalk = d.fusedWalk = (db.entropy == KNZ_E_HUFFMAN || db.entropy == KNZ_E_ANS0) && knz_test_switch("KNZ_HUF_SPLIT_WALK") == nullptr;   // (the variable lets the tests reach the two-launch path)
    // no transform stage behind the decode: the header pass also places the blocks and makes the host's checks, so nothing is
    // copied or synchronised between it and the walk+decode launch (a refused block shows up in its status at the end)
    d.xf = db.transform != 0 && !db.payload_only;
    const bool direct = d.direct = fusedWalk && !d.xf;
    wb.check_out = direct ? 1 : 0; wb.out_off = h->blk_off.as<uint64_t>(); wb.out_base = (uint64_t)db.d_out; wb.out_stride = db.out_stride;
    wb.out_cap = db.out_cap; wb.stream_block_size = db.block_size;
    wb.ans1_ctx_bit = nullptr;
    wb.ans1_walk_plain = knz_test_switch("KNZ_ANS1_WALK_PLAIN") != nullptr ? 1u : 0u;   // (A/B and cross-check: the generic reader's walk of the chunk headers)
    if (db.entropy == KNZ_E_ANS1) {                                           // the walk leaves every context header's position for the table kernel
        if (h->a1_ctxpos.reserve((size_t)nslots * 257 * 8 + 64)) return knz_set_error(h, KNZ_ERR_CREATE_DECOMPRESSOR, "device workspace allocation failed");
        wb.ans1_ctx_bit = h->a1_ctxpos.as<uint64_t>();
    }
    if (fusedWalk) hipLaunchKernelGGL(knz_dec_block_headers_kernel, dim3(nblocks), dim3(64), 0, st, wb);
    else hipLaunchKernelGGL(knz_dec_walk_blocks_kernel, dim3(nblocks), dim3(128), 0, st, wb);
    hipEventRecord(h->ev[1], st);
    return KNZ_OK;
}

// Reader.processBlock :1707-1710: block b, decoded to pre_len[b] bytes, fits the stream's block size and the caller's buffer
static int dec_block_fits(Handle* h, const DecodeBatch& db, uint32_t b) {
    if (db.pre_len[b] > db.block_size || (db.pre_len[b] > db.out_stride && b + 1 < db.nblocks))
        return knz_set_error(h, KNZ_ERR_PROCESS_BLOCK, "block decodes to more than the stream block size");
    if ((uint64_t)b * db.out_stride + db.pre_len[b] > db.out_cap) return knz_set_error(h, KNZ_ERR_WRITE_FILE, "destination buffer too small");
    return KNZ_OK;
}

// Output placement and pre-checks (not where the header pass has done both): transform NONE decodes straight to block b at b*out_stride; otherwise into
// region 1 of the transform pipeline, the inverse sequence follows
static int dec_place_outputs(Handle* h, DecStage& d, hipStream_t st) {
    DecodeBatch& db = d.db;
    XfBatch& xb = d.xb;
    const uint32_t nblocks = d.nblocks;
    const bool xf = d.xf;
    uint64_t& xstride = d.xstride;
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
    int first = KNZ_OK;
    for (uint32_t b = 0; b < nblocks; b++) {
        int rc = KNZ_OK;
        if (db.status[b]) rc = knz_set_error(h, db.status[b], "invalid block in stream");
        else if (xf) { if (db.pre_len[b] > xstride) rc = knz_set_error(h, KNZ_ERR_BLOCK_SIZE, "block larger than the decoder buffers"); }
        else rc = dec_block_fits(h, db, b);
        if (rc && db.block_failed(b, rc, first)) return rc;
    }
    return first;
}

// Inverse transforms and copy-out: the stages the fused chain has not done, in one pass or (the chain in two launches) two; then the blocks to where the
// caller wants them
static int dec_inverse_transforms(Handle* h, DecStage& d, hipStream_t st) {
    DecodeBatch& db = d.db;
    XfBatch& xb = d.xb;
    const RankPipe& pipe = d.pipe;
    const uint32_t nblocks = d.nblocks;
    if (!pipe.on) {
        std::vector<uint8_t> ones(nblocks, 1);
        HIP_OK(hipMemcpyAsync(xb.side, ones.data(), nblocks, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(xb.take, ones.data(), nblocks, hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));
    } else {
        xb.piped = h->pipe_flag.as<uint8_t>(); xb.piped_zrlt = (int)pipe.args.zrlt_stage; xb.piped_rank = (int)pipe.args.rank_stage;
    }
    xb.cur_ptr = h->blk_off.as<uint64_t>(); xb.cur_len = h->blk_len.as<uint32_t>(); xb.skip = h->blk_skip.as<uint8_t>() + nblocks;
    xb.blk_status = h->blk_status.as<int32_t>();
    int rc;
    if (pipe.groups) {
        uint8_t* takeAll = xb.take;
        xb.take = pipe.take[0];                                                   // pass A: the blocks of the short chains, while the long ones run
        rc = inverse_sequence(h, xb, db.transform, st);
        if (rc) return rc;
        hipStreamWaitEvent(st, h->ev_pipe[2], 0);
        xb.take = pipe.take[1];                                                   // pass B: the blocks of the long chains
        rc = inverse_sequence(h, xb, db.transform, st);
        xb.take = takeAll;
    } else rc = inverse_sequence(h, xb, db.transform, st);
    if (rc) return rc;
    HIP_OK(hipMemcpyAsync(db.pre_len.data(), h->blk_len.p, 4 * (size_t)nblocks, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(db.status.data(), h->blk_status.p, 4 * (size_t)nblocks, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    std::vector<uint64_t> dstp(nblocks);
    int first = KNZ_OK;
    for (uint32_t b = 0; b < nblocks; b++) {
        rc = db.status[b] ? knz_set_error(h, db.status[b], "inverse transform failed") : dec_block_fits(h, db, b);
        dstp[b] = (uint64_t)db.d_out + (uint64_t)b * db.out_stride;
        if (rc && db.block_failed(b, rc, first)) return rc;
    }
    if (first) return first;
    HIP_OK(hipMemcpyAsync(xb.out_ptr, dstp.data(), 8 * (size_t)nblocks, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
    hipLaunchKernelGGL(knz_copy_blocks_kernel, dim3(64, nblocks), dim3(256), 0, st, nblocks, xb.cur_ptr, xb.cur_len, xb.out_ptr, (const uint8_t*)nullptr);
    return KNZ_OK;
}

// Checksum (decodingTask.decode :1992-2007): hash of the decoded block vs the header field
static void dec_checksum(Handle* h, DecStage& d, hipStream_t st) {
    const DecodeBatch& db = d.db;
    const uint32_t nblocks = d.nblocks;
    XxhArgs xa;
    xa.nblocks = nblocks; xa.len = h->blk_len.as<uint32_t>(); xa.cksum = h->blk_cksum.as<uint64_t>(); xa.status = h->blk_status.as<int32_t>();
    xa.ptr = d.xf ? d.xb.out_ptr : h->blk_off.as<uint64_t>();
    xa.mode = nullptr; xa.bits = db.checksum_bits; xa.verify = 1;
    hipLaunchKernelGGL(knz_xxhash_kernel, dim3(nblocks), dim3(64), 0, st, xa);
}

// Results: status and end position of every block, its length where the host has not read it yet
static int dec_results(Handle* h, DecStage& d, hipStream_t st) {
    DecodeBatch& db = d.db;
    const uint32_t nblocks = d.nblocks;
    HIP_OK(hipMemcpyAsync(db.status.data(), h->blk_status.p, 4 * (size_t)nblocks, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(db.end_bit.data(), h->dec_tables.p, 8 * (size_t)nblocks, hipMemcpyDeviceToHost, st));
    if (d.direct) HIP_OK(hipMemcpyAsync(db.pre_len.data(), h->blk_len.p, 4 * (size_t)nblocks, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    db.done = true;
    int first = KNZ_OK;
    for (uint32_t b = 0; b < nblocks; b++) {
        if (db.status[b]) {
            const int rc = knz_set_error(h, db.status[b], db.status[b] == KNZ_ERR_CRC_CHECK ? "Corrupted bitstream: checksum mismatch" : "invalid entropy payload");
            if (db.block_failed(b, rc, first)) return rc;
        } else db.total_out += db.pre_len[b];
    }
    return first;
}

static int decode_batch(Handle* h, DecodeBatch& db, hipStream_t st) {
    h->nprobes = 0;
    if (!knz_supports(db.transform, db.entropy))
        return knz_set_error(h, KNZ_ERR_INVALID_CODEC, "transform/entropy combination has no device implementation in this build");
    const EntropyCodec& ec = *entropy_codec(db.entropy);
    h->dec_blocks = 0;
    int rc = dec_walk_framing(h, db, st);
    if (rc || db.nblocks == 0) return rc;
    h->dec_blocks = db.nblocks;
    DecStage d(h, db);
    if ((rc = dec_header_pass(h, d, ec, st)) != KNZ_OK) return rc;
    h->pipe_n = 0;
    if (!d.direct && (rc = dec_place_outputs(h, d, st)) != KNZ_OK) return rc;
    if ((rc = ec.decode(h, d, st)) != KNZ_OK) return rc;
    hipEventRecord(h->ev[2], st);
    if (d.xf && (rc = dec_inverse_transforms(h, d, st)) != KNZ_OK) return rc;
    if (db.checksum_bits != 0 && !db.payload_only) dec_checksum(h, d, st);
    hipEventRecord(h->ev[3], st);
    hipEventRecord(h->ev[4], st);
    h->ev_valid = true;
    return dec_results(h, d, st);
}
