// Several independent .knz streams in ONE device batch (knz_dev_compress_many / knz_dev_decompress_many, host side in knz_many.inc).
// The batch itself runs in its unframed form (per-block local streams at a fixed stride, the path of knz_encode_blocks / knz_decode_blocks)
// over a block table that the kernels below derive from the table of streams; nothing here grows with the number of streams but the grids.
//   encode: knz_many_scan_kernel (first block of every stream) -> knz_many_enc_tables_kernel (knz_batch.inc: the batch's block table) -> batch ->
//           knz_many_asm_plan_kernel (per stream: scan of the blocks' exact bit counts, capacity check, header, framing fields
//           (lw-3):5 written:lw of CompressedStream.go:951-976, end marker :593-594) -> knz_many_asm_copy_kernel (every block's bit string
//           funnel-shifted to its final bit offset, one thread per destination word)
//   decode: knz_many_heads_kernel (the first 32 bytes of every stream, for the host's header parse) -> knz_many_stage_kernel (the streams side
//           by side in one buffer, zero padded: every read of the decoders is bounded by that buffer) -> knz_many_walk_kernel (count) ->
//           knz_many_scan_kernel -> knz_many_walk_kernel (fill) -> batch -> knz_many_place_plan_kernel (per stream: scan of the decoded
//           lengths, block size and capacity checks) -> knz_many_place_copy_kernel
// Streams never share a destination word (d_dst is 4-byte aligned per stream); blocks of one stream do: interior words are stored,
// boundary words OR-ed into words the plan kernel zeroed (the rule of knz_concat_segment_kernel).
#include "bits.h"

struct ManyStream {                  // one row per stream: the host fills the inputs, the kernels the rest
    uint64_t src, n, dst, cap;       // device addresses and byte counts of the caller's knz_stream
    uint32_t hdr_words[8];           // compress: the stream header, BE words
    uint32_t hdr_bits;               // compress: its bit count ; decompress: bit position of the first block's framing
    uint32_t first_block, nblocks;   // the stream's rows of the batch's block table
    int32_t status;                  // 0 or a kanzi error code (a stream that fails contributes no blocks / gets nothing written)
    uint64_t out;                    // result: bytes written
    uint64_t stage_off;              // decompress: byte offset of the stream's copy in the staging buffer (16-byte aligned)
};

// first_block[k] = exclusive scan of the streams' block counts (from_len: ceil(n / bs), else what the walk counted); total[0] = their sum
__global__ __launch_bounds__(256) void knz_many_scan_kernel(ManyStream* s, uint32_t K, uint64_t bs, uint32_t from_len, uint32_t* total) {
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t k0 = 0; k0 < K; k0 += 256) {
        const uint32_t k = k0 + tid;
        uint32_t nb = 0;
        if (k < K && s[k].status == 0) nb = from_len ? (uint32_t)((s[k].n + bs - 1) / bs) : s[k].nblocks;
        const uint32_t incl = wave_scan_incl(nb);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = s_carry;
        for (int w = 0; w < wave; w++) before += s_wave[w];
        if (k < K) { s[k].first_block = before + incl - nb; s[k].nblocks = nb; }
        __syncthreads();
        if (tid == 255) s_carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) total[0] = s_carry;
}

// the stream that owns block b: the last one whose first block is <= b (streams without blocks share their successor's first block)
__device__ __forceinline__ uint32_t knz_many_owner(const ManyStream* s, uint32_t K, uint32_t b) {
    uint32_t lo = 0, hi = K;                       // invariant: first_block[lo] <= b, first_block[hi] > b (hi == K: the end)
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (s[mid].first_block <= b) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t knz_many_lw(uint64_t written) {             // bits of the `written` field (:951-956)
    return written >= 8 ? (31u - (uint32_t)__builtin_clz((uint32_t)(written >> 3))) + 4 : 3;
}

struct ManyAsmArgs {
    ManyStream* streams; uint32_t K;
    const uint64_t* blk_written;     // [nblocks] bits of every block-local stream (the batch's layout pass)
    const int32_t* blk_status;       // [nblocks]
    const uint32_t* blk_stream;      // [nblocks] owning stream
    uint64_t* blk_pos;               // [nblocks] out: bit position of the block's bits in its stream
    const uint8_t* stage; uint64_t stride;   // block b's local stream at stage + b * stride
};

// One workgroup per stream. Nothing of a stream is written before its size is known to fit (the rule of knz_layout_stream_kernel: whole BE
// words are stored, the last of them inside dst_cap).
__global__ __launch_bounds__(256) void knz_many_asm_plan_kernel(ManyAsmArgs a) {
    __shared__ uint64_t s_wsum[4];
    __shared__ uint64_t s_carry;
    __shared__ uint32_t s_bad;                       // the first block of the stream that failed
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    ManyStream& s = a.streams[blockIdx.x];
    if (s.status != 0) return;                                            // (refused by the host: nothing of it is in the batch)
    const uint32_t b0 = s.first_block, nb = s.nblocks;
    if (tid == 0) { s_carry = s.hdr_bits; s_bad = 0xFFFFFFFFu; }
    __syncthreads();
    for (uint32_t i0 = 0; i0 < nb; i0 += 256) {
        const uint32_t i = i0 + tid;
        uint64_t written = 0, sz = 0;
        if (i < nb) {
            written = a.blk_written[b0 + i];
            sz = 5 + knz_many_lw(written) + written;
            if (a.blk_status[b0 + i] != 0) atomicMin(&s_bad, i);
        }
        uint64_t incl = sz;
        for (int d = 1; d < 64; d <<= 1) { const uint64_t t = wave_shfl64(incl, lane - d); if (lane >= d) incl += t; }
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        uint64_t before = s_carry;
        for (int w = 0; w < wave; w++) before += s_wsum[w];
        if (i < nb) a.blk_pos[b0 + i] = before + incl - written;
        __syncthreads();
        if (tid == 255) s_carry = before + incl;
        __syncthreads();
    }
    const uint64_t endpos = s_carry, total = endpos + 8;                  // the end marker: (3-3):5, 0:3
    const uint64_t usable = s.cap >= 8 ? ((s.cap & ~(uint64_t)3) - 4) : 0;
    int32_t status = s_bad != 0xFFFFFFFFu ? a.blk_status[b0 + s_bad] : 0;
    if (status == 0 && total > usable * 8) status = KNZ_ERR_WRITE_FILE;
    __syncthreads();
    if (tid == 0) { s.status = status; s.out = status ? 0 : (total + 7) >> 3; }
    if (status != 0) return;
    uint32_t* dst = (uint32_t*)s.dst;
    const uint64_t nwords = (((total + 7) >> 3) + 3) >> 2;
    // pass 1: zero every word that is OR-ed into: header, every block's framing field up to its first word, its last word, the end
    for (uint64_t w = tid; w <= ((uint64_t)s.hdr_bits - 1) >> 5; w += 256) dst[w] = 0;
    for (uint64_t w = (endpos >> 5) + tid; w < nwords; w += 256) dst[w] = 0;
    for (uint32_t i = tid; i < nb; i += 256) {
        const uint64_t written = a.blk_written[b0 + i], base = a.blk_pos[b0 + i];
        for (uint64_t w = (base - 5 - knz_many_lw(written)) >> 5; w <= base >> 5; w++) dst[w] = 0;
        if (written) dst[(base + written - 1) >> 5] = 0;
    }
    __threadfence();
    __syncthreads();
    // pass 2: OR the header and the framing fields (the end marker is eight zero bits)
    for (uint32_t i = tid; i * 32 < s.hdr_bits; i += 256) {
        const uint32_t cnt = min(32u, s.hdr_bits - i * 32);
        knz_or_bits(dst, (uint64_t)i * 32, s.hdr_words[i] >> (32 - cnt), cnt);
    }
    for (uint32_t i = tid; i < nb; i += 256) {
        const uint64_t written = a.blk_written[b0 + i], base = a.blk_pos[b0 + i];
        const uint32_t lw = knz_many_lw(written);
        const uint64_t p = base - lw - 5;
        knz_or_bits(dst, p, lw - 3, 5);
        if (lw > 32) { knz_or_bits(dst, p + 5, (uint32_t)(written >> 32), lw - 32); knz_or_bits(dst, p + 5 + (lw - 32), (uint32_t)written, 32); }
        else knz_or_bits(dst, p + 5, (uint32_t)written, lw);
    }
}

// grid (nblocks, y): block b's bit string to its place; a thread owns destination words (knz_concat_segment_kernel, per block of a table)
__global__ __launch_bounds__(256) void knz_many_asm_copy_kernel(ManyAsmArgs a) {
    const uint32_t b = blockIdx.x;
    const ManyStream& s = a.streams[a.blk_stream[b]];
    if (s.status != 0) return;
    const uint64_t nbits = a.blk_written[b], dbit = a.blk_pos[b];
    if (nbits == 0) return;
    const uint8_t* src = a.stage + (uint64_t)b * a.stride;
    uint32_t* dst = (uint32_t*)s.dst;
    const uint64_t w0 = dbit >> 5, w1 = (dbit + nbits - 1) >> 5;
    const uint64_t step = (uint64_t)gridDim.y * 256;
    for (uint64_t w = w0 + (uint64_t)blockIdx.y * 256 + threadIdx.x; w <= w1; w += step) {
        const uint32_t sw = knz_bswap32(knz_fetch32(src, (int64_t)(w << 5) - (int64_t)dbit, (int64_t)nbits));
        if (w == w0 || w == w1) atomicOr(&dst[w], sw);
        else dst[w] = sw;
    }
}

// ---- decode side ---------------------------------------------------------------------------------------------------------------------
// the first 32 bytes of every stream (zero padded), side by side: one copy brings all heads to the host's header parse
__global__ void knz_many_heads_kernel(const ManyStream* s, uint32_t K, uint32_t* heads) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K * 8) return;
    const ManyStream& m = s[i >> 3];
    const uint64_t o = (uint64_t)(i & 7) * 4;
    uint32_t v = 0;
    if (m.status == 0 && o < m.n) {
        v = ((const uint32_t*)m.src)[i & 7];                              // (4-byte aligned, readable to the next multiple of 4)
        if (m.n - o < 4) v &= 0xFFFFFFFFu >> (8 * (4 - (uint32_t)(m.n - o)));
    }
    heads[i] = v;
}

// grid (K, y): stream k's n bytes to stage + stage_off, zero filled to the next multiple of 16. 16-byte accesses where the source allows
// them, 4-byte words elsewhere (the destination is 16-byte aligned; the bytes behind n are cleared).
__device__ __forceinline__ void knz_many_stage_bytes(const uint8_t* src, uint8_t* dst, const uint64_t n) {
    const uint64_t units = (n + 15) >> 4;
    const bool aligned = ((uint64_t)src & 15) == 0;
    for (uint64_t u = (uint64_t)blockIdx.y * 256 + threadIdx.x; u < units; u += (uint64_t)gridDim.y * 256) {
        const uint64_t o = u << 4;
        if (aligned && o + 16 <= n) { *(uint4*)(dst + o) = *(const uint4*)(src + o); continue; }
        for (uint64_t q = o; q < o + 16; q += 4) {
            uint32_t v = 0;
            if (q < n) {
                v = *(const uint32_t*)(src + q);
                if (n - q < 4) v &= 0xFFFFFFFFu >> (8 * (4 - (uint32_t)(n - q)));
            }
            *(uint32_t*)(dst + q) = v;
        }
    }
}
__global__ __launch_bounds__(256) void knz_many_stage_kernel(const ManyStream* s, uint8_t* stage) {
    const ManyStream& m = s[blockIdx.x];
    if (m.status != 0) return;
    knz_many_stage_bytes((const uint8_t*)m.src, stage + m.stage_off, m.n);
}

// One row per entry of knz_dev_decompress_many_range, next to its ManyStream row. The count walk finds where the selected frames lie, the host
// turns that into the bytes to stage (src_off a multiple of 16, so that 16-byte copies stay possible where the caller's pointer allows them).
struct ManyRange {
    uint32_t from, to;               // block ids, the first block is 1 ; to exclusive, 0xFFFFFFFF: through the last block
    uint64_t start_bit;              // the count walk starts at this frame, as block start_id (the header's end as 1, or the caller's hint as `from`)
    uint32_t start_id, hinted;       // hinted: start_bit is the caller's, the frame it names has to be a block
    uint64_t first_frame;            // count walk: the frame of block `from`, where the fill walk starts
    uint64_t span_lo, span_hi;       // count walk: the bits of the stream that hold the selected payloads
    uint64_t src_off, len;           // host: the bytes [src_off, src_off + len) of the stream go to stage + stage_off
};

// grid (K, y): ... for a range call: only the bytes that cover entry k's selected frames, however long the stream around them is
__global__ __launch_bounds__(256) void knz_many_stage_range_kernel(const ManyStream* s, const ManyRange* rg, uint8_t* stage) {
    const ManyStream& m = s[blockIdx.x];
    if (m.status != 0 || m.nblocks == 0) return;
    const ManyRange& g = rg[blockIdx.x];
    knz_many_stage_bytes((const uint8_t*)m.src + g.src_off, stage + m.stage_off, g.len);
}

struct ManyWalkArgs {
    ManyStream* streams; uint32_t K;
    const uint8_t* stage;
    uint32_t fill;                   // 0: count the blocks of every stream ; 1: write their positions at first_block + i
    uint64_t* blk_bit; uint64_t* blk_bits; uint32_t* blk_stream;
};

// knz_dec_walk_stream_kernel for K streams side by side, one thread each, every walker bounded by its own stream's n bytes
__global__ void knz_many_walk_kernel(ManyWalkArgs a) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.K) return;
    ManyStream& s = a.streams[k];
    if (s.status != 0) return;
    const uint64_t end = s.stage_off + s.n, limit = end << 3;
    const uint64_t maxBlocks = a.fill ? s.nblocks : min(s.n / 3 + 1, (uint64_t)1 << 24);
    KnzStreamReader r;
    r.init(a.stage, end, (s.stage_off << 3) + s.hdr_bits);
    uint32_t n = 0, err = 0;
    for (;;) {                                                           // every turn moves at least 8 bits ahead, or ends the walk
        if (r.tell() + 8 > limit) { err = KNZ_ERR_PROCESS_BLOCK; break; }
        const uint32_t lr = r.read(5) + 3;
        uint64_t read = 0;
        if (lr > 32) { read = (uint64_t)r.read(lr - 32) << 32; read |= r.read(32); }
        else read = r.read(lr);
        if (read == 0) break;
        if (read > ((uint64_t)1 << 34)) { err = KNZ_ERR_BLOCK_SIZE; break; }
        const uint64_t pos = r.tell();
        if (pos + read > limit) { err = KNZ_ERR_PROCESS_BLOCK; break; }
        if (n >= maxBlocks) { err = KNZ_ERR_BLOCK_SIZE; break; }
        if (a.fill) { a.blk_bit[s.first_block + n] = pos; a.blk_bits[s.first_block + n] = read; a.blk_stream[s.first_block + n] = k; }
        n++;
        r.seek(pos + read);
    }
    if (!a.fill) { s.nblocks = err ? 0 : n; s.status = (int32_t)err; }
}

// ... with a range per stream (knz_dec_walk_range_kernel side by side). The walkers read the CALLER's buffers, each bounded by its own stream's n bytes:
// nothing is staged before it is known which bytes hold the selected frames. count: frames in front of `from` are skipped, the walk stops behind the last
// block of the range and leaves where its frames lie ; fill: from the first selected frame on, positions rebased to the entry's bytes in the staging buffer.
__global__ void knz_many_walk_range_kernel(ManyWalkArgs a, ManyRange* rg) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.K) return;
    ManyStream& s = a.streams[k];
    if (s.status != 0) return;
    ManyRange& g = rg[k];
    const uint64_t limit = s.n << 3;
    const uint64_t maxBlocks = min(s.n / 3 + 1, (uint64_t)1 << 24);
    const uint64_t to = a.fill ? (uint64_t)g.from + s.nblocks : (g.to == 0xFFFFFFFFu ? ~(uint64_t)0 : (uint64_t)g.to);
    const uint64_t rebase = (s.stage_off << 3) - (g.src_off << 3);       // (fill: modulo 2^64, src_off * 8 <= every position)
    uint64_t id = a.fill ? g.from : g.start_id;
    KnzStreamReader r;
    r.init((const uint8_t*)s.src, s.n, a.fill ? g.first_frame : g.start_bit);
    uint32_t n = 0, seen = 0, err = 0;
    uint64_t first = 0, lo = 0, hi = 0;
    while (id < to) {                                                    // every turn moves at least 8 bits ahead, or ends the walk
        const uint64_t at = r.tell();
        if (at + 8 > limit) { err = KNZ_ERR_PROCESS_BLOCK; break; }
        const uint32_t lr = r.read(5) + 3;
        uint64_t read = 0;
        if (lr > 32) { read = (uint64_t)r.read(lr - 32) << 32; read |= r.read(32); }
        else read = r.read(lr);
        if (read == 0) { if (!a.fill && g.hinted && seen == 0) err = KNZ_ERR_PROCESS_BLOCK; break; }
        if (read > ((uint64_t)1 << 34)) { err = KNZ_ERR_BLOCK_SIZE; break; }
        const uint64_t pos = r.tell();
        if (pos + read > limit) { err = KNZ_ERR_PROCESS_BLOCK; break; }
        if (seen >= maxBlocks) { err = KNZ_ERR_BLOCK_SIZE; break; }
        seen++;
        if (id >= g.from) {
            if (a.fill) { a.blk_bit[s.first_block + n] = pos + rebase; a.blk_bits[s.first_block + n] = read; a.blk_stream[s.first_block + n] = k; }
            else { if (n == 0) { first = at; lo = pos; } hi = pos + read; }
            n++;
        }
        id++;
        r.seek(pos + read);
    }
    if (!a.fill) {
        s.nblocks = err ? 0 : n; s.status = (int32_t)err;
        g.first_frame = first; g.span_lo = lo; g.span_hi = hi;
    }
}

struct ManyPlaceArgs {
    ManyStream* streams; uint32_t K;
    const uint32_t* blk_len;         // [nblocks] decoded bytes of every block
    const int32_t* blk_status;       // [nblocks]
    const uint32_t* blk_stream;
    uint64_t* blk_pos;               // [nblocks] out: byte offset of the block in its stream's destination
    const uint8_t* stage; uint64_t stride;   // block b decoded at stage + b * stride
    uint32_t block_size;
};

// One workgroup per stream: where every block goes (short inner blocks included: the sum of the lengths in front of it), whether each fits the
// stream's block size (Reader.processBlock :1707-1710) and the destination
__global__ __launch_bounds__(256) void knz_many_place_plan_kernel(ManyPlaceArgs a) {
    __shared__ uint64_t s_wsum[4];
    __shared__ uint64_t s_carry;
    __shared__ uint32_t s_bad;                       // the first block of the stream that failed
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    ManyStream& s = a.streams[blockIdx.x];
    if (s.status != 0) return;
    const uint32_t b0 = s.first_block, nb = s.nblocks;
    if (tid == 0) { s_carry = 0; s_bad = 0xFFFFFFFFu; }
    __syncthreads();
    for (uint32_t i0 = 0; i0 < nb; i0 += 256) {
        const uint32_t i = i0 + tid;
        uint64_t len = 0;
        if (i < nb) {
            len = a.blk_len[b0 + i];
            if (a.blk_status[b0 + i] != 0 || len > a.block_size) atomicMin(&s_bad, i);
        }
        uint64_t incl = len;
        for (int d = 1; d < 64; d <<= 1) { const uint64_t t = wave_shfl64(incl, lane - d); if (lane >= d) incl += t; }
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        uint64_t before = s_carry;
        for (int w = 0; w < wave; w++) before += s_wsum[w];
        if (i < nb) a.blk_pos[b0 + i] = before + incl - len;
        __syncthreads();
        if (tid == 255) s_carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) {
        int32_t status = 0;
        if (s_bad != 0xFFFFFFFFu) status = a.blk_status[b0 + s_bad] ? a.blk_status[b0 + s_bad] : (int32_t)KNZ_ERR_PROCESS_BLOCK;
        if (status == 0 && s_carry > s.cap) status = KNZ_ERR_WRITE_FILE;
        s.status = status; s.out = status ? 0 : s_carry;
    }
}

// grid (nblocks, y): decoded block b to its place in its stream's destination; nothing of a stream that failed is written
__global__ __launch_bounds__(256) void knz_many_place_copy_kernel(ManyPlaceArgs a) {
    const uint32_t b = blockIdx.x;
    const ManyStream& m = a.streams[a.blk_stream[b]];
    if (m.status != 0) return;
    const uint32_t n = a.blk_len[b];
    const uint8_t* s = a.stage + (uint64_t)b * a.stride;
    uint8_t* d = (uint8_t*)m.dst + a.blk_pos[b];
    for (uint32_t i = (blockIdx.y * 256 + threadIdx.x) * 16; i < n; i += gridDim.y * 256 * 16) {
        if (i + 16 <= n && ((((uintptr_t)(s + i)) | ((uintptr_t)(d + i))) & 15) == 0) *(uint4*)(d + i) = *(const uint4*)(s + i);
        else for (uint32_t j = i; j < n && j < i + 16; j++) d[j] = s[j];
    }
}
