// Byte writes into .knz streams (knz_dev_write_many / knz_dev_append, host side in knz_write.inc): W writes (byte offset, length, data of any alignment)
// into one source stream give one new stream. The blocks the writes touch are decoded by the many-streams range batch and placed side by side at a
// stride of one block size; the kernels below do the rest:
//   knz_write_overlay_kernel (the visible pieces of the writes into the decoded blocks: one thread per 16-byte destination chunk, its piece found by
//   binary search over the scan of the chunk counts) -> encode batch (block-local streams of the touched and the new blocks) ->
//   knz_write_splice_plan_kernel (one workgroup: scan of the new stream's pieces - header, runs of untouched frames, re-encoded frames, end marker -,
//   capacity check, framing fields (lw-3):5 written:lw of CompressedStream.go:951-976) -> knz_write_splice_copy_kernel (one thread per 16 destination
//   bytes, every 32-bit word composed from all the pieces that have bits in it: no word is written twice, nothing is zeroed and OR-ed).
// The host's sweep leaves disjoint visible pieces (a later write wins): no two threads of the overlay store to the same byte. Untouched frames move as
// bits: a different size field in the header, or a length field that changed its width, shifts every frame behind it by any number of bits.
#include "bits.h"
#include "wave.h"

struct WriteCopy {                   // one visible piece of a write: len bytes from src (any alignment) to dst (any alignment, inside the decoded blocks)
    uint64_t dst, src, len;
};

struct WriteOverlayArgs {
    const WriteCopy* pieces; uint32_t K;
    const uint64_t* base;            // [K + 1] exclusive scan of the pieces' 16-byte destination chunks (the host made both), base[K] their sum
};

// One thread per destination chunk (the grid may be shorter than the chunks: it strides). Every byte it stores lies in its piece's dst[0 .. len).
__global__ __launch_bounds__(256) void knz_write_overlay_kernel(WriteOverlayArgs a) {
    const uint64_t total = a.base[a.K];
    uint32_t own = 0;                                                     // the piece of the thread's last chunk: a long piece keeps it over the turns
    uint64_t own_lo = 0, own_hi = 0;                                      // ... and its chunks [own_lo, own_hi)
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (uint64_t)gridDim.x * 256) {
        if (g >= own_hi) {
            uint32_t lo = 0, hi = a.K;                                    // invariant: base[lo] <= g < base[hi]
            while (hi - lo > 1) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (a.base[mid] <= g) lo = mid; else hi = mid;
            }
            own = lo; own_lo = a.base[lo]; own_hi = a.base[lo + 1];
        }
        const WriteCopy p = a.pieces[own];
        const uint64_t d = p.dst, at = (d & ~(uint64_t)15) + ((g - own_lo) << 4);    // the chunk's address: bytes [k0, k1) of the piece lie in it
        const uint64_t k0 = at > d ? at - d : 0, k1 = min(at + 16 - d, p.len);
        const uint8_t* src = (const uint8_t*)(p.src + k0);
        if (k1 - k0 == 16) {
            // interior chunk: the 16 bytes from src on, fetched as the aligned words that hold them, one aligned store
            const uint32_t* q = (const uint32_t*)((uintptr_t)src & ~(uintptr_t)3);
            const uint32_t sh = (uint32_t)((uintptr_t)src & 3) * 8;
            const KnzWords4 v = *(const KnzWords4*)q;
            const uint32_t v4 = sh ? q[4] : 0;                            // (sh != 0: byte 15 of the chunk lies in that word)
            uint4 o;
            o.x = knz_read_funnel(v.a, v.b, sh); o.y = knz_read_funnel(v.b, v.c, sh); o.z = knz_read_funnel(v.c, v.d, sh); o.w = knz_read_funnel(v.d, v4, sh);
            *(uint4*)at = o;
            continue;
        }
        uint8_t* dp = (uint8_t*)(d + k0);                                 // ragged head or tail of the piece: byte by byte
        for (uint64_t k = k0; k < k1; k++) *dp++ = *src++;
    }
}

// ---- the splice: the new stream as a list of pieces ----------------------------------------------------------------------------------------
enum { KNZ_WP_HEADER = 0, KNZ_WP_RUN = 1, KNZ_WP_FRAME = 2, KNZ_WP_END = 3 };

struct WritePiece {                  // the host fills kind, src and (header, run) nbits ; the plan kernel the rest
    uint64_t src;                    // run: bit position of its first frame in the source stream ; frame: its row of the encode batch
    uint64_t nbits;                  // header, run: given ; frame: framing field + block-local bits ; end marker: 8
    uint64_t dst_bit;                // plan: where the piece starts in the new stream
    uint64_t field;                  // frame, plan: (lw - 3):5 written:lw, right aligned
    uint32_t kind, fbits;            // frame, plan: 5 + lw
};

struct WriteSpliceArgs {
    WritePiece* pieces; uint32_t P;
    const uint64_t* written;         // [rows] exact bit count of every block-local stream of the encode batch
    const uint32_t* old_words;       // the source stream, 4-byte aligned
    const uint8_t* streams; uint64_t stride;     // row r's block-local stream at streams + r * stride (64-byte aligned)
    uint32_t hdr_words[8];           // the new header, BE words as values
    uint32_t* dst; uint64_t cap;     // the caller's d_dst and dst_cap
    uint64_t* result;                // [2] plan: {status, total bits}
};

// One workgroup: every piece's size, their exclusive scan, the total against dst_cap (whole BE words are stored, the last of them inside dst_cap:
// the rule of knz_layout_stream_kernel). Nothing of the destination is written here, and nothing by the copy kernel unless the status is 0.
__global__ __launch_bounds__(256) void knz_write_splice_plan_kernel(WriteSpliceArgs a) {
    __shared__ uint64_t s_wsum[4];
    __shared__ uint64_t s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t i0 = 0; i0 < a.P; i0 += 256) {
        const uint32_t i = i0 + tid;
        uint64_t sz = 0;
        if (i < a.P) {
            WritePiece& p = a.pieces[i];
            if (p.kind == KNZ_WP_FRAME) {
                const uint64_t written = a.written[p.src];
                const uint32_t lw = knz_many_lw(written);
                p.field = ((uint64_t)(lw - 3) << lw) | written;
                p.fbits = 5 + lw;
                p.nbits = p.fbits + written;
            } else if (p.kind == KNZ_WP_END) p.nbits = 8;                 // (3 - 3):5, 0:3
            sz = p.nbits;
        }
        uint64_t incl = sz;
        for (int d = 1; d < 64; d <<= 1) { const uint64_t t = wave_shfl64(incl, lane - d); if (lane >= d) incl += t; }
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        uint64_t before = s_carry;
        for (int w = 0; w < wave; w++) before += s_wsum[w];
        if (i < a.P) a.pieces[i].dst_bit = before + incl - sz;
        __syncthreads();
        if (tid == 255) s_carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) {
        const uint64_t total = s_carry;
        const uint64_t usable = a.cap >= 8 ? ((a.cap & ~(uint64_t)3) - 4) : 0;
        a.result[0] = total > usable * 8 ? (uint64_t)KNZ_ERR_WRITE_FILE : 0;
        a.result[1] = total;
    }
}

// cnt <= 32 bits from bit `bit` on of a string of BE words, in the top bits of the result (the others 0). The string ends at bit `limit`: the word
// behind the one that holds `bit` is read only where it holds bits of the string. swap: the words are in memory (else they are values already).
__device__ __forceinline__ uint32_t knz_write_bits(const uint32_t* words, uint64_t bit, uint32_t cnt, uint64_t limit, bool swap) {
    const uint64_t q = bit >> 5;
    const uint32_t r = (uint32_t)bit & 31;
    uint32_t w0 = words[q], w1 = (r && ((q + 1) << 5) < limit) ? words[q + 1] : 0u;
    if (swap) { w0 = knz_bswap32(w0); w1 = knz_bswap32(w1); }
    uint32_t v = r ? ((w0 << r) | (w1 >> (32 - r))) : w0;
    if (cnt < 32) v &= ~(0xFFFFFFFFu >> cnt);
    return v;
}

// bits [rel, rel + cnt) of piece p, cnt in 1 .. 32, in the top bits of the result
__device__ __forceinline__ uint32_t knz_write_piece_bits(const WriteSpliceArgs& a, const WritePiece& p, uint64_t rel, uint32_t cnt) {
    if (p.kind == KNZ_WP_HEADER) return knz_write_bits(a.hdr_words, rel, cnt, p.nbits, false);
    if (p.kind == KNZ_WP_RUN) return knz_write_bits(a.old_words, p.src + rel, cnt, p.src + p.nbits, true);
    if (p.kind == KNZ_WP_END) return 0u;
    const uint32_t* row = (const uint32_t*)(a.streams + p.src * a.stride);
    const uint64_t written = p.nbits - p.fbits;
    if (rel >= p.fbits) return knz_write_bits(row, rel - p.fbits, cnt, written, true);
    const uint32_t take = min(cnt, p.fbits - (uint32_t)rel);              // the framing field first (up to 42 bits of it), then the block's own bits
    const uint32_t f = (uint32_t)(p.field >> (p.fbits - (uint32_t)rel - take)) & (0xFFFFFFFFu >> (32 - take));
    uint32_t v = f << (32 - take);
    if (cnt > take) v |= knz_write_bits(row, 0, cnt - take, written, true) >> take;
    return v;
}

// the last piece that starts at or in front of `bit` (pieces are never empty, piece 0 starts at bit 0)
__device__ __forceinline__ uint32_t knz_write_piece_at(const WriteSpliceArgs& a, uint64_t bit) {
    uint32_t lo = 0, hi = a.P;                                            // invariant: dst_bit[lo] <= bit < dst_bit[hi] (hi == P: the end)
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a.pieces[mid].dst_bit <= bit) lo = mid; else hi = mid;
    }
    return lo;
}

// destination word w (a BE value), composed from every piece with bits in it, from piece p on ; bits behind the end marker are 0
__device__ __forceinline__ uint32_t knz_write_compose(const WriteSpliceArgs& a, uint64_t w, uint32_t p) {
    const uint64_t b0 = w << 5, b1 = b0 + 32;
    uint32_t acc = 0;
    for (; p < a.P; p++) {
        const WritePiece& pc = a.pieces[p];
        if (pc.dst_bit >= b1) break;
        const uint64_t lo = max(pc.dst_bit, b0), hi = min(pc.dst_bit + pc.nbits, b1);
        if (hi > lo) acc |= knz_write_piece_bits(a, pc, lo - pc.dst_bit, (uint32_t)(hi - lo)) >> (uint32_t)(lo - b0);
    }
    return acc;
}

// One thread per 16 aligned bytes of the destination (d_dst itself is only 4-byte aligned: the first group is short). A group that lies inside one
// run of untouched frames, or inside one block-local stream, is five source words funnel-shifted into one 16-byte store; every other word is composed
// from its pieces (a 1-byte block's frame is shorter than a word: three pieces and more meet in one). The last word is filled with zeros.
__global__ __launch_bounds__(256) void knz_write_splice_copy_kernel(WriteSpliceArgs a) {
    if (a.result[0] != 0) return;
    const uint64_t total = a.result[1];
    const uint64_t nwords = (((total + 7) >> 3) + 3) >> 2;
    const uint64_t lead = ((uintptr_t)a.dst & 15) >> 2;
    const uint64_t groups = (nwords + lead + 3) >> 2;
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * 256) {
        const uint64_t w0 = g * 4 >= lead ? g * 4 - lead : 0, w1 = min(g * 4 - lead + 4, nwords);      // (g == 0: 4 - lead words)
        const uint32_t p0 = knz_write_piece_at(a, w0 << 5);
        const WritePiece& pc = a.pieces[p0];
        if (w1 - w0 == 4 && (pc.kind == KNZ_WP_RUN || pc.kind == KNZ_WP_FRAME)) {
            const uint64_t from = pc.dst_bit + (pc.kind == KNZ_WP_FRAME ? pc.fbits : 0);
            if ((w0 << 5) >= from && (w1 << 5) <= pc.dst_bit + pc.nbits) {
                const uint32_t* words = pc.kind == KNZ_WP_RUN ? a.old_words : (const uint32_t*)(a.streams + pc.src * a.stride);
                const uint64_t s = (pc.kind == KNZ_WP_RUN ? pc.src : 0) + ((w0 << 5) - from);
                const uint32_t r = (uint32_t)s & 31;
                const KnzWords4 v = *(const KnzWords4*)(words + (s >> 5));
                const uint32_t x0 = knz_bswap32(v.a), x1 = knz_bswap32(v.b), x2 = knz_bswap32(v.c), x3 = knz_bswap32(v.d);
                const uint32_t x4 = r ? knz_bswap32(words[(s >> 5) + 4]) : 0;                     // (r != 0: the group's last bit lies in that word)
                uint4 o;
                o.x = knz_bswap32(r ? (x0 << r) | (x1 >> (32 - r)) : x0); o.y = knz_bswap32(r ? (x1 << r) | (x2 >> (32 - r)) : x1);
                o.z = knz_bswap32(r ? (x2 << r) | (x3 >> (32 - r)) : x2); o.w = knz_bswap32(r ? (x3 << r) | (x4 >> (32 - r)) : x3);
                *(uint4*)(a.dst + w0) = o;
                continue;
            }
        }
        uint32_t p = p0;
        for (uint64_t w = w0; w < w1; w++) {
            while (p + 1 < a.P && a.pieces[p + 1].dst_bit <= (w << 5)) p++;
            a.dst[w] = knz_bswap32(knz_write_compose(a, w, p));
        }
    }
}
