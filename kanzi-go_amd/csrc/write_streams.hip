// Byte writes into MANY .knz streams (knz_dev_write_streams, host side in knz_write_streams.inc): T targets (one source stream, one new stream each) and
// W writes that name their target, in ONE pass of every stage of knz_dev_write_many: framing, decode batch, overlay, encode batch, splice. The overlay is
// write.hip's kernel as it stands (its pieces carry absolute addresses) ; the kernels here are the framing walk and the splice over a table of targets:
//   knz_ws_walk_kernel (ONE thread per DISTINCT source, the frame step of knz_dec_walk_range_kernel with its bound and its codes: a count pass, then a
//   fill pass that leaves every frame's payload bit and bit count in the rows the count pass has sized) ->
//   ... decode batch, knz_write_overlay_kernel, encode batch (block-local streams of all targets' touched and new blocks, rows side by side) ... ->
//   knz_ws_plan_kernel (one workgroup per target: scan of its pieces - header, runs of untouched frames, re-encoded frames, end marker -, framing fields
//   (lw-3):5 written:lw, the total against the target's dst_cap, the target's 16-byte destination groups) -> knz_read_scan_kernel (read.hip, as it stands:
//   exclusive scan of the targets' group counts) -> knz_ws_copy_kernel (ONE launch for all targets, one thread per 16 aligned destination bytes: its
//   target by binary search over the scan, its piece by binary search over that target's pieces, every 32-bit word composed from all the pieces that
//   have bits in it: no word is written twice, nothing is zeroed and OR-ed, no atomics).
// A failed target has no groups: no byte of its destination is written. Outputs may be packed to the word: an output's first and last group are short,
// and neither stores outside the words the plan kernel has checked against its own dst_cap.
#include "bits.h"
#include "wave.h"

struct WsSource {                    // one row per distinct (d_src, n_bytes) of the batch
    uint64_t src, n;
    uint64_t row_first;              // fill pass: its frames are rows row_first .. of frames[]
    uint32_t first_bit;              // the first frame's bit (the header's end)
    int32_t status;                  // refused by the host (header, configuration): not walked
    uint32_t count;                  // out: its frames
    int32_t err;                     // out: the walk's code
};

struct WsFrame { uint64_t bit, bits; };      // a frame's payload: its first bit and its bit count (the frame starts where the one before it ends)

struct WsWalkArgs { WsSource* sources; uint32_t S; uint32_t fill; WsFrame* frames; };

// One thread per distinct source, from the header to the end marker. Every turn checks its frame against the source's last bit before it moves on, and
// the reader returns 0 for words behind d_src[0 .. n) rounded up to 4. fill: a row is stored only below the count the first pass has left.
__global__ __launch_bounds__(64) void knz_ws_walk_kernel(WsWalkArgs a) {
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k >= a.S) return;
    const WsSource s = a.sources[k];
    if (s.status != 0 || (a.fill && (s.err != 0 || s.count == 0))) return;
    const uint64_t limit = s.n << 3;
    const uint64_t maxBlocks = min(s.n / 3 + 1, (uint64_t)1 << 24);
    KnzStreamReader r;
    r.init((const uint8_t*)s.src, s.n, s.first_bit);
    uint32_t count = 0, err = 0;
    for (;;) {                                                            // every turn moves at least 8 bits ahead, or ends the walk
        const uint64_t at = r.tell();
        if (at + 8 > limit) { err = KNZ_ERR_PROCESS_BLOCK; break; }
        const uint32_t lr = r.read(5) + 3;
        uint64_t read = 0;
        if (lr > 32) { read = (uint64_t)r.read(lr - 32) << 32; read |= r.read(32); }
        else read = r.read(lr);
        if (read == 0) break;
        if (read > ((uint64_t)1 << 34)) { err = KNZ_ERR_BLOCK_SIZE; break; }
        const uint64_t pos = r.tell();
        if (pos + read > limit) { err = KNZ_ERR_PROCESS_BLOCK; break; }
        if (count >= maxBlocks) { err = KNZ_ERR_BLOCK_SIZE; break; }
        if (a.fill) {
            if (count >= s.count) break;                                  // (the stream changed between the passes: nothing behind the rows is stored)
            WsFrame f;
            f.bit = pos; f.bits = read;
            a.frames[s.row_first + count] = f;
        }
        count++;
        r.seek(pos + read);
    }
    if (!a.fill) { a.sources[k].count = count; a.sources[k].err = (int32_t)err; }
}

// ---- the splice over a table of targets ----------------------------------------------------------------------------------------------------------
struct WsOut {                       // one row per target: the host fills the inputs, the plan kernel the results
    uint64_t dst, cap;               // the caller's d_dst and dst_cap
    uint64_t old_words;              // its source stream, 4-byte aligned
    uint32_t hdr_words[8];           // the new header, BE words as values
    uint32_t piece_first, P;         // its pieces: rows piece_first .. of pieces[] (write.hip's WritePiece ; a frame's src is its row of the encode batch)
    int32_t status;                  // in: failed so far (it has no pieces then) ; out: that, or KNZ_ERR_WRITE_FILE
    uint32_t reserved;
    uint64_t total_bits;             // out
};

struct WsArgs {
    WsOut* outs; uint32_t T;
    WritePiece* pieces;
    const uint64_t* written;         // [rows] exact bit count of every block-local stream of the encode batch
    const uint8_t* streams; uint64_t stride;     // row r's block-local stream at streams + r * stride (64-byte aligned)
    uint64_t* base;                  // [T + 1] plan: the targets' group counts ; scan: their exclusive scan, base[T] their sum
};

// One workgroup per target: knz_write_splice_plan_kernel over the target's own pieces. Nothing of a destination is written here, and nothing by the copy
// kernel unless the status is 0.
__global__ __launch_bounds__(256) void knz_ws_plan_kernel(WsArgs a) {
    __shared__ uint64_t s_wsum[4];
    __shared__ uint64_t s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    WsOut& o = a.outs[blockIdx.x];
    const uint32_t P = o.status ? 0 : o.P;
    WritePiece* pcs = a.pieces + o.piece_first;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t i0 = 0; i0 < P; i0 += 256) {
        const uint32_t i = i0 + tid;
        uint64_t sz = 0;
        if (i < P) {
            WritePiece& p = pcs[i];
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
        if (i < P) pcs[i].dst_bit = before + incl - sz;
        __syncthreads();
        if (tid == 255) s_carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) {
        const uint64_t total = s_carry;
        const uint64_t usable = o.cap >= 8 ? ((o.cap & ~(uint64_t)3) - 4) : 0;
        int32_t status = o.status;
        if (status == 0 && total > usable * 8) status = KNZ_ERR_WRITE_FILE;
        const uint64_t nwords = (((total + 7) >> 3) + 3) >> 2, lead = (o.dst & 15) >> 2;
        o.status = status; o.total_bits = status ? 0 : total;
        a.base[blockIdx.x] = status ? 0 : (nwords + lead + 3) >> 2;
    }
}

// bits [rel, rel + cnt) of piece p of target o, cnt in 1 .. 32, in the top bits of the result (knz_write_piece_bits with the target's header and source)
__device__ __forceinline__ uint32_t knz_ws_piece_bits(const WsArgs& a, const WsOut& o, const WritePiece& p, uint64_t rel, uint32_t cnt) {
    if (p.kind == KNZ_WP_HEADER) return knz_write_bits(o.hdr_words, rel, cnt, p.nbits, false);
    if (p.kind == KNZ_WP_RUN) return knz_write_bits((const uint32_t*)o.old_words, p.src + rel, cnt, p.src + p.nbits, true);
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

// the last piece of pcs[0 .. P) that starts at or in front of `bit` (pieces are never empty, piece 0 starts at bit 0)
__device__ __forceinline__ uint32_t knz_ws_piece_at(const WritePiece* pcs, uint32_t P, uint64_t bit) {
    uint32_t lo = 0, hi = P;                                              // invariant: dst_bit[lo] <= bit < dst_bit[hi] (hi == P: the end)
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (pcs[mid].dst_bit <= bit) lo = mid; else hi = mid;
    }
    return lo;
}

// destination word w (a BE value) of target o, composed from every piece with bits in it, from piece p on ; bits behind the end marker are 0
__device__ __forceinline__ uint32_t knz_ws_compose(const WsArgs& a, const WsOut& o, const WritePiece* pcs, uint32_t P, uint64_t w, uint32_t p) {
    const uint64_t b0 = w << 5, b1 = b0 + 32;
    uint32_t acc = 0;
    for (; p < P; p++) {
        const WritePiece& pc = pcs[p];
        if (pc.dst_bit >= b1) break;
        const uint64_t lo = max(pc.dst_bit, b0), hi = min(pc.dst_bit + pc.nbits, b1);
        if (hi > lo) acc |= knz_ws_piece_bits(a, o, pc, lo - pc.dst_bit, (uint32_t)(hi - lo)) >> (uint32_t)(lo - b0);
    }
    return acc;
}

// One thread per 16 aligned bytes of some target's destination (the grid may be shorter than the groups: it strides ; d_dst itself is only 4-byte
// aligned: a target's first group is short, and so is its last). A group that lies inside one run of untouched frames, or inside one block-local
// stream, is five source words funnel-shifted into one 16-byte store ; every other word is composed from its pieces. A target's last word is filled
// with zeros. Every store lies in the words the plan kernel has checked against the target's dst_cap.
__global__ __launch_bounds__(256) void knz_ws_copy_kernel(WsArgs a) {
    const uint64_t total = a.base[a.T];
    uint32_t own = 0;                                                     // the target of the thread's last group: a long output keeps it over the turns
    uint64_t own_lo = 0, own_hi = 0;                                      // ... and its groups [own_lo, own_hi)
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (uint64_t)gridDim.x * 256) {
        if (g >= own_hi) {
            uint32_t lo = 0, hi = a.T;                                    // invariant: base[lo] <= g < base[hi] (targets without groups share their successor's base)
            while (hi - lo > 1) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (a.base[mid] <= g) lo = mid; else hi = mid;
            }
            own = lo; own_lo = a.base[lo]; own_hi = a.base[lo + 1];
        }
        const WsOut& o = a.outs[own];
        const WritePiece* pcs = a.pieces + o.piece_first;
        const uint32_t P = o.P;
        uint32_t* dst = (uint32_t*)o.dst;
        const uint64_t nwords = (((o.total_bits + 7) >> 3) + 3) >> 2;
        const uint64_t lead = (o.dst & 15) >> 2, q = (g - own_lo) * 4;
        const uint64_t w0 = q >= lead ? q - lead : 0, w1 = min(q - lead + 4, nwords);               // (q == 0: 4 - lead words)
        const uint32_t p0 = knz_ws_piece_at(pcs, P, w0 << 5);
        const WritePiece& pc = pcs[p0];
        if (w1 - w0 == 4 && (pc.kind == KNZ_WP_RUN || pc.kind == KNZ_WP_FRAME)) {
            const uint64_t from = pc.dst_bit + (pc.kind == KNZ_WP_FRAME ? pc.fbits : 0);
            if ((w0 << 5) >= from && (w1 << 5) <= pc.dst_bit + pc.nbits) {
                const uint32_t* words = pc.kind == KNZ_WP_RUN ? (const uint32_t*)o.old_words : (const uint32_t*)(a.streams + pc.src * a.stride);
                const uint64_t s = (pc.kind == KNZ_WP_RUN ? pc.src : 0) + ((w0 << 5) - from);
                const uint32_t r = (uint32_t)s & 31;
                const KnzWords4 v = *(const KnzWords4*)(words + (s >> 5));
                const uint32_t x0 = knz_bswap32(v.a), x1 = knz_bswap32(v.b), x2 = knz_bswap32(v.c), x3 = knz_bswap32(v.d);
                const uint32_t x4 = r ? knz_bswap32(words[(s >> 5) + 4]) : 0;                     // (r != 0: the group's last bit lies in that word)
                uint4 v4;
                v4.x = knz_bswap32(r ? (x0 << r) | (x1 >> (32 - r)) : x0); v4.y = knz_bswap32(r ? (x1 << r) | (x2 >> (32 - r)) : x1);
                v4.z = knz_bswap32(r ? (x2 << r) | (x3 >> (32 - r)) : x2); v4.w = knz_bswap32(r ? (x3 << r) | (x4 >> (32 - r)) : x3);
                *(uint4*)(dst + w0) = v4;
                continue;
            }
        }
        uint32_t p = p0;
        for (uint64_t w = w0; w < w1; w++) {
            while (p + 1 < P && pcs[p + 1].dst_bit <= (w << 5)) p++;
            dst[w] = knz_bswap32(knz_ws_compose(a, o, pcs, P, w, p));
        }
    }
}
