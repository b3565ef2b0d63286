// Block splice (knz_dev_splice_many / knz_dev_concat / knz_dev_slice, host side in knz_splice.inc): parts (source stream, block range) become output
// streams, header + the parts' frames in part order + end marker, and nothing is decoded or encoded: whole frames move as bits. The kernels:
//   knz_splice_walk_kernel (ONE thread per DISTINCT source: the framing from the header to the largest boundary some part asks for, the frame-start bit
//   and the block count left at every boundary it passes) -> knz_splice_plan_kernel (one workgroup per output: scan of its pieces - header, one run per
//   part, end marker -, the parts' results, the check against dst_cap, the output's 16-byte destination groups) -> knz_read_scan_kernel (read.hip, as it
//   stands: exclusive scan of the outputs' group counts) -> knz_splice_copy_kernel (ONE launch for all outputs, one thread per 16 aligned destination
//   bytes: its output by binary search over the scan, its piece by binary search over that output's pieces, every 32-bit word composed from all the
//   pieces that have bits in it: no word is written twice, nothing is zeroed and OR-ed, no atomics).
// It is knz_write_splice_copy_kernel (write.hip) with a source pointer per piece and an output per group; knz_write_bits is write.hip's, called as it
// stands. Unlike there, EMPTY PIECES ARE ORDINARY here (a stream of header + end marker, a range behind the last block): they stay in the table. An
// empty piece shares its successor's destination bit, so the search for "the last piece that starts at or in front of a bit" steps over it to the
// piece that holds the bit, and the composition skips what has no bits in the word.
#include "bits.h"
#include "wave.h"

#define KNZ_SPLICE_END 0xFFFFFFFFu   // a boundary behind every block: the walk runs to the end marker

struct SpliceSource {                // one row per distinct (d_src, n_bytes) of the call
    uint64_t src, n;
    uint32_t first_bit;              // the first frame's bit (the header's end)
    uint32_t b_first, b_count;       // its boundaries: rows b_first .. of bounds[] / marks[], ascending, distinct
    int32_t status;                  // refused by the host (pointer, header, configuration): not walked
};

struct SpliceMark {                  // what the walk leaves at a boundary of `count` blocks: the state once that many frames are passed, or where the stream ended
    uint64_t bit;                    // the bit of the next frame (of the end marker's frame where the stream ended in front of the boundary)
    uint32_t count;                  // frames passed: min(boundary, blocks of the stream)
    int32_t status;                  // the walk's code where it failed at or in front of this boundary
};

struct SplicePart {                  // one row per part: the host fills the inputs, the plan kernel the results
    uint32_t source;                 // its row of sources[]
    uint32_t lo, hi;                 // its marks: boundary from_block - 1 and boundary to_block - 1 of its source
    int32_t status;                  // in: refused by the host ; out: that, or the walk's code
    uint64_t blocks, bits;           // out
};

enum { KNZ_SP_HEADER = 0, KNZ_SP_RUN = 1, KNZ_SP_END = 2 };
struct SplicePiece {                 // plan: output o's pieces are rows part_first + 2 * o .. : header, its parts, end marker
    uint64_t src;                    // header: the output row's hdr_words ; run: the source stream, 4-byte aligned
    uint64_t src_bit, nbits, dst_bit;
    uint32_t kind, reserved;
};

struct SpliceOut {                   // one row per output: the host fills the inputs, the plan kernel the results
    uint64_t dst, cap;               // the caller's d_dst and dst_cap
    uint32_t hdr_words[8];           // the output's header, BE words as values
    uint32_t hdr_bits;
    uint32_t part_first, n_parts;    // its parts (consecutive rows)
    int32_t status;                  // in: refused by the host ; out: that, the code of its first failing part, or KNZ_ERR_WRITE_FILE
    uint64_t total_bits, blocks;     // out
};

struct SpliceArgs {
    const SpliceSource* sources; uint32_t S;
    const uint32_t* bounds; SpliceMark* marks;
    SplicePart* parts;
    SpliceOut* outs; uint32_t O;
    SplicePiece* pieces;
    uint64_t* base;                  // [O + 1] plan: the outputs' group counts ; scan: their exclusive scan, base[O] their sum
};

// One thread per distinct source. The frame step is knz_dec_walk_range_kernel's, with its bound and its codes: every turn checks its frame against the
// source's last bit before it moves on, and the reader returns 0 for words behind d_src[0 .. n) rounded up to 4. A finite boundary ends the walk once
// that many frames are passed: framing behind the largest boundary is not read. KNZ_SPLICE_END runs to the end marker.
__global__ __launch_bounds__(64) void knz_splice_walk_kernel(SpliceArgs a) {
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k >= a.S) return;
    const SpliceSource s = a.sources[k];
    if (s.status != 0 || s.b_count == 0) return;
    const uint64_t limit = s.n << 3;
    const uint64_t maxBlocks = min(s.n / 3 + 1, (uint64_t)1 << 24);
    KnzStreamReader r;
    uint64_t at = s.first_bit;
    uint32_t count = 0, err = 0;
    bool ended = false;
    r.init((const uint8_t*)s.src, s.n, at);
    for (uint32_t j = 0; j < s.b_count; j++) {
        const uint32_t target = a.bounds[s.b_first + j];
        while (err == 0 && !ended && count < target) {                    // every turn moves at least 8 bits ahead, or ends the walk
            if (at + 8 > limit) { err = KNZ_ERR_PROCESS_BLOCK; break; }
            const uint32_t lr = r.read(5) + 3;
            uint64_t read = 0;
            if (lr > 32) { read = (uint64_t)r.read(lr - 32) << 32; read |= r.read(32); }
            else read = r.read(lr);
            if (read == 0) { ended = true; break; }
            if (read > ((uint64_t)1 << 34)) { err = KNZ_ERR_BLOCK_SIZE; break; }
            const uint64_t pos = r.tell();
            if (pos + read > limit) { err = KNZ_ERR_PROCESS_BLOCK; break; }
            if (count >= maxBlocks) { err = KNZ_ERR_BLOCK_SIZE; break; }
            count++;
            at = pos + read;
            r.seek(at);
        }
        SpliceMark m;
        m.bit = at; m.count = count; m.status = (int32_t)err;
        a.marks[s.b_first + j] = m;
    }
}

// One workgroup per output: every piece's size, their exclusive scan, the total against dst_cap (knz_write_splice_plan_kernel's rule: whole BE words
// are stored, the last of them inside dst_cap). Nothing of a destination is written here, and nothing by the copy kernel unless the status is 0: a
// failed output has no groups.
__global__ __launch_bounds__(256) void knz_splice_plan_kernel(SpliceArgs a) {
    __shared__ uint64_t s_wsum[4], s_bsum[4];
    __shared__ uint64_t s_carry, s_blocks;
    __shared__ uint32_t s_bad;                       // the first part of the output that failed
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    SpliceOut& o = a.outs[blockIdx.x];
    const uint32_t P = o.n_parts + 2;
    SplicePiece* pcs = a.pieces + o.part_first + 2 * (uint64_t)blockIdx.x;
    if (tid == 0) { s_carry = 0; s_blocks = 0; s_bad = 0xFFFFFFFFu; }
    __syncthreads();
    for (uint32_t i0 = 0; i0 < P; i0 += 256) {
        const uint32_t i = i0 + tid;
        uint64_t sz = 0, nb = 0;
        SplicePiece pc;
        pc.src = 0; pc.src_bit = 0; pc.kind = KNZ_SP_END; pc.reserved = 0;
        if (i == 0) { sz = o.hdr_bits; pc.kind = KNZ_SP_HEADER; pc.src = (uint64_t)o.hdr_words; }
        else if (i == P - 1) sz = 8;                                      // the end marker: (3 - 3):5, 0:3
        else if (i < P) {
            SplicePart& pt = a.parts[o.part_first + i - 1];
            int32_t st = pt.status;
            pc.kind = KNZ_SP_RUN;
            if (st == 0) {
                const SpliceMark lo = a.marks[pt.lo], hi = a.marks[pt.hi];
                st = lo.status ? lo.status : hi.status;
                if (st == 0) { sz = hi.bit - lo.bit; nb = hi.count - lo.count; pc.src_bit = lo.bit; pc.src = a.sources[pt.source].src; }
            }
            pt.status = st; pt.blocks = nb; pt.bits = sz;
            if (st != 0) atomicMin(&s_bad, i - 1);
        }
        uint64_t incl = sz, bincl = nb;
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t t = wave_shfl64(incl, lane - d), u = wave_shfl64(bincl, lane - d);
            if (lane >= d) { incl += t; bincl += u; }
        }
        if (lane == 63) { s_wsum[wave] = incl; s_bsum[wave] = bincl; }
        __syncthreads();
        uint64_t before = s_carry, bbefore = s_blocks;
        for (int w = 0; w < wave; w++) { before += s_wsum[w]; bbefore += s_bsum[w]; }
        if (i < P) { pc.nbits = sz; pc.dst_bit = before + incl - sz; pcs[i] = pc; }
        __syncthreads();
        if (tid == 255) { s_carry = before + incl; s_blocks = bbefore + bincl; }
        __syncthreads();
    }
    if (tid == 0) {
        const uint64_t total = s_carry;
        const uint64_t usable = o.cap >= 8 ? ((o.cap & ~(uint64_t)3) - 4) : 0;
        int32_t status = o.status;
        if (status == 0 && s_bad != 0xFFFFFFFFu) status = a.parts[o.part_first + s_bad].status;
        if (status == 0 && total > usable * 8) status = KNZ_ERR_WRITE_FILE;
        const uint64_t nwords = (((total + 7) >> 3) + 3) >> 2, lead = (o.dst & 15) >> 2;
        o.status = status; o.total_bits = status ? 0 : total; o.blocks = status ? 0 : s_blocks;
        a.base[blockIdx.x] = status ? 0 : (nwords + lead + 3) >> 2;
    }
}

// bits [rel, rel + cnt) of piece p, cnt in 1 .. 32, in the top bits of the result
__device__ __forceinline__ uint32_t knz_splice_piece_bits(const SplicePiece& p, uint64_t rel, uint32_t cnt) {
    if (p.kind == KNZ_SP_END) return 0u;
    const bool run = p.kind == KNZ_SP_RUN;
    return knz_write_bits((const uint32_t*)p.src, p.src_bit + rel, cnt, p.src_bit + p.nbits, run);
}

// the last piece that starts at or in front of `bit` (piece 0 starts at bit 0 ; empty pieces start where their successor does: never the answer
// unless the bit lies behind the stream)
__device__ __forceinline__ uint32_t knz_splice_piece_at(const SplicePiece* pcs, uint32_t P, uint64_t bit) {
    uint32_t lo = 0, hi = P;                                              // invariant: dst_bit[lo] <= bit < dst_bit[hi] (hi == P: the end)
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (pcs[mid].dst_bit <= bit) lo = mid; else hi = mid;
    }
    return lo;
}

// destination word w (a BE value), composed from every piece with bits in it, from piece p on ; bits behind the end marker are 0
__device__ __forceinline__ uint32_t knz_splice_compose(const SplicePiece* pcs, uint32_t P, uint64_t w, uint32_t p) {
    const uint64_t b0 = w << 5, b1 = b0 + 32;
    uint32_t acc = 0;
    for (; p < P; p++) {
        const SplicePiece& pc = pcs[p];
        if (pc.dst_bit >= b1) break;
        const uint64_t lo = max(pc.dst_bit, b0), hi = min(pc.dst_bit + pc.nbits, b1);
        if (hi > lo) acc |= knz_splice_piece_bits(pc, lo - pc.dst_bit, (uint32_t)(hi - lo)) >> (uint32_t)(lo - b0);
    }
    return acc;
}

// One thread per 16 aligned bytes of some output's destination (the grid may be shorter than the groups: it strides ; d_dst itself is only 4-byte
// aligned: an output's first group is short). A group that lies inside one run is five source words funnel-shifted into one 16-byte store ; every
// other word is composed from its pieces (a 1-byte block's frame is shorter than a word: three pieces and more meet in one). An output's last word
// is filled with zeros. Every store lies in the words the plan kernel has checked against the output's dst_cap.
__global__ __launch_bounds__(256) void knz_splice_copy_kernel(SpliceArgs a) {
    const uint64_t total = a.base[a.O];
    uint32_t own = 0;                                                     // the output of the thread's last group: a long output keeps it over the turns
    uint64_t own_lo = 0, own_hi = 0;                                      // ... and its groups [own_lo, own_hi)
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (uint64_t)gridDim.x * 256) {
        if (g >= own_hi) {
            uint32_t lo = 0, hi = a.O;                                    // invariant: base[lo] <= g < base[hi] (outputs without groups share their successor's base)
            while (hi - lo > 1) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (a.base[mid] <= g) lo = mid; else hi = mid;
            }
            own = lo; own_lo = a.base[lo]; own_hi = a.base[lo + 1];
        }
        const SpliceOut& o = a.outs[own];
        const SplicePiece* pcs = a.pieces + o.part_first + 2 * (uint64_t)own;
        const uint32_t P = o.n_parts + 2;
        uint32_t* dst = (uint32_t*)o.dst;
        const uint64_t nwords = (((o.total_bits + 7) >> 3) + 3) >> 2;
        const uint64_t lead = (o.dst & 15) >> 2, q = (g - own_lo) * 4;
        const uint64_t w0 = q >= lead ? q - lead : 0, w1 = min(q - lead + 4, nwords);               // (q == 0: 4 - lead words)
        const uint32_t p0 = knz_splice_piece_at(pcs, P, w0 << 5);
        const SplicePiece& pc = pcs[p0];
        if (w1 - w0 == 4 && pc.kind == KNZ_SP_RUN && (w1 << 5) <= pc.dst_bit + pc.nbits) {
            const uint32_t* words = (const uint32_t*)pc.src;
            const uint64_t s = pc.src_bit + ((w0 << 5) - pc.dst_bit);
            const uint32_t r = (uint32_t)s & 31;
            const KnzWords4 v = *(const KnzWords4*)(words + (s >> 5));
            const uint32_t x0 = knz_bswap32(v.a), x1 = knz_bswap32(v.b), x2 = knz_bswap32(v.c), x3 = knz_bswap32(v.d);
            const uint32_t x4 = r ? knz_bswap32(words[(s >> 5) + 4]) : 0;                             // (r != 0: the group's last bit lies in that word)
            uint4 v4;
            v4.x = knz_bswap32(r ? (x0 << r) | (x1 >> (32 - r)) : x0); v4.y = knz_bswap32(r ? (x1 << r) | (x2 >> (32 - r)) : x1);
            v4.z = knz_bswap32(r ? (x2 << r) | (x3 >> (32 - r)) : x2); v4.w = knz_bswap32(r ? (x3 << r) | (x4 >> (32 - r)) : x3);
            *(uint4*)(dst + w0) = v4;
            continue;
        }
        uint32_t p = p0;
        for (uint64_t w = w0; w < w1; w++) {
            while (p + 1 < P && pcs[p + 1].dst_bit <= (w << 5)) p++;
            dst[w] = knz_bswap32(knz_splice_compose(pcs, P, w, p));
        }
    }
}
