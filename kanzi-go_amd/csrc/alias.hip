// PACK and DNA transforms (ids 18 and 19) of kanzi bitstream v6 on gfx950: the reference's AliasCodec (v2/transform/AliasCodec.go:74-292,
// 297-436). A block with at least 240 unused byte values is bit-packed (one symbol: 6 bytes; up to 4 symbols: 4 per byte; up to 16: 2 per
// byte); otherwise the n0 most frequent byte pairs are replaced by the n0 byte values the block does not use. DNA is the same codec that
// declines whatever is not DNA text (ctx["packOnlyDNA"]).
//
// Nothing here is a chain. Forward, per group of blocks:
//   knz_alias_hist0_kernel    order-0 histogram, one workgroup per 8 KiB segment, LDS counters joined with one global add per value in use
//   knz_alias_plan_kernel     the declines, absent[], DetectSimpleType (written to ctx["dataType"] even when the stage declines, :128-138),
//                             the mode; headers of the packed modes
//   knz_alias_hist1_kernel    the 65536-bin pair histogram. 256 KiB of counters do not fit LDS: a workgroup owns 64 first-byte values
//                             (64 KiB of LDS counters) and a 1 MiB stretch of the block, reads the stretch, counts the pairs whose first byte
//                             is its own and adds the bins in use to the block's table. Four workgroups read every stretch; the table sees one
//                             add per (workgroup, bin in use) instead of one per position.
//   knz_alias_select_kernel   n1, the n0 largest keys freq << 16 | pair (radix select, 6 digit passes over the table, then the chosen keys
//                             are ranked among themselves), header, the savings rule
//   knz_alias_pack_kernel     payload of the packed modes (map + gather)
//   knz_alias_parse_kernel    the greedy parse `srcIdx += alias >> 8` without the chain. With a[i] = "the pair at i has an alias", a position
//                             is a token start iff its distance to the position behind the last a == 0 in front of it is even: inside a
//                             run of a == 1 the starts are the even offsets, and a position with a == 0 is always followed by a start. So a
//                             segment needs one number from the segments in front of it (the last position with a == 0), and only its
//                             positions up to its own first a == 0 depend on it: the count pass keeps (first zero, last zero, starts behind
//                             the first zero), knz_alias_offsets_kernel turns them into every segment's carry and output offset (wave scans,
//                             max and sum), and the write pass scatters through LDS. The last byte of the block is a position with a == 0.
// Inverse: header kernel (every check the reference makes plus the ones Go gets from its bounds checks: a damaged block ends in
// KNZ_ERR_PROCESS_BLOCK, never in an access outside its regions), then output lengths (1 or 2) per segment, offsets, scatter; the packed
// modes are a table expansion, the one-symbol mode a fill.
#include "bits.h"

#define KNZ_ALIAS_MIN_BLOCK 1024
#define KNZ_ALIAS_STATE_WORDS 512                 // per block: 16 scalars | 256 words (histogram / inverse map) | absent[256] | map8[256]
#define KNZ_ALIAS_SLICES 4                        // first-byte slices of the pair histogram (64 rows of 256 counters = 64 KiB of LDS each)
#define KNZ_ALIAS_H1_CHUNK (1u << 20)             // positions per workgroup of the pair histogram
#define KNZ_ALIAS_H1_THREADS 1024
enum { KNZ_AL_MODE = 0, KNZ_AL_N0 = 1, KNZ_AL_HDR = 2, KNZ_AL_TOTAL = 3, KNZ_AL_SRC0 = 4, KNZ_AL_SRCEND = 5, KNZ_AL_ADJ = 6, KNZ_AL_VAL = 7,
       KNZ_AL_F0 = 16, KNZ_AL_ABSENT = 272, KNZ_AL_MAP8 = 336 };
// modes (forward): 0 declined / nothing to do, 1 one symbol (done by the plan kernel), 2 four symbols per byte, 3 two symbols per byte,
// 4 digram (histogram and selection pending), 5 digram (header written, parse pending), 6 digram (offsets known, write pending)
// modes (inverse): 0 failed / nothing to do, 1 fill, 2 / 3 packed, 4 digram (lengths pending), 5 digram (write pending)

struct AliasArgs : XfIo {
    uint8_t* blk_dt;             // [nblocks] ctx["dataType"], may be null (= undefined, not recorded)
    uint32_t* state;             // [nblocks * KNZ_ALIAS_STATE_WORDS], zeroed by the host
    uint32_t* f1;                // [nblocks << 16] pair histogram, zeroed by the host (forward)
    uint32_t* seg;               // [nblocks * segs_per_block * 4]: first zero + 1 | last zero + 1 (then the carry) | count | offset
    uint32_t only_dna;           // the DNA transform
    uint32_t h1_chunks;          // stretches of KNZ_ALIAS_H1_CHUNK positions per block (grid of the pair histogram)
};

// the checks in front of any work (:83-109)
__device__ __forceinline__ bool knz_alias_fwd_wanted(const AliasArgs& a, uint32_t b, uint32_t count) {
    const uint32_t dt = a.blk_dt ? a.blk_dt[b] : (uint32_t)KNZ_DT_UNDEFINED;
    if (count < KNZ_ALIAS_MIN_BLOCK || (uint64_t)a.out_cap < (uint64_t)count + 1024) return false;
    if (dt == KNZ_DT_MULTIMEDIA || dt == KNZ_DT_UTF8 || dt == KNZ_DT_EXE || dt == KNZ_DT_BIN) return false;
    if (a.only_dna && dt != KNZ_DT_UNDEFINED && dt != KNZ_DT_DNA) return false;
    return true;
}

// exclusive sum / max over the 256 threads of a workgroup (s_w: 4 words of LDS); `total` = the value over all threads
__device__ __forceinline__ uint32_t knz_alias_wg_scan_add(uint32_t v, uint32_t* s_w, uint32_t& total) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t incl = wave_scan_incl(v);
    __syncthreads();
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (int k = 0; k < 4; k++) { const uint32_t w = s_w[k]; base += k < wave ? w : 0u; tot += w; }
    total = tot;
    return base + incl - v;
}
__device__ __forceinline__ uint32_t knz_alias_wave_scan_max(uint32_t v) {
    const int lane = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = wave_shfl(v, lane - d); if (lane >= d) v = t > v ? t : v; }
    return v;
}
__device__ __forceinline__ uint32_t knz_alias_wg_scan_max_excl(uint32_t v, uint32_t* s_w) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t incl = knz_alias_wave_scan_max(v);
    __syncthreads();
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t r = wave_shfl(incl, lane - 1);
    if (lane == 0) r = 0;
    for (int k = 0; k < 4; k++) { const uint32_t w = s_w[k]; if (k < wave && w > r) r = w; }
    return r;
}

// 32 consecutive bytes of a block for one thread (p0 .. p0 + 31, bytes behind `count` read 0) and the byte behind them
struct AliasChunk { uint32_t w[8]; uint32_t next; };
__device__ __forceinline__ uint32_t knz_alias_byte(const AliasChunk& c, int k) { return k < 32 ? (c.w[k >> 2] >> (8 * (k & 3))) & 0xFFu : c.next; }
__device__ __forceinline__ AliasChunk knz_alias_load_chunk(const uint8_t* src, uint32_t p0, uint32_t count) {
    AliasChunk c;
    if (p0 + 32 <= count) {
        const KnzPacked128* v = (const KnzPacked128*)(src + p0);
        const KnzPacked128 x = v[0], y = v[1];
        c.w[0] = x.x; c.w[1] = x.y; c.w[2] = x.z; c.w[3] = x.w; c.w[4] = y.x; c.w[5] = y.y; c.w[6] = y.z; c.w[7] = y.w;
    } else {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            uint32_t w = 0;
#pragma unroll
            for (int r = 0; r < 4; r++) { const uint32_t p = p0 + 4 * q + r; if (p < count) w |= (uint32_t)src[p] << (8 * r); }
            c.w[q] = w;
        }
    }
    c.next = p0 + 32 < count ? src[p0 + 32] : 0u;
    return c;
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void knz_alias_hist0_kernel(AliasArgs a) {
    __shared__ uint32_t s_h[4][256];
    const uint32_t b = blockIdx.y, s = blockIdx.x;
    const int tid = threadIdx.x;
    if (!a.active[b]) return;
    const uint32_t count = a.in_len[b], lo = s * KNZ_SEG;
    if (lo >= count || !knz_alias_fwd_wanted(a, b, count)) return;
    const uint8_t* src = (const uint8_t*)a.in_ptr[b];
    for (int k = 0; k < 4; k++) s_h[k][tid] = 0;
    __syncthreads();
    knz_histogram_256t(src + lo, min(count - lo, (uint32_t)KNZ_SEG), s_h, tid);
    __syncthreads();
    const uint32_t c = s_h[0][tid] + s_h[1][tid] + s_h[2][tid] + s_h[3][tid];
    if (c) atomicAdd(&a.state[(size_t)b * KNZ_ALIAS_STATE_WORDS + KNZ_AL_F0 + tid], c);
}

__global__ __launch_bounds__(256) void knz_alias_plan_kernel(AliasArgs a) {
    __shared__ uint32_t s_f[256];
    const uint32_t b = blockIdx.x;
    const int tid = threadIdx.x;
    if (!a.active[b]) return;
    const uint32_t count = a.in_len[b];
    uint32_t* st = a.state + (size_t)b * KNZ_ALIAS_STATE_WORDS;
    if (count == 0) { if (tid == 0) { a.ok[b] = 1; a.out_len[b] = 0; } return; }          // Forward of nothing: (0, 0, nil)
    if (!knz_alias_fwd_wanted(a, b, count)) { if (tid == 0) { a.ok[b] = 0; a.out_len[b] = 0; } return; }
    s_f[tid] = st[KNZ_AL_F0 + tid];
    __syncthreads();
    if (tid != 0) return;
    a.ok[b] = 0; a.out_len[b] = 0;
    const uint8_t* src = (const uint8_t*)a.in_ptr[b];
    uint8_t* dst = (uint8_t*)a.out_ptr[b];
    uint8_t* absent = (uint8_t*)(st + KNZ_AL_ABSENT);
    uint8_t* map8 = (uint8_t*)(st + KNZ_AL_MAP8);
    uint32_t n0 = 0;
    for (int i = 0; i < 256; i++) if (s_f[i] == 0) absent[n0++] = (uint8_t)i;
    if (n0 < 16) return;                                                                    // :124-126, before the type detection
    uint32_t dt = a.blk_dt ? a.blk_dt[b] : (uint32_t)KNZ_DT_UNDEFINED;
    if (dt == KNZ_DT_UNDEFINED) {                                                           // :128-138
        dt = (uint32_t)knz_detect_simple_type((int)count, s_f);
        if (a.blk_dt && dt != KNZ_DT_UNDEFINED) a.blk_dt[b] = (uint8_t)dt;                  // stays whatever the stage does next
        if (dt != KNZ_DT_DNA && a.only_dna) return;
    }
    if (n0 < 240) { st[KNZ_AL_N0] = n0; st[KNZ_AL_MODE] = 4; return; }                      // digram coding
    dst[0] = (uint8_t)n0;
    if (n0 == 255) {                                                                        // one symbol
        dst[1] = src[0];
        dst[2] = (uint8_t)count; dst[3] = (uint8_t)(count >> 8); dst[4] = (uint8_t)(count >> 16); dst[5] = (uint8_t)(count >> 24);
        st[KNZ_AL_MODE] = 1;
        a.ok[b] = 1; a.out_len[b] = 6;
        return;
    }
    uint32_t dstIdx = 1, j = 0;
    for (int i = 0; i < 256; i++) if (s_f[i] != 0) { dst[dstIdx++] = (uint8_t)i; map8[i] = (uint8_t)j++; }
    uint32_t adj, total;
    if (n0 >= 252) {                                                                        // 4 symbols or less
        adj = count & 3;
        dst[dstIdx++] = (uint8_t)adj;
        for (uint32_t k = 0; k < adj; k++) dst[dstIdx++] = src[k];
        total = dstIdx + ((count - adj) >> 2);
    } else {                                                                                // 16 symbols or less
        adj = count & 1;
        dst[dstIdx++] = (uint8_t)adj;
        if (adj) dst[dstIdx++] = src[0];
        total = dstIdx + (count >> 1);
    }
    if (total >= count) return;                                                             // :287-289
    st[KNZ_AL_HDR] = dstIdx; st[KNZ_AL_ADJ] = adj; st[KNZ_AL_MODE] = n0 >= 252 ? 2 : 3;
    a.ok[b] = 1; a.out_len[b] = total;
}

// ComputeHistogram(src, freqs1, false, false) (internal/Global.go:304-341): every position is counted with the byte in front of it, the
// first one with 0. grid (KNZ_ALIAS_SLICES * h1_chunks, blocks)
__global__ __launch_bounds__(KNZ_ALIAS_H1_THREADS) void knz_alias_hist1_kernel(AliasArgs a) {
    __shared__ uint32_t s_h[(256 / KNZ_ALIAS_SLICES) * 256];
    const uint32_t b = blockIdx.y, slice = blockIdx.x % KNZ_ALIAS_SLICES, chunk = blockIdx.x / KNZ_ALIAS_SLICES;
    const uint32_t tid = threadIdx.x;
    if (!a.active[b]) return;
    const uint32_t* st = a.state + (size_t)b * KNZ_ALIAS_STATE_WORDS;
    if (st[KNZ_AL_MODE] != 4) return;
    const uint32_t count = a.in_len[b], lo = chunk * KNZ_ALIAS_H1_CHUNK;
    if (lo >= count) return;
    const uint32_t hi = min(count, lo + KNZ_ALIAS_H1_CHUNK);
    const uint8_t* src = (const uint8_t*)a.in_ptr[b];
    const uint32_t rows = 256 / KNZ_ALIAS_SLICES, row0 = slice * rows;
    for (uint32_t i = tid; i < rows * 256; i += KNZ_ALIAS_H1_THREADS) s_h[i] = 0;
    __syncthreads();
    for (uint32_t p0 = lo + 16 * tid; p0 < hi; p0 += 16 * KNZ_ALIAS_H1_THREADS) {
        uint32_t prv = p0 ? src[p0 - 1] : 0u;
        if (p0 + 16 <= hi) {
            const KnzPacked128 x = *(const KnzPacked128*)(src + p0);
            const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const uint32_t cur = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                if (prv - row0 < rows) atomicAdd(&s_h[((prv - row0) << 8) | cur], 1u);
                prv = cur;
            }
        } else {
            for (uint32_t p = p0; p < hi; p++) {
                const uint32_t cur = src[p];
                if (prv - row0 < rows) atomicAdd(&s_h[((prv - row0) << 8) | cur], 1u);
                prv = cur;
            }
        }
    }
    __syncthreads();
    uint32_t* f1 = a.f1 + ((size_t)b << 16) + ((size_t)row0 << 8);
    for (uint32_t i = tid; i < rows * 256; i += KNZ_ALIAS_H1_THREADS) { const uint32_t c = s_h[i]; if (c) atomicAdd(&f1[i], c); }
}

// n1, the n0 most frequent pairs by (frequency, value) descending (:231-237: the keys freq << 16 | value are unique), header, savings
__global__ __launch_bounds__(1024) void knz_alias_select_kernel(AliasArgs a) {
    __shared__ uint32_t s_hist[256];
    __shared__ unsigned long long s_keys[256];
    __shared__ unsigned long long s_prefix;
    __shared__ uint32_t s_k, s_n1, s_cnt, s_sav;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (!a.active[b]) return;
    uint32_t* st = a.state + (size_t)b * KNZ_ALIAS_STATE_WORDS;
    if (st[KNZ_AL_MODE] != 4) return;
    const uint32_t count = a.in_len[b];
    const uint32_t* f1 = a.f1 + ((size_t)b << 16);
    uint8_t* dst = (uint8_t*)a.out_ptr[b];
    const uint8_t* absent = (const uint8_t*)(st + KNZ_AL_ABSENT);
    if (tid == 0) { s_n1 = 0; s_cnt = 0; s_sav = 0; s_prefix = 0; }
    __syncthreads();
    {
        uint32_t c = 0;
        for (uint32_t i = tid; i < 65536; i += 1024) c += f1[i] != 0 ? 1u : 0u;
        c = wave_reduce_add(c);
        if ((tid & 63) == 0) atomicAdd(&s_n1, c);
    }
    __syncthreads();
    const uint32_t n0 = min(st[KNZ_AL_N0], s_n1);                                           // :221-228
    if (n0 < 16) { if (tid == 0) st[KNZ_AL_MODE] = 0; return; }
    if (tid == 0) s_k = n0;
    for (int shift = 40; shift >= 0; shift -= 8) {                                          // the n0-th largest key, a digit per pass (freq < 2^31: 47 bits)
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
        const unsigned long long prefix = s_prefix;
        for (uint32_t i = tid; i < 65536; i += 1024) {
            const uint32_t f = f1[i];
            const unsigned long long key = ((unsigned long long)f << 16) | i;
            if (f != 0 && (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_hist[(uint32_t)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t acc = 0, k = s_k;
            for (int d = 255; d >= 0; d--) {
                const uint32_t c = s_hist[d];
                if (acc + c >= k) { s_prefix = prefix | ((unsigned long long)d << shift); s_k = k - acc; break; }
                acc += c;
            }
        }
        __syncthreads();
    }
    const unsigned long long thr = s_prefix;
    for (uint32_t i = tid; i < 65536; i += 1024) {
        const uint32_t f = f1[i];
        const unsigned long long key = ((unsigned long long)f << 16) | i;
        if (f != 0 && key >= thr) { const uint32_t at = atomicAdd(&s_cnt, 1u); if (at < 256) s_keys[at] = key; }
    }
    __syncthreads();
    if (tid < n0) {
        const unsigned long long key = s_keys[tid];
        uint32_t r = 0;
        for (uint32_t j = 0; j < n0; j++) r += s_keys[j] > key ? 1u : 0u;
        uint8_t* m = dst + 2 + 3 * r;                                                       // :253-261
        m[0] = (uint8_t)(key >> 8); m[1] = (uint8_t)key; m[2] = absent[r];
        atomicAdd(&s_sav, (uint32_t)(key >> 16));
    }
    __syncthreads();
    if (tid != 0) return;
    dst[0] = (uint8_t)n0; dst[1] = 0;
    if (s_sav < count / 20) { st[KNZ_AL_MODE] = 0; return; }                                // :264-266
    st[KNZ_AL_N0] = n0; st[KNZ_AL_HDR] = 2 + 3 * n0; st[KNZ_AL_MODE] = 5;
}

// payload of the packed modes: grid (segments of 8192 OUTPUT bytes, blocks)
__global__ __launch_bounds__(256) void knz_alias_pack_kernel(AliasArgs a) {
    __shared__ uint8_t s_map[256];
    const uint32_t b = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
    if (!a.active[b]) return;
    const uint32_t* st = a.state + (size_t)b * KNZ_ALIAS_STATE_WORDS;
    const uint32_t mode = st[KNZ_AL_MODE];
    if (mode != 2 && mode != 3) return;
    const uint32_t count = a.in_len[b], adj = st[KNZ_AL_ADJ], hdr = st[KNZ_AL_HDR];
    const uint32_t np = mode == 2 ? (count - adj) >> 2 : (count - adj) >> 1;
    const uint32_t lo = s * KNZ_SEG;
    if (lo >= np) return;
    const uint32_t hi = min(np, lo + KNZ_SEG);
    const uint8_t* src = (const uint8_t*)a.in_ptr[b] + adj;
    uint8_t* dst = (uint8_t*)a.out_ptr[b] + hdr;
    s_map[tid] = ((const uint8_t*)(st + KNZ_AL_MAP8))[tid];
    __syncthreads();
    for (uint32_t j = lo + tid; j < hi; j += 256) {
        if (mode == 2) {
            const uint32_t w = knz_vle32(src + 4 * (size_t)j);
            dst[j] = (uint8_t)((s_map[w & 255] << 6) | (s_map[(w >> 8) & 255] << 4) | (s_map[(w >> 16) & 255] << 2) | s_map[w >> 24]);
        } else {
            const uint8_t* p = src + 2 * (size_t)j;
            dst[j] = (uint8_t)((s_map[p[0]] << 4) | s_map[p[1]]);
        }
    }
}

// The pairs that have an alias, for one workgroup: a 65536-bit map, the number of set bits in front of every word and the aliases in the
// order of the pairs' values (at most 239). Read back from the header the selection has written.
struct AliasLut { uint32_t* bits; uint8_t* pre; uint8_t* alias; };
__device__ __forceinline__ void knz_alias_build_lut(const AliasLut& l, const uint8_t* hdr, uint32_t n0, uint32_t* s_w) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < 2048; i += 256) l.bits[i] = 0;
    __syncthreads();
    uint32_t pair = 0;
    if (tid < n0) { pair = ((uint32_t)hdr[2 + 3 * tid] << 8) | hdr[3 + 3 * tid]; atomicOr(&l.bits[pair >> 5], 1u << (pair & 31)); }
    __syncthreads();
    uint32_t c = 0;
    for (int k = 0; k < 8; k++) c += (uint32_t)__popc(l.bits[8 * tid + k]);
    uint32_t total;
    uint32_t run = knz_alias_wg_scan_add(c, s_w, total);
    for (int k = 0; k < 8; k++) { l.pre[8 * tid + k] = (uint8_t)run; run += (uint32_t)__popc(l.bits[8 * tid + k]); }
    __syncthreads();
    if (tid < n0) l.alias[l.pre[pair >> 5] + (uint32_t)__popc(l.bits[pair >> 5] & ((1u << (pair & 31)) - 1u))] = hdr[4 + 3 * tid];
    __syncthreads();
}

// WRITE == false: per segment first / last position with a == 0 (+ 1; 0 = none) and the token starts behind the first one.
// WRITE == true: the tokens, from the carry and the offset knz_alias_offsets_kernel has worked out.
template <bool WRITE>
__global__ __launch_bounds__(256) void knz_alias_parse_kernel(AliasArgs a) {
    __shared__ uint32_t s_bits[2048];
    __shared__ uint8_t s_pre[2048];
    __shared__ uint8_t s_alias[256];
    __shared__ uint8_t s_out[WRITE ? KNZ_SEG : 16];
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_fz, s_lz;
    const uint32_t b = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
    if (!a.active[b]) return;
    const uint32_t* st = a.state + (size_t)b * KNZ_ALIAS_STATE_WORDS;
    if (st[KNZ_AL_MODE] != (WRITE ? 6u : 5u)) return;
    const uint32_t count = a.in_len[b], lo = s * KNZ_SEG;
    if (lo >= count) return;
    const uint32_t n0 = st[KNZ_AL_N0], hdr = st[KNZ_AL_HDR];
    const uint8_t* src = (const uint8_t*)a.in_ptr[b];
    uint8_t* dst = (uint8_t*)a.out_ptr[b];
    uint32_t* seg = a.seg + ((size_t)b * a.segs_per_block + s) * 4;
    AliasLut lut; lut.bits = s_bits; lut.pre = s_pre; lut.alias = s_alias;
    knz_alias_build_lut(lut, dst, n0, s_w);
    if (tid == 0) { s_fz = 0xFFFFFFFFu; s_lz = 0; }
    const uint32_t p0 = lo + 32 * tid;
    uint32_t amask = 0, ob[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t myFirst = 0xFFFFFFFFu, myLast = 0;                                             // positions + 1 with a == 0 in my 32
    if (p0 < count) {
        const AliasChunk c = knz_alias_load_chunk(src, p0, count);
#pragma unroll
        for (int k = 0; k < 32; k++) {
            const uint32_t pos = p0 + k, x = knz_alias_byte(c, k);
            uint32_t o = x;
            if (pos + 1 < count) {                                                          // srcEnd = count - 1: the last byte pairs with nothing
                const uint32_t idx = (x << 8) | knz_alias_byte(c, k + 1);
                const uint32_t w = s_bits[idx >> 5], bit = 1u << (idx & 31);
                if (w & bit) { amask |= 1u << k; o = s_alias[s_pre[idx >> 5] + (uint32_t)__popc(w & (bit - 1u))]; }
            }
            ob[k >> 2] |= o << (8 * (k & 3));
        }
        const uint32_t nv = min(32u, count - p0);
        const uint32_t zeros = ~amask & (nv == 32 ? 0xFFFFFFFFu : ((1u << nv) - 1u));
        if (zeros) { myFirst = p0 + (uint32_t)__builtin_ctz(zeros) + 1; myLast = p0 + (31u - (uint32_t)__builtin_clz(zeros)) + 1; }
    }
    __syncthreads();
    if (myLast) { atomicMin(&s_fz, myFirst); atomicMax(&s_lz, myLast); }
    uint32_t lz1 = knz_alias_wg_scan_max_excl(myLast, s_w);                                 // last zero + 1 in front of my 32, inside the segment
    __syncthreads();
    const uint32_t fz1 = s_fz == 0xFFFFFFFFu ? 0u : s_fz;
    // a position is a start iff (pos - (last zero in front of it + 1)) is even. Without the carry the segment's start stands in for it:
    // right behind the segment's first zero, which is all the count pass keeps.
    const uint32_t carry1 = WRITE ? seg[1] : lo;
    if (carry1 > lz1) lz1 = carry1;
    uint32_t starts = 0, cnt = 0;
    if (p0 < count) {
        const uint32_t nv = min(32u, count - p0);
        for (uint32_t k = 0; k < nv; k++) {
            const uint32_t pos = p0 + k;
            if (((pos - lz1) & 1u) == 0) { starts |= 1u << k; if (WRITE || (fz1 && pos >= fz1)) cnt++; }
            if (!((amask >> k) & 1u)) lz1 = pos + 1;
        }
    }
    uint32_t total;
    const uint32_t at = knz_alias_wg_scan_add(cnt, s_w, total);
    if (!WRITE) {
        if (tid == 0) { seg[0] = fz1; seg[1] = s_lz; seg[2] = total; }
        return;
    }
    if (p0 < count) {
        uint32_t o = at;
        const uint32_t nv = min(32u, count - p0);
        for (uint32_t k = 0; k < nv; k++)
            if ((starts >> k) & 1u) s_out[o++] = (uint8_t)(ob[k >> 2] >> (8 * (k & 3)));
        if (p0 + nv == count && ((starts >> (nv - 1)) & 1u)) dst[1] = 1;                    // the last byte stands alone (:278-283)
    }
    __syncthreads();
    uint8_t* o = dst + hdr + seg[3];
    for (uint32_t i = tid; i < total; i += 256) o[i] = s_out[i];
}

// per block: every segment's carry (last zero + 1 in front of it) and output offset; the final decline (:287-289)
__global__ __launch_bounds__(64) void knz_alias_offsets_kernel(AliasArgs a) {
    const uint32_t b = blockIdx.x;
    const int lane = threadIdx.x;
    if (!a.active[b]) return;
    uint32_t* st = a.state + (size_t)b * KNZ_ALIAS_STATE_WORDS;
    if (st[KNZ_AL_MODE] != 5) return;
    const uint32_t count = a.in_len[b], nseg = (count + KNZ_SEG - 1) / KNZ_SEG;
    uint32_t carry1 = 0, off = 0;                                                           // (position -1 counts as a zero: position 0 is a start)
    for (uint32_t base = 0; base < nseg; base += 64) {
        const uint32_t s = base + (uint32_t)lane;
        const bool valid = s < nseg;
        uint32_t* seg = a.seg + ((size_t)b * a.segs_per_block + s) * 4;
        const uint32_t fz1 = valid ? seg[0] : 0u, lzSeg = valid ? seg[1] : 0u, fixed = valid ? seg[2] : 0u;
        const uint32_t incl = knz_alias_wave_scan_max(lzSeg);
        uint32_t cin = wave_shfl(incl, lane - 1);                                           // last zero + 1 in front of my segment
        if (lane == 0) cin = 0;
        if (carry1 > cin) cin = carry1;
        uint32_t cnt = 0;
        if (valid) {
            const uint32_t lo = s * KNZ_SEG, hi = min(count, lo + KNZ_SEG);
            const uint32_t last = fz1 ? fz1 - 1 : hi - 1;                                   // positions lo .. last (up to the first zero) follow the carry
            const uint32_t first = lo + ((lo - cin) & 1u);
            if (first <= last) cnt = (last - first) / 2 + 1;
            cnt += fixed;
            seg[1] = cin; seg[3] = 0;
        }
        const uint32_t inclS = wave_scan_incl(cnt);
        if (valid) seg[3] = off + inclS - cnt;
        off += wave_bcast(inclS, 63);
        const uint32_t m = wave_bcast(incl, 63);
        if (m > carry1) carry1 = m;
    }
    if (lane != 0) return;
    const uint32_t total = st[KNZ_AL_HDR] + off;
    if (total >= count) { st[KNZ_AL_MODE] = 0; return; }
    st[KNZ_AL_MODE] = 6;
    a.ok[b] = 1; a.out_len[b] = total;
}

// ---- inverse -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void knz_alias_inv_header_kernel(AliasArgs a) {
    const uint32_t b = blockIdx.x;
    const int lane = threadIdx.x;
    if (!a.active[b]) return;
    const uint64_t count = a.in_len[b], cap = a.out_cap;
    uint32_t* st = a.state + (size_t)b * KNZ_ALIAS_STATE_WORDS;
    const uint8_t* src = (const uint8_t*)a.in_ptr[b];
    uint8_t* dst = (uint8_t*)a.out_ptr[b];
    if (count == 0) { if (lane == 0) { a.ok[b] = 1; a.out_len[b] = 0; } return; }
    const uint32_t n = count >= 2 ? src[0] : 0u;
    if (n >= 16 && n < 240 && 2 + 3 * (uint64_t)n <= count)                                 // alias -> symbol (:407-413)
        for (int i = lane; i < 256; i += 64) st[KNZ_AL_F0 + i] = 0x10000u | (uint32_t)i;
    wave_sync();
    __threadfence();
    if (lane != 0) return;
    a.ok[b] = -KNZ_ERR_PROCESS_BLOCK; a.out_len[b] = 0;                                      // until the header has passed
    if (count < 2 || n < 16) return;                                                        // :302-314
    if (count > (uint64_t)a.segs_per_block * KNZ_SEG) return;                               // (more input than the output region holds bytes)
    if (n >= 240) {
        const uint32_t ns = 256 - n;
        if (ns == 1) {                                                                      // one symbol
            if (count < 6) return;
            const uint32_t oSize = (uint32_t)src[2] | ((uint32_t)src[3] << 8) | ((uint32_t)src[4] << 16) | ((uint32_t)src[5] << 24);
            if ((uint64_t)oSize > cap) return;                                              // :329-331
            st[KNZ_AL_VAL] = src[1]; st[KNZ_AL_TOTAL] = oSize; st[KNZ_AL_MODE] = 1;
            a.ok[b] = 1; a.out_len[b] = oSize;
            return;
        }
        if (2 + (uint64_t)ns > count) return;                                               // symbols and the adjust byte
        uint8_t* sym = (uint8_t*)(st + KNZ_AL_MAP8);
        for (uint32_t i = 0; i < 16; i++) sym[i] = i < ns ? src[1 + i] : 0;
        const uint32_t adjust = src[1 + ns];
        if (adjust > 3) return;                                                             // :351-353
        const uint64_t src0 = 2 + (uint64_t)ns;
        uint64_t raw, total;
        if (ns <= 4) { raw = adjust; if (src0 + raw > count) return; total = raw + 4 * (count - src0 - raw); }
        else { raw = adjust ? 1 : 0; if (src0 + raw > count) return; total = raw + 2 * (count - src0 - raw); }
        if (total > cap) return;
        for (uint64_t k = 0; k < raw; k++) dst[k] = src[src0 + k];
        st[KNZ_AL_SRC0] = (uint32_t)(src0 + raw); st[KNZ_AL_ADJ] = (uint32_t)raw; st[KNZ_AL_TOTAL] = (uint32_t)total; st[KNZ_AL_MODE] = ns <= 4 ? 2 : 3;
        a.ok[b] = 1; a.out_len[b] = (uint32_t)total;
        return;
    }
    const uint64_t src0 = 2 + 3 * (uint64_t)n;
    if (src0 > count) return;
    for (uint32_t i = 0; i < n; i++) {                                                      // in the header's order: a later entry replaces an earlier one (:415-418)
        const uint8_t* m = src + 2 + 3 * i;
        st[KNZ_AL_F0 + m[2]] = 0x20000u | m[0] | ((uint32_t)m[1] << 8);
    }
    const uint64_t tail = src[1];
    uint64_t end = count >= tail ? count - tail : 0;                                        // srcEnd = len(src) - src[1]; the loop leaves srcIdx at max(start, srcEnd)
    if (end < src0) end = src0;
    if (tail != 0 && end >= count) return;                                                  // src[srcIdx] behind the input (:428-432)
    st[KNZ_AL_SRC0] = (uint32_t)src0; st[KNZ_AL_SRCEND] = (uint32_t)end; st[KNZ_AL_ADJ] = tail != 0 ? 1u : 0u; st[KNZ_AL_MODE] = 4;
}

// WRITE == false: output bytes of every segment of 8192 aliases. WRITE == true: the bytes, and the fill / table expansion of the other modes
template <bool WRITE>
__global__ __launch_bounds__(256) void knz_alias_inv_seg_kernel(AliasArgs a) {
    __shared__ uint32_t s_map[256];
    __shared__ uint8_t s_out[WRITE ? 2 * KNZ_SEG : 16];
    __shared__ uint32_t s_w[4];
    const uint32_t b = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
    if (!a.active[b]) return;
    const uint32_t* st = a.state + (size_t)b * KNZ_ALIAS_STATE_WORDS;
    const uint32_t mode = st[KNZ_AL_MODE];
    const uint8_t* src = (const uint8_t*)a.in_ptr[b];
    uint8_t* dst = (uint8_t*)a.out_ptr[b];
    if (WRITE && mode == 1) {                                                               // one symbol: segments of the output
        const uint32_t oSize = st[KNZ_AL_TOTAL], lo = s * KNZ_SEG, val = st[KNZ_AL_VAL];
        for (uint32_t i = lo + tid; i < min(oSize, lo + KNZ_SEG); i += 256) dst[i] = (uint8_t)val;
        return;
    }
    if (WRITE && (mode == 2 || mode == 3)) {                                                // packed: segments of the payload
        const uint32_t src0 = st[KNZ_AL_SRC0], raw = st[KNZ_AL_ADJ], np = a.in_len[b] - src0, lo = s * KNZ_SEG;
        if (lo >= np) return;
        const uint8_t* sym = (const uint8_t*)(st + KNZ_AL_MAP8);
        if (mode == 2) s_map[tid] = (uint32_t)sym[(tid >> 6) & 3] | ((uint32_t)sym[(tid >> 4) & 3] << 8) | ((uint32_t)sym[(tid >> 2) & 3] << 16) | ((uint32_t)sym[tid & 3] << 24);
        else s_map[tid] = (uint32_t)sym[tid >> 4] | ((uint32_t)sym[tid & 15] << 8);
        __syncthreads();
        const uint32_t hi = min(np, lo + KNZ_SEG);
        for (uint32_t j = lo + tid; j < hi; j += 256) {
            const uint32_t v = s_map[src[src0 + j]];
            if (mode == 2) ((KnzPacked32*)(dst + raw + 4 * (size_t)j))->v = v;
            else { uint8_t* o = dst + raw + 2 * (size_t)j; o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); }
        }
        return;
    }
    if (mode != (WRITE ? 5u : 4u)) return;
    const uint32_t src0 = st[KNZ_AL_SRC0], end = st[KNZ_AL_SRCEND];
    const uint32_t lo = src0 + s * KNZ_SEG;
    if (lo >= end || lo < src0) return;
    uint32_t* seg = a.seg + ((size_t)b * a.segs_per_block + s) * 4;
    s_map[tid] = st[KNZ_AL_F0 + tid];
    __syncthreads();
    const uint32_t p0 = lo + 32 * tid, segEnd = min(end, lo + KNZ_SEG);
    uint32_t two = 0, len = 0;                                                               // my 32 aliases: which ones stand for two bytes
    AliasChunk c;
    for (int k = 0; k < 8; k++) c.w[k] = 0;
    c.next = 0;
    if (p0 < segEnd) {
        c = knz_alias_load_chunk(src, p0, segEnd);
        const uint32_t nv = min(32u, segEnd - p0);
#pragma unroll
        for (int k = 0; k < 32; k++)
            if ((uint32_t)k < nv) { const uint32_t v = s_map[knz_alias_byte(c, k)]; if (v & 0x20000u) two |= 1u << k; }
        len = nv + (uint32_t)__popc(two);
    }
    uint32_t total;
    const uint32_t at = knz_alias_wg_scan_add(len, s_w, total);
    if (!WRITE) { if (tid == 0) seg[2] = total; return; }
    if (p0 < segEnd) {
        const uint32_t nv = min(32u, segEnd - p0);
        uint32_t o = at;
#pragma unroll
        for (int k = 0; k < 32; k++)
            if ((uint32_t)k < nv) {
                const uint32_t v = s_map[knz_alias_byte(c, k)];
                s_out[o++] = (uint8_t)v;
                if (v & 0x20000u) s_out[o++] = (uint8_t)(v >> 8);
            }
    }
    __syncthreads();
    uint8_t* o = dst + seg[3];
    for (uint32_t i = tid; i < total; i += 256) o[i] = s_out[i];
}

__global__ __launch_bounds__(64) void knz_alias_inv_offsets_kernel(AliasArgs a) {
    const uint32_t b = blockIdx.x;
    const int lane = threadIdx.x;
    if (!a.active[b]) return;
    uint32_t* st = a.state + (size_t)b * KNZ_ALIAS_STATE_WORDS;
    if (st[KNZ_AL_MODE] != 4) return;
    const uint32_t src0 = st[KNZ_AL_SRC0], end = st[KNZ_AL_SRCEND], nseg = (end - src0 + KNZ_SEG - 1) / KNZ_SEG;
    const uint8_t* src = (const uint8_t*)a.in_ptr[b];
    uint8_t* dst = (uint8_t*)a.out_ptr[b];
    uint64_t off = 0;
    for (uint32_t base = 0; base < nseg; base += 64) {
        const uint32_t s = base + (uint32_t)lane;
        uint32_t* seg = a.seg + ((size_t)b * a.segs_per_block + s) * 4;
        const uint32_t cnt = s < nseg ? seg[2] : 0u;
        const uint32_t incl = wave_scan_incl(cnt);
        if (s < nseg) seg[3] = (uint32_t)(off + incl - cnt);                                // (only read when the total fits the region)
        off += wave_bcast(incl, 63);
    }
    if (lane != 0) return;
    // Go's bounds checks: every alias stores dst[dstIdx] and dst[dstIdx + 1] (:423-425), the lone last byte dst[dstIdx] (:428-432)
    const uint64_t cap = a.out_cap, tail = st[KNZ_AL_ADJ];
    bool bad = false;
    if (end > src0) { const uint64_t lastLen = st[KNZ_AL_F0 + src[end - 1]] >> 16; bad = off - lastLen + 2 > cap; }
    if (tail && off >= cap) bad = true;
    if (bad) { st[KNZ_AL_MODE] = 0; return; }                                               // (ok stays at -KNZ_ERR_PROCESS_BLOCK)
    if (tail) dst[off] = src[end];
    st[KNZ_AL_MODE] = 5;
    a.ok[b] = 1; a.out_len[b] = (uint32_t)(off + tail);
}
