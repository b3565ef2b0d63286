// Pattern search in .knz streams (knz_dev_find_many, host side in knz_find.inc): Q queries (source, window, byte string) -> the decoded offsets at which
// the string starts. The blocks a query's extended read (offset, length + pattern_len - 1) covers are decoded once by the many-streams batch, as
// for the byte reads (read.hip: one ReadEntry per distinct (source, block), the decoded block at stage + blk * stride). The decoded bytes stay there:
// the kernels below are the batch's tail for this call, and only offsets leave the workspace.
//   knz_find_plan_kernel (one wave per query: status, ext, scanned, tiles of candidate start positions) -> knz_read_scan_kernel (the tiles' scan) ->
//   knz_find_match_kernel (one workgroup per tile, its query found by binary search over the scan: one long window and thousands of short ones fill
//   the machine alike ; leaves a bitmap of the tile's matches and their number) -> knz_read_scan_kernel (the scan of those numbers over all tiles: a
//   query's tiles are neighbours, so its hits in front of a tile are a difference of two entries) -> knz_find_finish_kernel (n_hits) ->
//   knz_find_fill_kernel (one workgroup per tile: the set bits become offsets, in ascending order, below hits_cap).
// Nothing here is atomic: the same input gives the same words in d_hits on every run.
#include "bits.h"
#include "wave.h"

#define KNZ_FIND_TILE 4096           // candidate start positions one workgroup of the match kernel takes (KNZ_FIND_TILE, tests: fewer, a multiple of 256)
#define KNZ_FIND_THREADS 256
#define KNZ_FIND_LDS_BYTES (KNZ_FIND_TILE + KNZ_FIND_MAX_PATTERN + 32)     // a tile, pattern_len - 1 bytes behind it, and what shares their first and last 16-byte chunk

struct FindRow {                     // one row per query: the host fills the inputs, the kernels the rest
    uint64_t hits, cap;              // the caller's d_hits and hits_cap
    uint64_t offset, length;         // the window, its length clamped to the source's blocks
    uint64_t n_hits, scanned;        // results
    uint64_t ext;                    // plan: bytes the extended read delivers
    uint32_t first, count;           // its entries: the blocks offset / block_size + 1 .. of its source
    uint32_t off0;                   // offset % block_size
    uint32_t pat, pat_len;           // the pattern: bytes pats[pat .. pat + pat_len)
    int32_t status;                  // in: refused by the host ; out: 0 or the code of the first failing block of the extended read's window
};

struct FindArgs {
    ReadArgs rd;                     // ent, blk_len, blk_status, block_size, stage, stride ; R = the queries, base = [R + 1] the scan of their tiles
    FindRow* rows;
    const uint8_t* pats;
    uint32_t tile;                   // start positions a tile, a multiple of 256, <= KNZ_FIND_TILE
    uint32_t max_tiles;              // rows of cnt and of bits: no query list comes to more tiles (the host's bound)
    uint64_t* cnt;                   // [max_tiles + 1] match: the tiles' hits ; scan: their exclusive scan, cnt[max_tiles] their sum
    uint64_t* bits;                  // [max_tiles][tile / 64] bit p % 64 of word p / 64: the pattern starts at the tile's position p
};

// start positions of a query: k < scanned with k + pattern_len <= ext
__device__ __forceinline__ uint64_t knz_find_positions(const FindRow& r) {
    return r.ext >= r.pat_len ? min(r.scanned, r.ext - r.pat_len + 1) : 0;
}

// One wave per query. ext as knz_read_finish computes `out` for the extended read, with one difference: the entries end at the source's last block
// (there is no entry for a block that does not exist), so a window whose blocks are all full ends with them.
__global__ __launch_bounds__(256) void knz_find_plan_kernel(FindArgs a) {
    const uint32_t q = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (q >= a.rd.R) return;                                              // (whole waves leave)
    FindRow& r = a.rows[q];
    int32_t fail = r.status;
    uint64_t ext = 0;
    if (fail == 0 && r.count != 0) {
        uint32_t stop, stop_len;
        knz_read_window_wave(a.rd, r.first, r.count, lane, fail, stop, stop_len);
        if (fail == 0) {
            const uint64_t avail = (uint64_t)stop * a.rd.block_size + stop_len;       // (stop == count: every block full, stop_len 0)
            ext = avail > r.off0 ? min(r.length + r.pat_len - 1, avail - r.off0) : 0;
        }
    }
    if (lane != 0) return;
    r.status = fail; r.ext = ext; r.scanned = min(r.length, ext); r.n_hits = 0;
    a.rd.base[q] = (knz_find_positions(r) + a.tile - 1) / a.tile;
}

// the query that owns tile t: base[q] <= t < base[q + 1] (queries without tiles share their successor's base)
__device__ __forceinline__ uint32_t knz_find_owner(const FindArgs& a, uint64_t t) {
    uint32_t lo = 0, hi = a.rd.R;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a.rd.base[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// One workgroup per tile (the grid may be shorter than the tiles: it strides). The tile's start positions and the pattern_len - 1 bytes behind them come
// into LDS as the aligned 16-byte chunks that hold them: byte g of the query's blocks laid end to end is byte g % block_size of entry g / block_size,
// the block size is a multiple of 16 and every block's slot is 64-byte aligned, so a chunk never straddles two blocks. Position p of the tile is
// thread p % 256 in turn p / 256: a wave's ballot is word p / 64 of the tile's bitmap.
__global__ __launch_bounds__(KNZ_FIND_THREADS) void knz_find_match_kernel(FindArgs a) {
    __shared__ uint4 s_q[KNZ_FIND_LDS_BYTES / 16];
    __shared__ uint8_t s_pat[KNZ_FIND_MAX_PATTERN];
    __shared__ uint32_t s_wcnt[KNZ_FIND_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t bs = a.rd.block_size, wpt = a.tile >> 6;
    const uint64_t total = min(a.rd.base[a.rd.R], (uint64_t)a.max_tiles);
    const uint32_t* s32 = (const uint32_t*)s_q;
    const uint8_t* s8 = (const uint8_t*)s_q;
    for (uint64_t t = blockIdx.x; t < total; t += gridDim.x) {
        const uint32_t q = knz_find_owner(a, t);
        const FindRow& r = a.rows[q];
        const uint32_t pl = r.pat_len;
        const uint64_t k0 = (t - a.rd.base[q]) * a.tile, kend = min(k0 + a.tile, knz_find_positions(r));      // the tile's positions [k0, kend) of the window
        const uint64_t g0 = r.off0 + k0;
        const uint32_t a0 = (uint32_t)g0 & 15;                            // the first position's place in its chunk
        const uint32_t nchunks = (a0 + (uint32_t)(kend - k0) + pl - 1 + 15) >> 4;       // (<= KNZ_FIND_LDS_BYTES / 16: a0 <= 15, the positions <= the tile, pl <= 256)
        const uint64_t j0 = (g0 - a0) / bs;
        const uint32_t w0 = (uint32_t)((g0 - a0) % bs);
        for (uint32_t c = tid; c < nchunks; c += KNZ_FIND_THREADS) {
            const uint32_t rel = w0 + (c << 4);                           // (< 2^30 + 2^13)
            const uint8_t* src = a.rd.stage + (uint64_t)a.rd.ent[r.first + j0 + rel / bs].blk * a.rd.stride + rel % bs;
            s_q[c] = *(const uint4*)src;
        }
        if (tid < pl) s_pat[tid] = a.pats[r.pat + tid];
        __syncthreads();
        const uint32_t fl = min(pl, 4u);
        uint32_t first4 = 0;
        for (uint32_t m = 0; m < fl; m++) first4 |= (uint32_t)s_pat[m] << (8 * m);
        const uint32_t mask = fl == 4 ? 0xFFFFFFFFu : (1u << (8 * fl)) - 1;
        uint32_t cnt = 0;
        for (uint32_t i = 0; i < a.tile / KNZ_FIND_THREADS; i++) {
            const uint32_t p = i * KNZ_FIND_THREADS + tid, b = a0 + p;
            const uint32_t v = (uint32_t)((((uint64_t)s32[(b >> 2) + 1] << 32) | s32[b >> 2]) >> ((b & 3) * 8));      // the four bytes from position p on
            bool hit = k0 + p < kend && ((v ^ first4) & mask) == 0;
            for (uint32_t m = 4; m < pl && hit; m++) hit = s8[b + m] == s_pat[m];
            const uint64_t word = wave_ballot(hit);
            if (lane == 0) a.bits[t * wpt + i * 4 + wave] = word;
            cnt += (uint32_t)__builtin_popcountll(word);
        }
        if (lane == 0) s_wcnt[wave] = cnt;
        __syncthreads();
        if (tid == 0) a.cnt[t] = (uint64_t)s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
        __syncthreads();                                                  // (the next tile's chunks go where this one's are still read)
    }
}

// per query: its hits are those of its tiles, neighbours in the scan
__global__ __launch_bounds__(256) void knz_find_finish_kernel(FindArgs a) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= a.rd.R) return;
    const uint64_t lo = min(a.rd.base[q], (uint64_t)a.max_tiles), hi = min(a.rd.base[q + 1], (uint64_t)a.max_tiles);
    a.rows[q].n_hits = a.cnt[hi] - a.cnt[lo];
}

// One workgroup per tile with hits to write: hit number h of the query (h = the hits of the query's tiles in front + the set bits of the tile in
// front) goes to d_hits[h] where h < hits_cap, as one 8-byte store. Words in front of a wave's word: their popcounts scanned by wave 0, through LDS.
__global__ __launch_bounds__(KNZ_FIND_THREADS) void knz_find_fill_kernel(FindArgs a) {
    __shared__ uint32_t s_pre[KNZ_FIND_TILE / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t wpt = a.tile >> 6;
    const uint64_t total = min(a.rd.base[a.rd.R], (uint64_t)a.max_tiles);
    for (uint64_t t = blockIdx.x; t < total; t += gridDim.x) {
        const uint32_t q = knz_find_owner(a, t);
        const FindRow& r = a.rows[q];
        const uint64_t tb = a.cnt[t] - a.cnt[a.rd.base[q]];               // the query's hits in front of this tile
        if (a.cnt[t + 1] == a.cnt[t] || tb >= r.cap) continue;            // (the same for the whole workgroup)
        if (wave == 0) {
            const uint32_t c = lane < wpt ? (uint32_t)__builtin_popcountll(a.bits[t * wpt + lane]) : 0;
            const uint32_t incl = wave_scan_incl(c);
            if (lane < wpt) s_pre[lane] = incl - c;
        }
        __syncthreads();
        uint64_t* hits = (uint64_t*)r.hits;
        const uint64_t at0 = r.offset + (t - a.rd.base[q]) * a.tile;      // decoded offset of the tile's first position
        for (uint32_t w = wave; w < wpt; w += KNZ_FIND_THREADS / 64) {
            const uint64_t word = a.bits[t * wpt + w];
            const uint64_t h = tb + s_pre[w] + wave_mbcnt64(word);
            if (((word >> lane) & 1) != 0 && h < r.cap) hits[h] = at0 + (w << 6) + lane;
        }
        __syncthreads();                                                  // (s_pre is the next tile's too)
    }
}
