// Byte reads from .knz streams (knz_dev_read_many, host side in knz_read.inc): K triples (source, byte offset, length) and K destinations of any
// alignment. The covering blocks are decoded once by the many-streams batch (one entry per distinct (source, block), knz_many.inc) and sit in the
// staging buffer at a fixed stride; the kernels below replace knz_many_place_plan_kernel / knz_many_place_copy_kernel for this call:
//   knz_read_plan_kernel (per read: status, bytes delivered, 16-byte destination chunks) -> knz_read_scan_kernel (exclusive scan of the chunk
//   counts) -> knz_read_gather_kernel (one thread per destination chunk, its read found by binary search over the scan: many short reads and one
//   long read fill the machine alike).
// A read owns exactly the bytes d_dst[0 .. out): chunks inside them are one aligned 16-byte store, the ragged head and tail are byte stores, so
// that destinations of different reads may follow each other to the byte. Source and destination disagree mod 16 as a rule: the source comes in
// as aligned 32-bit words and is shifted into place.
#include "bits.h"
#include "wave.h"

#define KNZ_READ_NO_BLOCK 0xFFFFFFFFu
#define KNZ_READ_LONG 32             // a read over more entries than this gets a wave of the plan kernel, not a thread

struct ReadEntry {                   // one row per distinct (source, block) of the call, sorted: a read's blocks are consecutive rows
    uint32_t blk;                    // its row in the batch's block tables (decoded at stage + blk * stride) ; KNZ_READ_NO_BLOCK: not in the batch
    int32_t status;                  // ... because of this code (hint refused, framing in front of it damaged, block refused), or 0: no such block
};

struct ReadRow {                     // one row per read: the host fills the inputs, the plan kernel the rest
    uint64_t dst, length;            // the caller's d_dst and length
    uint64_t out;                    // result: bytes delivered
    uint32_t first, count;           // its entries: the blocks offset / block_size + 1 .. of its source
    uint32_t off0;                   // offset % block_size
    int32_t status;                  // in: refused by the host ; out: 0 or the code of the first failing block of its window
};

struct ReadArgs {
    ReadRow* reads; uint32_t R;
    const ReadEntry* ent;
    const uint32_t* blk_len;         // [nblocks] decoded bytes of every block of the batch
    const int32_t* blk_status;       // [nblocks]
    uint32_t block_size;
    const uint32_t* long_ids; uint32_t n_long;   // the reads over more than KNZ_READ_LONG entries
    uint64_t* base;                  // [R + 1] plan: the reads' chunk counts ; scan: their exclusive scan, base[R] their sum
    const uint8_t* stage; uint64_t stride;
};

// what entry e gives a read: a failure code, or 0 and the block's decoded length (0: there is no such block)
__device__ __forceinline__ int32_t knz_read_entry(const ReadArgs& a, uint32_t e, uint32_t& len) {
    const ReadEntry en = a.ent[e];
    len = 0;
    if (en.status != 0 || en.blk == KNZ_READ_NO_BLOCK) return en.status;
    const int32_t st = a.blk_status[en.blk];
    if (st != 0) return st;
    len = a.blk_len[en.blk];
    return len > a.block_size ? (int32_t)KNZ_ERR_PROCESS_BLOCK : 0;
}

// fail: code of the first failing entry of the window ; stop: the first entry that decoded to less than a block (count: none), stop_len its length.
// Every block in front of `stop` is full: the read's byte k is byte (off0 + k) % block_size of entry (off0 + k) / block_size.
// chunks: the 16-byte chunks of the destination's grid that hold dst[0 .. out) (ragged head, interior, ragged tail)
__device__ __forceinline__ void knz_read_finish(ReadRow& r, uint64_t& chunks, int32_t fail, uint32_t stop, uint32_t stop_len, uint32_t bs) {
    uint64_t out = 0;
    if (fail == 0 && r.count != 0) {
        if (stop >= r.count) out = r.length;
        else {
            const uint64_t avail = (uint64_t)stop * bs + stop_len;
            out = avail > r.off0 ? min(r.length, avail - r.off0) : 0;
        }
    }
    r.status = fail; r.out = out;
    chunks = out ? ((r.dst + out + 15) >> 4) - (r.dst >> 4) : 0;
}

// fail / stop / stop_len of the window of entries [first, first + count), taken by one whole wave (every lane calls it and gets the same answer):
// what the long reads' plan and the find calls' plan (find.hip) share
__device__ __forceinline__ void knz_read_window_wave(const ReadArgs& a, uint32_t first, uint32_t count, uint32_t lane, int32_t& fail, uint32_t& stop, uint32_t& stop_len) {
    uint32_t bad = count;                                                 // the lane's first failing / first short entry
    stop = count;
    for (uint32_t j = lane; j < count; j += 64) {
        uint32_t len;
        const int32_t st = knz_read_entry(a, first + j, len);
        if (st != 0 && bad == count) bad = j;
        if (st == 0 && len < a.block_size && stop == count) stop = j;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t b2 = wave_shfl(bad, (int)(lane ^ d)), s2 = wave_shfl(stop, (int)(lane ^ d));
        bad = min(bad, b2); stop = min(stop, s2);
    }
    fail = 0; stop_len = 0;
    uint32_t len;
    if (bad < count) fail = knz_read_entry(a, first + bad, len);
    else if (stop < count) { knz_read_entry(a, first + stop, len); stop_len = len; }
}

// wide == 0: one thread per read, reads over more than KNZ_READ_LONG entries left out ; wide == 1: one wave per read of long_ids
__global__ __launch_bounds__(256) void knz_read_plan_kernel(ReadArgs a, uint32_t wide) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (!wide) {
        if (t >= a.R) return;
        ReadRow& r = a.reads[t];
        if (r.count > KNZ_READ_LONG) return;
        if (r.status != 0) { r.out = 0; a.base[t] = 0; return; }
        int32_t fail = 0;
        uint32_t stop = r.count, stop_len = 0;
        for (uint32_t j = 0; j < r.count && fail == 0; j++) {
            uint32_t len;
            fail = knz_read_entry(a, r.first + j, len);
            if (stop == r.count && len < a.block_size) { stop = j; stop_len = len; }
        }
        knz_read_finish(r, a.base[t], fail, stop, stop_len, a.block_size);
        return;
    }
    if ((t >> 6) >= a.n_long) return;                                     // (whole waves leave)
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t id = a.long_ids[t >> 6];
    ReadRow& r = a.reads[id];
    if (r.status != 0) { if (lane == 0) { r.out = 0; a.base[id] = 0; } return; }
    int32_t fail;
    uint32_t stop, stop_len;
    knz_read_window_wave(a, r.first, r.count, lane, fail, stop, stop_len);
    if (lane != 0) return;
    knz_read_finish(r, a.base[id], fail, stop, stop_len, a.block_size);
}

// base[k] = exclusive scan of the reads' chunk counts (the plan kernel left them in base[k]), base[R] = their sum. One workgroup of 1 024 threads walks
// the table, four neighbouring rows a thread and turn.
#define KNZ_READ_SCAN_THREADS 1024
__global__ __launch_bounds__(KNZ_READ_SCAN_THREADS) void knz_read_scan_kernel(ReadArgs a) {
    __shared__ uint64_t s_wave[KNZ_READ_SCAN_THREADS / 64];
    __shared__ uint64_t s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t k0 = 0; k0 < a.R; k0 += 4 * KNZ_READ_SCAN_THREADS) {
        const uint32_t k = k0 + 4 * tid;
        uint64_t c[4];
        for (int i = 0; i < 4; i++) c[i] = k + i < a.R ? a.base[k + i] : 0;
        const uint64_t own = c[0] + c[1] + c[2] + c[3];
        uint64_t incl = own;
        for (int d = 1; d < 64; d <<= 1) { const uint64_t v = wave_shfl64(incl, lane - d); if (lane >= d) incl += v; }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint64_t before = s_carry;
        for (int w = 0; w < wave; w++) before += s_wave[w];
        uint64_t at = before + incl - own;
        for (int i = 0; i < 4; i++) { if (k + i < a.R) a.base[k + i] = at; at += c[i]; }
        __syncthreads();
        if (tid == KNZ_READ_SCAN_THREADS - 1) s_carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) a.base[a.R] = s_carry;
}

struct __attribute__((packed, aligned(4))) KnzWords4 { uint32_t a, b, c, d; };   // four words at any 4-byte aligned address
__device__ __forceinline__ uint32_t knz_read_funnel(uint32_t lo, uint32_t hi, uint32_t sh) {      // bits sh .. sh + 31 of hi:lo, sh < 32
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
}

// One thread per destination chunk (the grid may be shorter than the chunks: it strides). Every byte it stores lies in its read's dst[0 .. out).
__global__ __launch_bounds__(256) void knz_read_gather_kernel(ReadArgs a) {
    const uint64_t total = a.base[a.R];
    const uint32_t bs = a.block_size;
    uint32_t own = 0;                                                     // the read of the thread's last chunk: a long read keeps it over the turns
    uint64_t own_lo = 0, own_hi = 0;                                      // ... and its chunks [own_lo, own_hi)
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (uint64_t)gridDim.x * 256) {
        if (g >= own_hi) {
            uint32_t lo = 0, hi = a.R;                                    // invariant: base[lo] <= g < base[hi] (reads without chunks share their successor's base)
            while (hi - lo > 1) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (a.base[mid] <= g) lo = mid; else hi = mid;
            }
            own = lo; own_lo = a.base[lo]; own_hi = a.base[lo + 1];
        }
        const ReadRow& r = a.reads[own];
        const uint64_t d = r.dst, at = (d & ~(uint64_t)15) + ((g - own_lo) << 4);    // the chunk's address: bytes [k0, k1) of the read lie in it
        const uint64_t k0 = at > d ? at - d : 0, k1 = min(at + 16 - d, r.out);
        const uint64_t p = (uint64_t)r.off0 + k0;
        uint32_t j, w;                                                    // byte k0 is byte w of the read's entry j
        if ((p >> 32) == 0) { j = (uint32_t)p / bs; w = (uint32_t)p % bs; }
        else { j = (uint32_t)(p / bs); w = (uint32_t)(p % bs); }
        const uint8_t* src = a.stage + (uint64_t)a.ent[r.first + j].blk * a.stride;
        if (k1 - k0 == 16 && w + 16 <= bs) {
            // interior chunk out of one block: the 16 bytes from src + w on, fetched as the aligned words that hold them, one aligned store
            const uint32_t* q = (const uint32_t*)((uintptr_t)(src + w) & ~(uintptr_t)3);
            const uint32_t sh = (uint32_t)((uintptr_t)(src + w) & 3) * 8;
            const KnzWords4 v = *(const KnzWords4*)q;
            const uint32_t v4 = sh ? q[4] : 0;                            // (a block's slot ends inside the staging buffer: stride >= block size, 64 bytes behind the last)
            uint4 o;
            o.x = knz_read_funnel(v.a, v.b, sh); o.y = knz_read_funnel(v.b, v.c, sh); o.z = knz_read_funnel(v.c, v.d, sh); o.w = knz_read_funnel(v.d, v4, sh);
            *(uint4*)at = o;
            continue;
        }
        // ragged head or tail of the read, or a chunk across a block boundary (the next block sits at the next entry's place): byte by byte
        uint8_t* dp = (uint8_t*)(d + k0);
        for (uint64_t k = k0; k < k1; k++) {
            *dp++ = src[w];
            if (++w == bs && k + 1 < k1) { w = 0; j++; src = a.stage + (uint64_t)a.ent[r.first + j].blk * a.stride; }
        }
    }
}
