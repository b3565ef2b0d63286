// libknz_gpu: C ABI (include/knz_gpu.h) + GPU batch scheduler. Unity build of the gfx950 kernels.
// Product code: gfx950 only, no CPU fallback (knz_open fails without a GPU).
#include "knz_internal.h"
#include "huffman_enc.hip"
#include "huffman_dec.hip"
#include "huffman_par.hip"
#include "ans0.hip"
#include "ans1.hip"
#include "fpaq.hip"
#include "transforms.hip"
#include "rank_inv.hip"
#include "rank_pipe.hip"
#include "bwt.hip"
#include "lz.hip"
#include "lz_par.hip"
#include "lz_inv_par.hip"
#include "lz_fwd_seg.hip"
#include "srt_lzp.hip"
#include "text.hip"
#include "text_par.hip"
#include "utf.hip"
#include "alias.hip"
#include "xxhash.hip"
#include "skip.hip"
#include "prims.h"
#include "bwt_sort.hip"
#include "layout.hip"
#include "many.hip"
#include "read.hip"
#include "find.hip"
#include "write.hip"
#include "write_streams.hip"
#include "splice.hip"
#include <algorithm>
#include <cstdio>
#include <cstring>

#define HIP_OK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess) return knz_set_error(h, KNZ_ERR_UNKNOWN, hipGetErrorString(e__)); \
    } while (0)

static int probe_begin(Handle* h, hipStream_t st, const char* name) {
    if (h->nprobes >= KNZ_MAX_PROBES) return -1;
    KernelProbe& p = h->probes[h->nprobes];
    if (!p.a && (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess)) return -1;
    p.name = name;
    hipEventRecord(p.a, st);
    return h->nprobes++;
}
static void probe_end(Handle* h, hipStream_t st, int id) { if (id >= 0) hipEventRecord(h->probes[id].b, st); }
// launch with a probe: `h` and `st` are in scope at every call site
#define KNZ_LAUNCH_PROBED(kern, ...)                         \
    do {                                                      \
        const int pid__ = probe_begin(h, st, #kern);          \
        hipLaunchKernelGGL(kern, __VA_ARGS__);                \
        probe_end(h, st, pid__);                              \
    } while (0)

// HIP's current device is a per-host-thread setting: every entry point binds the calling thread to the handle's device for the
// duration of the call (a handle opened on device N may be used from any goroutine / OS thread) and restores what was there.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(const Handle* h) {
        if (h && hipGetDevice(&prev) == hipSuccess && prev != h->device) switched = hipSetDevice(h->device) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// the stream a call runs on: the caller's or else the handle's own for device pointers ; the handle's non-blocking one, where it exists, for host pointers
static hipStream_t dev_call_stream(const Handle* h, void* hip_stream) { return hip_stream ? (hipStream_t)hip_stream : h->stream; }
static hipStream_t host_call_stream(const Handle* h) { return h->hstream ? h->hstream : h->stream; }

// several lanes behind one handle (knz_multi.inc)
static int multi_blocks(Handle* h, knz_block* blocks, int n, int job);
static void multi_close(Handle* h);
static Handle* lane0(Handle* h);
static Handle* lane_of_pointer(Handle* h, const void* d_ptr);

int knz_set_error(Handle* h, int code, const char* msg) {
    if (h) h->err = msg ? msg : "";
    return code;
}

// A workspace growth of 64 MiB or more is refused while it would leave the device with less than 1/16 of its memory (4 GiB at least): a device driven to its
// last byte takes the HIP runtime down with it (queue creation aborts the process), and several handles share one device. A refused
// growth comes back as KNZ_ERR_CREATE_COMPRESSOR / _DECOMPRESSOR; the host-pointer entry points then release the workspace and take the
// batch in halves (knz_host_api.inc). KNZ_TEST_ALLOC_LIMIT (tests): bytes one buffer may hold.
static thread_local std::vector<DevBuf*>* g_buf_registry = nullptr;
static thread_local bool g_alloc_refused = false;
DevBuf::DevBuf() { if (g_buf_registry) g_buf_registry->push_back(this); }
int DevBuf::reserve(size_t n) {
    if (n <= cap) return 0;
    // (every check comes before the old buffer is given back: a refused growth leaves the handle as it was)
    const size_t want = n + n / 8 + 256;
    if (const char* lim = knz_test_switch("KNZ_TEST_ALLOC_LIMIT")) { if (want > (size_t)strtoull(lim, nullptr, 10)) { g_alloc_refused = true; return -1; } }
    size_t freeB = 0, totalB = 0;
    if (want - cap >= ((size_t)64 << 20) && hipMemGetInfo(&freeB, &totalB) == hipSuccess && totalB != 0) {   // the headroom rule is for growths that matter (>= 64 MiB)
        const size_t keep = std::min(std::max<size_t>(totalB / 16, (size_t)4 << 30), totalB / 2);
        const size_t avail = freeB + cap;                 // (the old buffer goes first)
        if (want > avail || avail - want < keep) { g_alloc_refused = true; return -1; }
    }
    if (p) hipFree(p);
    p = nullptr; cap = 0;
    if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; (void)hipGetLastError(); g_alloc_refused = true; return -1; }
    cap = want;
    return 0;
}
void DevBuf::release() { if (p) hipFree(p); p = nullptr; cap = 0; }
static void knz_release_workspace(Handle* h) {
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->hstream) hipStreamSynchronize(h->hstream);
    if (h->pipe_ready) { hipStreamSynchronize(h->stream2); hipStreamSynchronize(h->stream3); }
    for (DevBuf* b : h->all_bufs) b->release();
    h->text_stat_ready = false;                      // (the static TEXT dictionary lives in one of them: uploaded again on demand)
    h->huf_fallback_n = 0; h->lzs_n = 0; h->lzi_serial_n = 0; h->pipe_n = 0;
}

// The HIP runtime multiplexes all streams of a process onto GPU_MAX_HW_QUEUES hardware queues (4 by default), and kernels of streams that share
// a queue run one after the other. A Go host keeps one handle per io.Writer / io.Reader (two streams each: the caller's and the fused ZRLT / RANK
// chain's), so four queues serialise everything beyond two handles (measured: profiles/r05_multi_handle.json). The variable is read when the
// runtime initialises: set here, when the library is loaded, unless the host has chosen a value (no effect if HIP is already up).
#ifndef KNZ_HIP_EMU
__attribute__((constructor)) static void knz_more_hw_queues() { setenv("GPU_MAX_HW_QUEUES", "32", 0); }
#endif

// ---- stream header, v2/io/CompressedStream.go:429-519 -----------------------------------------------------------
static void hdr_put(uint32_t* words, uint32_t& pos, uint64_t value, uint32_t count) {
    for (int i = (int)count - 1; i >= 0; i--) {      // host side, a couple of hundred bits: bit by bit is fine
        uint32_t bit = (uint32_t)((value >> i) & 1);
        words[pos >> 5] |= bit << (31 - (pos & 31));
        pos++;
    }
}
uint32_t knz_build_stream_header(const knz_cfg& cfg, int64_t inputSize, uint32_t words[8]) {
    for (int i = 0; i < 8; i++) words[i] = 0;
    uint32_t pos = 0;
    const int ckSize = cfg.checksum_bits == 32 ? 1 : (cfg.checksum_bits == 64 ? 2 : 0);
    hdr_put(words, pos, 0x4B414E5Au, 32);              // _BITSTREAM_TYPE
    hdr_put(words, pos, 6, 4);                         // _BITSTREAM_FORMAT_VERSION
    hdr_put(words, pos, (uint64_t)ckSize, 2);
    hdr_put(words, pos, cfg.entropy, 5);
    hdr_put(words, pos, cfg.transform, 48);
    hdr_put(words, pos, cfg.block_size >> 4, 28);
    uint32_t szMask;
    if (inputSize <= 0 || inputSize >= ((int64_t)1 << 48)) szMask = 0;
    else if (inputSize >= ((int64_t)1 << 32)) szMask = 3;
    else if (inputSize >= ((int64_t)1 << 16)) szMask = 2;
    else szMask = 1;
    hdr_put(words, pos, szMask, 2);
    if (szMask) hdr_put(words, pos, (uint64_t)inputSize, 16 * szMask);
    hdr_put(words, pos, 0, 15);
    const uint32_t HASH = 0x1E35A7BDu;
    uint32_t ck = HASH * (0x01030507u * 6u);
    ck ^= HASH * (uint32_t)(~(uint32_t)ckSize);
    ck ^= HASH * (uint32_t)(~cfg.entropy);
    ck ^= HASH * (uint32_t)((~cfg.transform) >> 32);
    ck ^= HASH * (uint32_t)(~cfg.transform);
    ck ^= HASH * (uint32_t)(~cfg.block_size);
    if (szMask) {
        ck ^= HASH * (uint32_t)((~(uint64_t)inputSize) >> 32);
        ck ^= HASH * (uint32_t)(~(uint64_t)inputSize);
    }
    ck = (ck >> 23) ^ (ck >> 3);
    hdr_put(words, pos, ck & 0xFFFFFF, 24);
    return pos;
}

// ---- open / close --------------------------------------------------------------------------------------------------
static thread_local std::string g_open_error;

extern "C" int knz_open(const knz_cfg* cfg, void** handle) {
    if (!cfg || !handle) return KNZ_ERR_MISSING_PARAM;
    *handle = nullptr;
    g_open_error.clear();
    if (cfg->block_size < 1024 || cfg->block_size > (1u << 30) || (cfg->block_size & 15)) { g_open_error = "invalid block size"; return KNZ_ERR_BLOCK_SIZE; }
    if (cfg->checksum_bits != 0 && cfg->checksum_bits != 32 && cfg->checksum_bits != 64) { g_open_error = "invalid checksum size"; return KNZ_ERR_INVALID_PARAM; }
    if (cfg->bs_version != 0 && cfg->bs_version != 6) { g_open_error = "only bitstream version 6"; return KNZ_ERR_STREAM_VERSION; }
    std::vector<DevBuf*> bufs;
    g_buf_registry = &bufs;
    Handle* h = new Handle();
    g_buf_registry = nullptr;
    h->all_bufs = bufs;
    h->cfg = *cfg;
    h->cfg.bs_version = 6;
    int dev = cfg->device;
    hipError_t e = hipSuccess;
    if (dev < 0) { e = hipGetDevice(&dev); if (e != hipSuccess) dev = 0; }
    e = hipSetDevice(dev);
    if (e != hipSuccess) { g_open_error = std::string("hipSetDevice: ") + hipGetErrorString(e); delete h; return KNZ_ERR_CREATE_COMPRESSOR; }
    h->device = dev;
    void* probe = nullptr;
    e = hipMalloc(&probe, 256);                      // no usable GPU: fail loudly, there is no CPU fallback
    if (e != hipSuccess) { g_open_error = std::string("hipMalloc: ") + hipGetErrorString(e); delete h; return KNZ_ERR_CREATE_COMPRESSOR; }
    hipFree(probe);
    e = hipHostMalloc(&h->pinned, 4096);
    if (e != hipSuccess) { g_open_error = std::string("hipHostMalloc: ") + hipGetErrorString(e); delete h; return KNZ_ERR_CREATE_COMPRESSOR; }
    // the handle's own stream: a blocking stream, i.e. ordered against the null stream (callers that prepare buffers on the
    // default stream, PyTorch included, need no extra synchronisation) but not against the streams of other handles
    if (hipStreamCreateWithFlags(&h->stream, hipStreamDefault) == hipSuccess) h->own_stream = true;
    else h->stream = nullptr;
    // ... and one for the host-pointer entry points (knz_encode_blocks, knz_decode_blocks, the single-object calls): every buffer of the caller is host
    // memory there, so nothing has to be ordered against the NULL stream of whatever else lives in the process
    if (hipStreamCreateWithFlags(&h->hstream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); h->hstream = nullptr; }
    for (int i = 0; i <= KNZ_STAGE_COUNT; i++) hipEventCreate(&h->ev[i]);
    // The two streams of the fused ZRLT / RANK chain (rank_pipe.hip) get priorities of their own: the runtime keeps a pool of hardware queues per priority
    // level, so the long chains (stream3, highest), the short ones (stream2, lowest) and the caller's stream (the decoder under which they start) can never
    // share a hardware queue. At one priority the runtime deals its few queues out in turn to every stream the PROCESS creates: where two of the three landed
    // on one queue the kernels ran one after the other (a decode of configs[3] in 833 ms instead of 525, seen with the handle's own stream in a torch process).
    {
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); least = greatest = 0; }
        const bool s2 = (least != greatest && hipStreamCreateWithPriority(&h->stream2, hipStreamNonBlocking, least) == hipSuccess) ||
                        ((void)hipGetLastError(), hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking) == hipSuccess);
        const bool s3 = (least != greatest && hipStreamCreateWithPriority(&h->stream3, hipStreamNonBlocking, greatest) == hipSuccess) ||
                        ((void)hipGetLastError(), hipStreamCreateWithFlags(&h->stream3, hipStreamNonBlocking) == hipSuccess);
        h->pipe_ready = s2 && s3;
    }
    for (int i = 0; i < 3; i++) if (hipEventCreateWithFlags(&h->ev_pipe[i], hipEventDisableTiming) != hipSuccess) h->pipe_ready = false;
    for (int i = 0; i < KNZ_STAGE_COUNT; i++) h->stage_ms[i] = 0.f;
    *handle = h;
    return KNZ_OK;
}

extern "C" int knz_close(void* handle) {
    Handle* h = (Handle*)handle;
    if (!h) return KNZ_OK;
    if (h->multi) { multi_close(h); delete h; return KNZ_OK; }
    DeviceGuard dg(h);                                  // (the workspace buffers are freed by ~Handle while the device is bound)
    if (h->own_stream) { hipStreamSynchronize(h->stream); hipStreamDestroy(h->stream); h->stream = nullptr; h->own_stream = false; }
    if (h->pinned) hipHostFree(h->pinned);
    if (h->hstream && h->hstream != h->stream) { hipStreamSynchronize(h->hstream); hipStreamDestroy(h->hstream); }
    h->hstream = nullptr;
    for (int i = 0; i <= KNZ_STAGE_COUNT; i++) hipEventDestroy(h->ev[i]);
    if (h->pipe_ready) { hipStreamSynchronize(h->stream2); hipStreamDestroy(h->stream2); h->stream2 = nullptr; hipStreamSynchronize(h->stream3); hipStreamDestroy(h->stream3); h->stream3 = nullptr; }
    for (int i = 0; i < 3; i++) if (h->ev_pipe[i]) { hipEventDestroy(h->ev_pipe[i]); h->ev_pipe[i] = nullptr; }
    for (int i = 0; i < KNZ_MAX_PROBES; i++) if (h->probes[i].a) { hipEventDestroy(h->probes[i].a); hipEventDestroy(h->probes[i].b); }
    delete h;
    return KNZ_OK;
}

extern "C" const char* knz_last_error(void* handle) { return handle ? ((Handle*)handle)->err.c_str() : g_open_error.c_str(); }

static int multi_last_timing(Handle* h, float* stage_ms, int cap);
static int multi_last_counter(Handle* h, int id, uint64_t* value);

extern "C" int knz_last_timing(void* handle, float* stage_ms, int cap) {
    Handle* h = (Handle*)handle;
    if (!h || !stage_ms) return 0;
    if (h->multi) return multi_last_timing(h, stage_ms, cap);
    DeviceGuard dg(h);
    if (h->ev_valid) {
        hipEventSynchronize(h->ev[KNZ_STAGE_COUNT]);
        for (int i = 0; i < KNZ_STAGE_COUNT; i++) hipEventElapsedTime(&h->stage_ms[i], h->ev[i], h->ev[i + 1]);
    }
    int n = std::min(cap, (int)KNZ_STAGE_COUNT);
    for (int i = 0; i < n; i++) stage_ms[i] = h->stage_ms[i];
    return n;
}

extern "C" int knz_last_kernel_times(void* handle, char* names, int names_cap, float* ms, int cap) {
    Handle* h = lane0((Handle*)handle);                  // (several lanes: the launches of the first one)
    if (!h || !names || !ms || names_cap <= 0) return 0;
    DeviceGuard dg(h);
    int n = 0, pos = 0;
    names[0] = 0;
    for (int i = 0; i < h->nprobes && n < cap; i++) {
        const KernelProbe& p = h->probes[i];
        const int len = (int)strlen(p.name);
        if (pos + len + 2 > names_cap) break;
        if (hipEventSynchronize(p.b) != hipSuccess || hipEventElapsedTime(&ms[n], p.a, p.b) != hipSuccess) ms[n] = 0.f;
        memcpy(names + pos, p.name, len); pos += len; names[pos++] = '\n'; names[pos] = 0;
        n++;
    }
    return n;
}

// the first n flag bytes of a workspace buffer, brought over: their sum, or with only != 0 the number of them that have this value
static int sum_flags(const DevBuf& buf, size_t n, uint8_t only, uint64_t* value) {
    *value = 0;
    if (n == 0) return KNZ_OK;
    std::vector<uint8_t> f(n);
    if (hipMemcpy(f.data(), buf.p, f.size(), hipMemcpyDeviceToHost) != hipSuccess) return KNZ_ERR_UNKNOWN;
    for (uint8_t v : f) *value += only ? (v == only ? 1 : 0) : v;
    return KNZ_OK;
}

extern "C" int knz_last_counter(void* handle, int id, uint64_t* value) {
    Handle* h = (Handle*)handle;
    if (!h || !value || id < KNZ_COUNTER_HUF_SERIAL_CHUNKS || id > KNZ_COUNTER_ENCODE_BATCH_BLOCKS) return KNZ_ERR_INVALID_PARAM;
    if (h->multi) return multi_last_counter(h, id, value);
    DeviceGuard dg(h);
    *value = 0;
    if (id == KNZ_COUNTER_POST_TRANSFORM_BYTES) { *value = h->post_bytes; return KNZ_OK; }
    if (id == KNZ_COUNTER_DECODE_BATCH_BLOCKS) { *value = h->dec_blocks; return KNZ_OK; }
    if (id == KNZ_COUNTER_ENCODE_BATCH_BLOCKS) { *value = h->enc_blocks; return KNZ_OK; }
    if (id >= KNZ_COUNTER_STAGE_BYTES0) { *value = h->stage_bytes[id - KNZ_COUNTER_STAGE_BYTES0]; return KNZ_OK; }
    if (id == KNZ_COUNTER_TEXT_CHAIN_BLOCKS) {
        uint32_t v = 0;
        if (h->text_cnt.p && hipMemcpy(&v, h->text_cnt.p, 4, hipMemcpyDeviceToHost) != hipSuccess) return KNZ_ERR_UNKNOWN;
        *value = v;
        return KNZ_OK;
    }
    if (id == KNZ_COUNTER_LZ_FWD_ROUNDS) { *value = h->lzs_rounds; return KNZ_OK; }
    if (id == KNZ_COUNTER_RANK_PIPE_BLOCKS) return sum_flags(h->pipe_flag, h->pipe_n, 0, value);
    if (id == KNZ_COUNTER_LZ_FWD_SERIAL_BLOCKS) return sum_flags(h->lzs_misc, h->lzs_n, 2, value);
    if (id == KNZ_COUNTER_LZ_INV_SERIAL_BLOCKS) return sum_flags(h->lzi_serial, h->lzi_serial_n, 0, value);
    return sum_flags(h->huf_fallback, h->huf_fallback_n, 0, value);
}

#ifdef KNZ_PROFILE_PHASES
extern "C" int knz_debug_prof(unsigned long long* out, int reset) {
    if (out) hipMemcpyFromSymbol(out, HIP_SYMBOL(g_knz_prof), sizeof(unsigned long long) * 32);
    if (reset) { unsigned long long z[32] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(g_knz_prof), z, sizeof(z)); }
    return 0;
}
#endif

#include "knz_transforms.inc"
#include "knz_batch.inc"

// ---- capabilities: the transforms are the rows of kXfCodecs (knz_transforms.inc), the entropy codecs those of kEntropyCodecs (knz_batch.inc) ----
extern "C" int knz_supports(uint64_t transform, uint32_t entropy) {
    for (int s = 42; s >= 0; s -= 6) if (!xf_codec((uint32_t)((transform >> s) & 63))) return 0;
    return entropy_on_device(entropy) ? 1 : 0;
}

extern "C" uint32_t knz_max_encoded_len(uint64_t transform, uint32_t n) {     // Sequence.go:189-205
    uint64_t req = n;
    for (int s = 42; s >= 0; s -= 6)
        if (const XfCodec* c = xf_codec((uint32_t)((transform >> s) & 63))) req += (c->grow_div && req > 1024) ? req / c->grow_div : c->grow;
    return (uint32_t)std::min<uint64_t>(req, 0xFFFFFFFFu);
}

// the two device-resident encode calls: `out` takes the bytes of a whole stream, or the bits of a segment
static int dev_encode(void* handle, EncodeBatch eb, uint64_t* out, bool bytes, void* hip_stream) {
    Handle* h = lane_of_pointer((Handle*)handle, eb.d_dst);
    if (!h || !eb.d_dst || !out || (!eb.d_src && eb.n)) return KNZ_ERR_MISSING_PARAM;
    DeviceGuard dg(h);
    if (((uintptr_t)eb.d_dst & 3) || ((uintptr_t)eb.d_src & 15)) return knz_set_error(h, KNZ_ERR_INVALID_PARAM, "d_src must be 16-byte and d_dst 4-byte aligned");
    int rc = encode_batch(h, eb, dev_call_stream(h, hip_stream));
    if (rc) return rc;
    *out = bytes ? (eb.total_bits + 7) >> 3 : eb.total_bits;
    return KNZ_OK;
}

extern "C" int knz_dev_compress(void* handle, const void* d_src, uint64_t n, int64_t header_input_size, void* d_dst,
                                uint64_t dst_cap, uint64_t* out_bytes, void* hip_stream) {
    return dev_encode(handle, EncodeBatch::stream((const uint8_t*)d_src, n, (uint8_t*)d_dst, dst_cap, header_input_size), out_bytes, true, hip_stream);
}

extern "C" int knz_dev_compress_blocks(void* handle, const void* d_src, uint64_t n, void* d_dst, uint64_t dst_cap,
                                       uint64_t* out_bits, void* hip_stream) {
    return dev_encode(handle, EncodeBatch::segment((const uint8_t*)d_src, n, (uint8_t*)d_dst, dst_cap), out_bits, false, hip_stream);
}

#include "knz_host_api.inc"
#include "knz_multi.inc"
#include "knz_many.inc"
#include "knz_read.inc"
#include "knz_find.inc"
#include "knz_write.inc"
#include "knz_write_streams.inc"
#include "knz_splice.inc"
