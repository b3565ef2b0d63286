/*
 * knz_gpu.h — C ABI of the MI355X-native Kanzi block-compression hot path.
 *
 * Drop-in boundary for flanglet/kanzi-go (bitstream v6). Bit-exactness is pinned by a MECHANICAL TRANSLATION of the reference, not yet by a Go-built
 * binary: the image has no Go toolchain, so kanzi-go's .go sources are translated to C++ by tools/go2cpp and compiled (oracle/_ref); the device is compared
 * with that build directly, through 387 stream vectors it wrote (tests/test_ref_streams.py), through the full-size BASELINE streams by sha256
 * (tests/golden/ref_streams/fullsize_manifest.json), and with the hand-written restatement (oracle/) that _ref pins case by case. A misreading of Go shared by
 * the translator and the restatement would pass all of that; a stream from a Go-compiled build is the missing witness (tools/make_ref_vectors.sh writes the
 * same manifests on any machine with Go). Every entry point names the reference interface it replaces; the cgo stubs a kanzi-go maintainer would add are
 * in INTEGRATION.md and go/.
 * Plain pointers and sizes only; the library never keeps a caller pointer after a call returns.
 * Return value: 0 on success, otherwise a kanzi error code (v2/Definitions.go:25-46), except
 * knz_transform_forward() which returns KNZ_SKIP when the transform declines (in kanzi-go a
 * Forward error means "skip this transform", v2/transform/Sequence.go:86-91).
 *
 * The product library (libknz_gpu.so) contains gfx950 code only. There is no CPU fallback: with no
 * usable GPU knz_open() fails with KNZ_ERR_CREATE_COMPRESSOR.
 */
#ifndef KNZ_GPU_H
#define KNZ_GPU_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* v2/Definitions.go:25-46 */
enum {
    KNZ_OK = 0,
    KNZ_ERR_MISSING_PARAM = 1, KNZ_ERR_BLOCK_SIZE = 2, KNZ_ERR_INVALID_CODEC = 3,
    KNZ_ERR_CREATE_COMPRESSOR = 4, KNZ_ERR_CREATE_DECOMPRESSOR = 5, KNZ_ERR_READ_FILE = 11,
    KNZ_ERR_WRITE_FILE = 12, KNZ_ERR_PROCESS_BLOCK = 13, KNZ_ERR_CREATE_CODEC = 14,
    KNZ_ERR_INVALID_FILE = 15, KNZ_ERR_STREAM_VERSION = 16, KNZ_ERR_INVALID_PARAM = 18,
    KNZ_ERR_CRC_CHECK = 19, KNZ_ERR_UNKNOWN = 127,
    KNZ_SKIP = -1
};

/* knz_cfg.flags: KNZ_FLAG_SKIP_BLOCKS = the CLI's -s / ctx["skipBlocks"] (v2/io/CompressedStream.go:778-800): blocks that start
 * with the magic number of a compressed format or whose order-0 entropy is >= 973/1024 are emitted as copy blocks */
enum { KNZ_FLAG_SKIP_BLOCKS = 1 };

/* transform ids, v2/transform/Factory.go:31-53 (6 bits each, first transform in bits 47..42). KNZ_T_TEXT is DICT_TYPE ("TEXT"): which of
 * its two stream formats is written / read follows knz_cfg.entropy (Factory.go:100-120: NONE, HUFFMAN, RANGE, ANS0 -> the byte-oriented one),
 * its hash size follows knz_cfg.block_size (TextCodec.go:610-650, :1137-1188), as ctx["entropy"] / ctx["blockSize"] do in the reference; the data
 * type it detects (ctx["dataType"]) reaches the UTF and LZ stages behind it in the same sequence. */
enum { KNZ_T_NONE = 0, KNZ_T_BWT = 1, KNZ_T_LZ = 3, KNZ_T_ZRLT = 6, KNZ_T_MTFT = 7, KNZ_T_RANK = 8, KNZ_T_TEXT = 10, KNZ_T_SRT = 13, KNZ_T_LZP = 14, KNZ_T_LZX = 16, KNZ_T_UTF = 17, KNZ_T_PACK = 18, KNZ_T_DNA = 19 };
/* entropy ids, v2/entropy/EntropyCodecFactory.go:26-42 */
enum { KNZ_E_NONE = 0, KNZ_E_HUFFMAN = 1, KNZ_E_FPAQ = 2, KNZ_E_ANS0 = 5, KNZ_E_ANS1 = 8 };

/* Flat form of the ctx map handed to every kanzi-go factory (v2/io/CompressedStream.go:217-224,370-382). */
typedef struct {
    uint64_t transform;      /* packed as transform.GetType() returns it (Factory.go:289-328) */
    uint32_t entropy;        /* entropy.GetType() value                                      */
    uint32_t block_size;     /* ctx["blockSize"], multiple of 16, 1 KiB .. 1 GiB              */
    uint32_t checksum_bits;  /* 0, 32 or 64 (Writer hasher32/hasher64)                        */
    uint32_t bs_version;     /* ctx["bsVersion"]; only 6 is produced/accepted                 */
    int32_t  device;         /* HIP device ordinal, -1 = current device                       */
    uint32_t flags;          /* KNZ_FLAG_* bits                                               */
} knz_cfg;

/* One block of a batch: what one encodingTask/decodingTask owns (CompressedStream.go:189-214,1020-1045). */
typedef struct {
    const uint8_t* src;      /* encode: block bytes ; decode: block-local payload (mode byte first) */
    uint32_t src_len;        /* bytes                                                          */
    uint8_t* dst;            /* encode: block-local stream ; decode: decoded bytes              */
    uint32_t dst_cap;
    uint64_t out_bits;       /* encode: exact bit count (obs.Written() after Close, :912-914) ; decode: decoded bytes */
    uint32_t post_len;       /* post-transform length (EVT_AFTER_TRANSFORM size)               */
    uint8_t  skip_flags;     /* ByteTransformSequence.SkipFlags()                              */
    uint8_t  mode;           /* block mode byte                                                */
    uint16_t reserved;
    uint64_t checksum;       /* XXHash32/64 of the original block when checksum_bits != 0       */
    int32_t  status;         /* per-block kanzi error code (0 = ok)                            */
    int32_t  reserved2;
} knz_block;

/* Handle = one GPU batch scheduler (device workspace + stream). One per io.Writer / io.Reader. */
int knz_open(const knz_cfg* cfg, void** handle);
int knz_close(void* handle);
const char* knz_last_error(void* handle);

/*
 * One handle over several devices: the `jobs`-wide goroutine fan-out of Writer.processBlock / Reader.processBlock
 * (v2/io/CompressedStream.go:621-710, :1614-1744) becomes a fan-out over GPUs inside knz_encode_blocks / knz_decode_blocks (SURVEY 8b's
 * device_mask, as a list). ordinals[0..n): HIP device ordinals, one LANE each (own workspace, own stream, own host worker thread), 1 <= n <= 64.
 * An ordinal may be named several times: its lanes share the device, and the uploads / downloads of one run under the kernels of another.
 * A batch is cut into n contiguous balanced ranges (the first nblocks % n lanes take one block more: 26 blocks over 8 lanes = 4,4,3,3,3,3,3,3);
 * every lane copies its blocks in, runs them and copies the results straight into the caller's dst. Blocks are independent
 * (v2/Definitions.go:73-77, io/CompressedStream.go:896-898): no collective is involved and the bytes are those of a one-device handle.
 * Per-block status and the first failing block's error code are reported as by a one-device batch. The other entry points accept such a handle too:
 * single-object calls run on the first lane, device-resident calls (knz_dev_*) on the lane whose device owns d_dst.
 * cfg->device is ignored. knz_device_count() = hipGetDeviceCount (0 without a usable GPU).
 */
int knz_open_devices(const knz_cfg* cfg, const int32_t* ordinals, int n, void** handle);
int knz_device_count(void);
/* lanes behind a handle (1 for a knz_open handle) ; per lane of the last batch call: device ordinal, blocks taken, wall-clock ms (upload .. download). Returns lanes filled. */
int knz_lane_count(void* handle);
int knz_last_lane_times(void* handle, int32_t* devices, int32_t* blocks, float* ms, int cap);

/*
 * Replaces the goroutine fan-out of Writer.processBlock (v2/io/CompressedStream.go:636-701): the n
 * buffered blocks are encoded in one device batch. For every block the result equals
 * encodingTask.encode up to obs.Close() (:729-914): dst holds mode byte .. entropy payload, out_bits the
 * exact bit count. The Go host then performs the ordered emission (:951-976).
 */
int knz_encode_blocks(void* handle, knz_block* blocks, int n);

/*
 * Replaces the concurrent part of Reader.processBlock / decodingTask.decode after the payload has been
 * read from the shared stream (:1875-2011). src = payload bytes (r = (read+7)>>3 of them).
 */
int knz_decode_blocks(void* handle, knz_block* blocks, int n);

/*
 * Whole-stream, device-resident form used by the bench and by multi-GPU sharding: d_src/d_dst are
 * DEVICE pointers. Produces/consumes the complete .knz stream (header :429-519, blocks, end marker
 * :593-594). hip_stream is a hipStream_t (NULL = the handle's own stream). out_bytes is a host pointer.
 * header_input_size is ctx["fileSize"] written to the stream header (0 = unknown).
 * Compressed streams are read as big-endian 32-bit words: d_src of the decode calls (and d_dst of the encode calls) must be 4-byte aligned
 * and readable / writable up to the next multiple of 4 bytes behind n_bytes / dst_cap.
 */
int knz_dev_compress(void* handle, const void* d_src, uint64_t n, int64_t header_input_size,
                     void* d_dst, uint64_t dst_cap, uint64_t* out_bytes, void* hip_stream);
int knz_dev_decompress(void* handle, const void* d_src, uint64_t n_bytes,
                       void* d_dst, uint64_t dst_cap, uint64_t* out_bytes, void* hip_stream);

/*
 * Many independent streams in ONE device batch: what a host that compresses a tree of files (one .knz stream per file) calls instead of
 * K times knz_dev_compress / knz_dev_decompress. All blocks of all streams run side by side through one batch; every pointer of a
 * knz_stream is a DEVICE pointer, the array itself is host memory.
 *   compress:   d_dst[0 .. out_bytes) of stream k is byte for byte what knz_dev_compress(handle, d_src, n, header_input_size, ...) writes
 *               for that input alone (its own header with its own size field, block framing, skip flags, checksums, copy blocks, end
 *               marker; n == 0 gives the header and the end marker, as there). d_src is 16-byte aligned, d_dst 4-byte aligned.
 *   decompress: stream k gives the bytes and out_bytes of knz_dev_decompress for it alone, or that call's error code in status. Every
 *               stream's header is parsed; all streams of a call carry the transform, entropy codec, block size and checksum size of the
 *               first stream whose header parses: one that does not gets KNZ_ERR_INVALID_PARAM. Short inner blocks are placed per stream.
 *   results:    the call returns 0 or the status of the first stream (lowest index) that failed. A stream that fails (damaged, too small
 *               a destination: KNZ_ERR_WRITE_FILE) never keeps the others from completing, and nothing is written behind any dst_cap.
 *               dst_cap follows the single calls' rule (whole big-endian words are stored: the stream plus up to 7 bytes must fit).
 *   counters:   knz_last_counter / knz_last_kernel_times report the one batch (KNZ_COUNTER_POST_TRANSFORM_BYTES: the sum over the streams).
 *   workspace:  a stream list whose workspace the device refuses is taken in halves. On a handle of several lanes the call runs on the
 *               lane that owns streams[0].d_dst; a stream whose d_dst lives on another device gets KNZ_ERR_INVALID_PARAM.
 *   n <= 0 returns 0. There is no limit on n or on the number of blocks beyond the batch's own.
 */
typedef struct {
    const void* d_src; uint64_t n;    /* compress: the input bytes (n may be 0) ; decompress: one .knz stream, 4-byte aligned, readable to the next multiple of 4 */
    void* d_dst; uint64_t dst_cap;    /* 4-byte aligned, same rules as knz_dev_compress / knz_dev_decompress */
    int64_t header_input_size;        /* compress: ctx["fileSize"] for this stream's header (0 = unknown) ; decompress: ignored */
    uint64_t out_bytes;               /* result */
    int32_t status; int32_t reserved; /* result: 0 or this stream's kanzi error code */
} knz_stream;
int knz_dev_compress_many(void* handle, knz_stream* streams, int n, void* hip_stream);
int knz_dev_decompress_many(void* handle, knz_stream* streams, int n, void* hip_stream);

/*
 * Random access: the index of a stream, and the decode of a range of its blocks. What the Reader does with ctx["from"] / ctx["to"] (the CLI's
 * --from / --to, v2/io/CompressedStream.go:1149-1160, :1859-1871: blocks outside the range have their frames read and dropped), device resident.
 * Cost and workspace follow the range, not the stream: only the blocks of the range enter the decode batch.
 *   knz_dev_stream_index:  parses the header (its errors) and walks the framing on the device (its errors: those of the whole-stream decode). Fills
 *               info and pos[0 .. min(info->n_blocks, pos_cap)), a host array that may be NULL. info->n_blocks is always the true count: a second call
 *               can size the array. A stream of header + end marker gives n_blocks 0 and returns 0. d_src as for knz_dev_decompress.
 *   knz_dev_decompress_range: d_dst[0 .. *out_bytes) takes the decoded bytes of blocks from_block .. min(to_block, n_blocks + 1) - 1, from offset 0,
 *               short inner blocks packed: byte for byte what knz_dev_decompress writes for those blocks. {1, KNZ_BLOCK_END, 0} is knz_dev_decompress
 *               (bytes, out_bytes, error code). from_block == 0 or to_block <= from_block: KNZ_ERR_INVALID_PARAM. from_block behind the last block:
 *               *out_bytes = 0, return 0 (the Reader skips every block and reports nothing). dst_cap holds the range as knz_dev_decompress's holds
 *               the stream (block b of the range is decoded at b * block_size before short inner blocks are packed: for a stream a kanzi Writer
 *               wrote that is the decoded bytes of the range and no more); too small: KNZ_ERR_WRITE_FILE, nothing is written behind dst_cap.
 *               THE WALK ENDS ONCE THE LAST BLOCK OF THE RANGE IS LOCATED: framing behind the range is not read (the Reader reads every frame up
 *               to the end marker; this one departure is what makes the call random access). Only the blocks of the range are decoded and checksum
 *               verified: damage outside the range does not fail the call, damaged framing in front of it does, with the whole decode's code.
 *               from_bit != 0: the walk starts at that bit as block from_block (the header is still parsed for the codec parameters). It is a hint
 *               of an untrusted caller: >= 8 * n_bytes or in front of the first block gives KNZ_ERR_INVALID_PARAM; a wrong value inside the stream
 *               behaves like damaged framing or a damaged block (an error code, or bytes that fail their checksum); the frame it names has to be a
 *               block: an end marker there is damaged framing (KNZ_ERR_PROCESS_BLOCK), not an empty range. Whatever it says, every read
 *               stays inside d_src[0 .. n_bytes) rounded up to 4 and every write inside dst_cap.
 *   knz_dev_decompress_many_range: entry k behaves like knz_dev_decompress_range(streams[k], ranges[k]); everything else follows
 *               knz_dev_decompress_many (status / out_bytes per entry, the first header's codec parameters, the lane of streams[0].d_dst, halves
 *               on a refused workspace). The same d_src may appear in several entries. Only the words that hold an entry's selected blocks are
 *               staged: a short range of a very long stream does not copy the stream.
 *   KNZ_COUNTER_DECODE_BATCH_BLOCKS tells "decoded the range" from "decoded everything and sliced".
 */
typedef struct { uint64_t bit; uint64_t bits; } knz_block_pos;
/* bit:  position in the stream of the block's FRAME: the 5-bit width field of Reader.processBlock (:1817). Block 1's equals header_bits.
 * bits: payload bits behind the length field (`read`, :1818). */
typedef struct {
    uint64_t transform; uint32_t entropy, block_size, checksum_bits, bs_version;   /* as the header says */
    int64_t  output_size;   /* the header's size field, 0 = the header has none */
    uint32_t header_bits;   /* first bit behind the header */
    uint32_t n_blocks;      /* frames in front of the end marker */
    uint64_t end_bit;       /* first bit behind the end marker */
} knz_stream_info;
#define KNZ_BLOCK_END 0xFFFFFFFFu
typedef struct {
    uint32_t from_block, to_block;  /* block ids as the reference counts them: the first block is 1. from inclusive, to exclusive.
                                       KNZ_BLOCK_END = through the last block */
    uint64_t from_bit;              /* 0: walk from the header. Otherwise knz_block_pos.bit of block from_block, from an earlier index */
} knz_block_range;
int knz_dev_stream_index(void* handle, const void* d_src, uint64_t n_bytes, knz_stream_info* info,
                         knz_block_pos* pos /* host, may be NULL */, uint32_t pos_cap, void* hip_stream);
int knz_dev_decompress_range(void* handle, const void* d_src, uint64_t n_bytes, const knz_block_range* range,
                             void* d_dst, uint64_t dst_cap, uint64_t* out_bytes, void* hip_stream);
int knz_dev_decompress_many_range(void* handle, knz_stream* streams, const knz_block_range* ranges, int n, void* hip_stream);

/*
 * Byte reads: K triples (source, byte offset, length) and K destinations, a ReadAt over .knz streams. The covering blocks are decoded once, in one
 * batch, and the bytes land where they were asked for; no block ids, no block-sized destinations, no second copy.
 *   addressing: byte `offset` lies in block offset / block_size + 1 at offset % block_size; block_size comes from the stream's header. For a stream a
 *               kanzi Writer wrote, only the last block is short: the offset is then the offset in the decoded stream, and d_dst[0 .. out_bytes) equals
 *               knz_dev_decompress(...)[offset .. offset + out_bytes). A read delivers bytes in order until its length is served or it meets the end
 *               of a block that decoded to fewer than block_size bytes (the stream's last block, or a short inner block): it ends there with status 0
 *               and out_bytes < length, like a short ReadAt. It never delivers a byte from a wrong position. Zero bytes with status 0 are the answer
 *               for an offset at or behind the end, an offset behind a block's decoded length, and length == 0. Blocks in front of a read's first
 *               block are neither decoded nor checked, framing behind its last block is not read (the departure of knz_dev_decompress_range).
 *   once:       the batch holds every distinct (source, block) pair that some read touches, once, however many reads touch it;
 *               KNZ_COUNTER_DECODE_BATCH_BLOCKS reports that number. Two knz_source rows with the same d_src are two sources.
 *   results:    a read's result depends only on its own source and window (the blocks offset / block_size + 1 .. (offset + length - 1) / block_size + 1),
 *               not on what else is in the call or in what order. A read whose window holds a failing block (damaged payload, checksum mismatch,
 *               decoded length above the block size) takes that block's code, the one knz_dev_decompress_range gives for that block alone (the first
 *               such block's, in block order): out_bytes = 0 and NOTHING of its destination is written. A read whose window lies in other blocks of
 *               the same stream completes. Damaged framing in front of a read's first block fails that read with the walk's code (the walk starts at
 *               the header, or at the hinted frame).
 *   sources:    headers are parsed as knz_dev_decompress_many parses them: the first parsable header's transform, entropy codec, block size and
 *               checksum size rule the call, a source that differs gets KNZ_ERR_INVALID_PARAM. A source's non-zero status (its header's code, a NULL
 *               d_src: KNZ_ERR_MISSING_PARAM, a d_src off 4 bytes: KNZ_ERR_INVALID_PARAM) is the status of all its reads.
 *   hints:      with pos present, the walk for block b <= n_pos starts at pos[b-1].bit (knz_block_range.from_bit, checked as there); blocks behind
 *               n_pos walk from the header. Hints come from an untrusted caller: one outside the stream (>= 8 * n, or in front of the header's
 *               end) gives KNZ_ERR_INVALID_PARAM on the reads that use it, a wrong one inside the stream an error code or that frame's bytes.
 *               Whatever the hint says, every read stays inside d_src[0 .. n) rounded up to 4, and every write inside d_dst[0 .. length).
 *   writes:     exactly the bytes d_dst[0 .. out_bytes) of each read are written. Destinations of different reads may be adjacent to the byte, as in
 *               a packed output tensor, at any alignment. Overlapping destinations are the caller's mistake and undefined.
 *   arguments:  offset + length overflowing, or source >= n_sources: KNZ_ERR_INVALID_PARAM on that read. NULL reads or sources (n_reads > 0): the
 *               call returns KNZ_ERR_MISSING_PARAM; a NULL d_dst with length > 0: KNZ_ERR_MISSING_PARAM on that read. n_reads <= 0 returns 0.
 *               The call returns 0 or the status of the first read (lowest index) that failed.
 *   workspace:  a read list whose workspace the device refuses is taken in halves, by the many calls' rule (a block that both halves touch is then
 *               decoded in each). On a handle of several lanes the call runs on the lane that owns reads[0].d_dst.
 *   knz_dev_read: one source, one read, no hint.
 */
typedef struct {
    const void* d_src; uint64_t n;             /* one .knz stream, device; alignment and readability as knz_dev_decompress's d_src */
    const knz_block_pos* pos; uint32_t n_pos;  /* host, may be NULL / 0: rows 0 .. n_pos-1 of knz_dev_stream_index for this stream (blocks 1 .. n_pos) */
    int32_t status;                            /* result: 0, or the code of this stream's header / pointer check; its reads take it */
} knz_source;
typedef struct {
    uint32_t source, reserved;                 /* index into sources[] */
    uint64_t offset, length;                   /* bytes of the decoded stream */
    void*    d_dst;                            /* device, ANY alignment, `length` bytes writable */
    uint64_t out_bytes;                        /* result */
    int32_t  status, reserved2;                /* result: 0 or a kanzi error code */
} knz_read;
int knz_dev_read_many(void* handle, knz_source* sources, int n_sources, knz_read* reads, int n_reads, void* hip_stream);
int knz_dev_read(void* handle, const void* d_src, uint64_t n_bytes, uint64_t offset, uint64_t length,
                 void* d_dst, uint64_t* out_bytes, void* hip_stream);

/*
 * Pattern search: Q queries (source, window, byte string) give the decoded offsets at which the string starts, a bytes.find / zgrep over .knz streams. The
 * covering blocks are decoded once, in one batch, and searched where they lie in the workspace: no decoded byte reaches the caller, only offsets do.
 * Where nothing else is said a query behaves like the read (offset, length + pattern_len - 1) of knz_dev_read_many, its EXTENDED READ.
 *   addressing: as knz_dev_read_many: byte `offset` lies in block offset / block_size + 1 at offset % block_size. Let ext be the bytes the extended read
 *               would deliver: it stops at the end of a block that decoded to fewer than block_size bytes (the stream's last block, or a short inner
 *               block). scanned = min(length, ext). A match is a position p in [offset, offset + scanned) with p - offset + pattern_len <= ext and
 *               the decoded bytes at p .. equal to the pattern: it STARTS inside the window and may end behind the window's end; one that starts
 *               in front of the window is none. Overlapping matches all count: "aaa" in "aaaaa" gives 3.
 *   results:    n_hits is the number of matches and is not clipped. d_hits[0 .. min(n_hits, hits_cap)) holds their absolute decoded offsets in
 *               ascending order, nothing behind that is written (8-byte stores). The same input gives the same words on every run.
 *   once:       every distinct (source, block) pair that some query touches is decoded once, however many queries and patterns name it;
 *               KNZ_COUNTER_DECODE_BATCH_BLOCKS reports that number.
 *   locality:   a query's result depends only on its own source, window and pattern. A failing block inside the extended read's window fails the
 *               query with that block's code (knz_dev_decompress_range's for that block alone): n_hits = 0 and NOTHING of its d_hits is written.
 *               Queries over other blocks of the same stream complete.
 *   no phantom entries: no entry of the batch is made for a block that does not exist. KNZ_LENGTH_END, and windows far past the end, are clamped
 *               to the source's block count, taken from ONE framing walk per queried source (knz_dev_stream_index's walk, up to the last block a
 *               query of the call asks for). Where that walk meets damaged framing, the blocks in front of the damage count: queries inside them
 *               complete, a query that reaches the frame the walk could not read, or lies behind it, fails with the walk's code (as a read there does). Hints (pos / n_pos) mean what they mean for reads; the count walk
 *               starts at the last hinted frame, and is not run where the hints cover every block the queries ask for.
 *   arguments:  pattern_len 0 or above KNZ_FIND_MAX_PATTERN, source >= n_sources, offset + length overflowing (length not KNZ_LENGTH_END), d_hits off
 *               8 bytes: KNZ_ERR_INVALID_PARAM on the query. NULL pattern, NULL d_hits with hits_cap > 0: KNZ_ERR_MISSING_PARAM on the query. A
 *               source's non-zero status (knz_dev_read_many's rules) is the status of its queries. length == 0, or an offset at or behind the end:
 *               status 0, n_hits = 0, scanned = 0. NULL finds or sources (n_finds > 0): the call returns KNZ_ERR_MISSING_PARAM. n_finds <= 0
 *               returns 0. The call returns 0 or the status of the first query (lowest index) that failed.
 *   workspace:  a query list whose workspace the device refuses is taken in halves, as reads are; one query's window has to fit. On a handle of
 *               several lanes the call runs on the lane that owns finds[0].d_hits, else on the first lane.
 *   knz_dev_find: one source, its whole stream ({0, KNZ_LENGTH_END}), no hint. n_hits is a host pointer.
 */
#define KNZ_FIND_MAX_PATTERN 256
#define KNZ_LENGTH_END 0xFFFFFFFFFFFFFFFFull      /* window runs to the end of the stream */
typedef struct {
    uint32_t source, pattern_len;       /* index into sources[]; 1 .. KNZ_FIND_MAX_PATTERN */
    const void* pattern;                /* HOST, pattern_len bytes */
    uint64_t offset, length;            /* matches that START in [offset, offset + length) of the decoded stream */
    uint64_t* d_hits; uint64_t hits_cap;/* device, 8-byte aligned, may be NULL when hits_cap == 0 (count only) */
    uint64_t n_hits, scanned;           /* results */
    int32_t  status, reserved;          /* result */
} knz_find;
int knz_dev_find_many(void* handle, knz_source* sources, int n_sources, knz_find* finds, int n_finds, void* hip_stream);
int knz_dev_find(void* handle, const void* d_src, uint64_t n_bytes, const void* pattern, uint32_t pattern_len,
                 uint64_t* d_hits, uint64_t hits_cap, uint64_t* n_hits, void* hip_stream);   /* one source, whole stream */

/*
 * Byte writes: W writes (byte offset, length, data) into ONE source stream give ONE new stream in d_dst, a WriteAt / append over .knz streams. Blocks are
 * independent and a frame carries no block id (v2/io/CompressedStream.go:896-898, :951-976): only the blocks the writes touch are decoded and encoded
 * again, every other frame is copied bit for bit to its new bit position, the end marker closes the stream. d_dst must not overlap d_src.
 *   addressing: as knz_dev_read_many: byte `offset` lies in block offset / block_size + 1. The old length L = (n_blocks - 1) * block_size + the decoded
 *               length of the last block (0 for a stream of header + end marker). L is needed only when a write reaches the last block (its end lies behind
 *               (n_blocks - 1) * block_size) or uses KNZ_OFFSET_END: the last block then counts as touched, whether a byte of it changes or not.
 *   order:      the writes apply in index order: where two overlap the later one wins. KNZ_OFFSET_END resolves to the length of the stream as it stands
 *               when that write is applied, the growth of earlier writes included. A write whose resolved offset lies behind that length would leave a
 *               hole: KNZ_ERR_INVALID_PARAM on that write. A write may run past the end: the new length L' = max(L, every write's end), the new stream
 *               has ceil(L' / block_size) blocks.
 *   all or nothing: the result is one stream, so a failing write fails the call: it returns the code of the first failing write (lowest index),
 *               *out_bytes = 0 and NO byte of d_dst is written. Every writes[i].status is set: a write's own code (its arguments, a hole, the code of
 *               the first failing block it touches; 0 for a write that is not to blame), or, where the call fails for a reason that is no write's
 *               (the source's header or framing, the configuration, dst_cap, the workspace), that code on every write. Argument errors are reported
 *               before the stream is looked at: holes are then not looked for.
 *   touched:    a block is touched when some write covers one of its bytes (visible or overwritten by a later write), or when it is new. Every touched
 *               existing block is decoded and checksum-verified, all of them in one decode batch (entries of one block each, as knz_dev_read_many's);
 *               the visible bytes of the writes are laid over them; all touched blocks, existing and new, are encoded in one encode batch under the
 *               handle's knz_cfg. A touched block that fails to decode fails the call with the code knz_dev_decompress_range gives for that block
 *               alone. A touched block that is not the last one and decodes to fewer than block_size bytes is a short inner block: its offsets are not
 *               those of the decoded stream, KNZ_ERR_INVALID_PARAM.
 *   untouched:  frames no write touches are never decoded or checked: their bits (framing field and payload) are copied verbatim, damaged payloads and
 *               short inner blocks included. The framing is walked from the header to the end marker: damaged framing anywhere fails the call with
 *               the code knz_dev_stream_index gives for the stream.
 *   configuration: the source header's transform, entropy codec, block size and checksum size must equal the handle's knz_cfg, else
 *               KNZ_ERR_INVALID_PARAM. Hence, for a source written under this configuration and these flags, d_dst[0 .. out_bytes) equals byte for
 *               byte what knz_dev_compress writes for the edited input with the same header_input_size.
 *   header:     rebuilt by the function knz_dev_compress uses; header_input_size means what it means there (0 = no size field).
 *               KNZ_HEADER_SIZE_KEEP: no field if the source has none, else the source's value + (L' - L). The header is 0, 16, 32 or 48 bits longer
 *               with the field (:466-490): another field shifts every frame.
 *   dst_cap:    the single calls' rule: whole big-endian words are stored, the stream plus up to 7 bytes must fit. Checked on the device before any
 *               word is stored; too small: KNZ_ERR_WRITE_FILE, nothing is written. After a good call nothing behind the stream's last word is written.
 *   arguments:  n_writes <= 0: returns 0, *out_bytes = 0, nothing is written. NULL writes, d_src, d_dst or out_bytes: KNZ_ERR_MISSING_PARAM. d_src or d_dst
 *               off 4 bytes: KNZ_ERR_INVALID_PARAM. A NULL d_data with length > 0: KNZ_ERR_MISSING_PARAM on that write; offset + length overflowing:
 *               KNZ_ERR_INVALID_PARAM on that write. d_data may have any alignment.
 *   workspace:  on a handle of several lanes the call runs on the lane that owns d_dst. A decode or encode batch whose workspace the device refuses
 *               is taken in halves (the many calls' rule) ; the touched blocks and their streams themselves have to fit.
 *   counters:   KNZ_COUNTER_DECODE_BATCH_BLOCKS: the touched existing blocks ; KNZ_COUNTER_ENCODE_BATCH_BLOCKS: those and the new ones.
 *   knz_dev_append: one write at KNZ_OFFSET_END (length 0: the stream comes back under the new header).
 */
#define KNZ_OFFSET_END  0xFFFFFFFFFFFFFFFFull    /* "at the end of the decoded stream as it stands when this write is applied" */
#define KNZ_HEADER_SIZE_KEEP (-1)                /* header size field: none if the source has none, else the source's value + (new length - old length) */
typedef struct {
    uint64_t offset, length;   /* bytes of the decoded stream; offset may be KNZ_OFFSET_END */
    const void* d_data;        /* device, ANY alignment, `length` bytes readable */
    int32_t status, reserved;  /* result */
} knz_write;
int knz_dev_write_many(void* handle, const void* d_src, uint64_t n_bytes, knz_write* writes, int n_writes,
                       int64_t header_input_size, void* d_dst, uint64_t dst_cap, uint64_t* out_bytes, void* hip_stream);
int knz_dev_append(void* handle, const void* d_src, uint64_t n_bytes, const void* d_data, uint64_t length,
                   int64_t header_input_size, void* d_dst, uint64_t dst_cap, uint64_t* out_bytes, void* hip_stream);

/*
 * Byte writes into MANY streams: T targets (one source stream, one new stream each) and W writes that name their target, in one call. For every target
 * the call delivers what knz_dev_write_many delivers for that target alone (its text above is the specification): the writes of target t are the rows
 * with target == t, in index order (rows of different targets may interleave), and d_dst[0 .. out_bytes), out_bytes, the target's status (the single
 * call's return value) and its writes' statuses are the single call's. The work of all targets goes through ONE framing pass, ONE decode batch, ONE
 * overlay, ONE encode batch and ONE splice: launches and host synchronisations do not grow with T, and the chains of the transforms run side by side.
 *   failure:    per target, all or nothing: a failed target has out_bytes 0 and NO byte of its d_dst is written, every other target completes. A damaged
 *               touched block, a hole, a header that does not parse, another configuration than the handle's, a dst_cap too small fail their target
 *               only. The call returns 0 or the status of the first failed target (lowest index).
 *   no writes:  a target that no write names gets status 0 and out_bytes 0, nothing of it is read or written (the single call's n_writes <= 0).
 *   arguments:  n_targets <= 0 returns 0. NULL targets, or NULL writes with n_writes > 0: KNZ_ERR_MISSING_PARAM. A write whose target >= n_targets makes
 *               the call malformed: KNZ_ERR_INVALID_PARAM for the call, on every target and every write, nothing is written (the splice call's rule
 *               for `out`). NULL d_src or d_dst (KNZ_ERR_MISSING_PARAM ; the target's writes are not looked at and keep status 0), a write's own
 *               arguments, d_src or d_dst off 4 bytes: the single call's codes, on that target. d_dst on another device than the call's lane, or
 *               d_dst[0 .. dst_cap) overlapping a source of the call or another target's range (checked on the host from the pointers, over the
 *               targets some write names): KNZ_ERR_INVALID_PARAM on that target and on its writes. The same d_src may serve several targets: each
 *               gets its own decoded copies of the blocks it touches, and the source is walked once.
 *   lanes:      on a handle of several lanes the call runs on the lane that owns targets[0].d_dst.
 *   workspace:  a batch whose workspace the device refuses is taken in halves of the target list (the many calls' rule). A target's own touched blocks
 *               and block streams have to fit: a target that does not fit alone takes the workspace's code on itself and on its writes, the others
 *               complete.
 *   counters:   KNZ_COUNTER_DECODE_BATCH_BLOCKS: the touched existing blocks, summed over the targets that reached the decode batch ;
 *               KNZ_COUNTER_ENCODE_BATCH_BLOCKS: the rows of the encode batch, touched and new blocks of all targets.
 *   safety:     whatever a stream says, every read stays inside its own d_src[0 .. n_bytes) rounded up to 4 and every write inside its own target's
 *               dst_cap. Outputs may follow each other to the word: nothing outside a stream's own 32-bit words is written. Nothing is atomic: the same
 *               input gives the same bytes.
 */
typedef struct {
    const void* d_src; uint64_t n_bytes;   /* the source stream: device, 4-byte aligned, readable to the next multiple of 4 */
    void* d_dst; uint64_t dst_cap;         /* the new stream: 4-byte aligned; the single calls' rule for dst_cap */
    int64_t header_input_size;             /* as knz_dev_write_many; KNZ_HEADER_SIZE_KEEP allowed */
    uint64_t out_bytes;                    /* result */
    int32_t status, reserved;              /* result */
} knz_write_target;
typedef struct {
    uint32_t target, reserved0;            /* index into targets[] */
    uint64_t offset, length;               /* as knz_write; offset may be KNZ_OFFSET_END */
    const void* d_data;                    /* device, ANY alignment, `length` bytes readable */
    int32_t status, reserved;              /* result */
} knz_write_to;
int knz_dev_write_streams(void* handle, knz_write_target* targets, int n_targets, knz_write_to* writes, int n_writes, void* hip_stream);

/*
 * Block splice: parts (source stream, block range) become output streams, and nothing but whole frames moves. Blocks are independent, a frame carries no
 * block id, the checksum travels inside the frame and the header does not depend on the block count: concatenating K streams, slicing blocks [from, to)
 * out of one, splitting one into K or regrouping any list of parts into any number of outputs needs no decode chain and no encode chain.
 *   result:     output o holds the header, then the frames of its parts in part order, then the end marker. Every frame is bit for bit the source's:
 *               framing field and payload, copy blocks, skip flags, checksums and damaged payloads included. Nothing is decoded, encoded or
 *               checksum-verified: KNZ_COUNTER_DECODE_BATCH_BLOCKS and KNZ_COUNTER_ENCODE_BATCH_BLOCKS read 0 after the call.
 *   identity:   for whole streams whose decoded lengths, except the last one's, are multiples of the block size, the output equals byte for byte what
 *               knz_dev_compress writes for the concatenated input under that header size.
 *   ranges:     mean what knz_dev_decompress_range's mean (ids from 1, to exclusive, KNZ_BLOCK_END = through the last block). from_block == 0 or
 *               to_block <= from_block: KNZ_ERR_INVALID_PARAM on that part. to_block is clamped to the last block ; a range wholly behind the last
 *               block contributes nothing (status 0, blocks 0). With a finite to_block the framing behind the range is not read: damage there does
 *               not fail the part. With KNZ_BLOCK_END the walk runs to the end marker and checks it. Damaged framing in front of the range or inside
 *               it gives the code knz_dev_stream_index gives for that stream. A stream of header + end marker is a valid, empty part; an output with no
 *               parts, or only empty ones, is header + end marker. Each distinct (d_src, n_bytes) of the call is walked once, from its header to the
 *               largest boundary some part asks for, however many parts and outputs name it.
 *   configuration: every source's transform, entropy codec, block size and checksum size must equal the handle's knz_cfg (the write call's rule), else
 *               KNZ_ERR_INVALID_PARAM on the part ; a header that does not parse gives its code. The header is rebuilt by the function
 *               knz_dev_compress uses ; header_input_size means what it means there (0 = no size field). KNZ_HEADER_SIZE_KEEP: the sum of the sources'
 *               size fields when every part of the output is a whole stream ({1, KNZ_BLOCK_END}) and every such source has the field, else no field.
 *   short inner blocks: a part whose last block is short, followed by another part, gives a short inner block. That is still a valid stream:
 *               knz_dev_decompress and the reference Reader return the concatenation. The byte addressing of knz_dev_read_many and knz_dev_write_many
 *               behind such a block is off, as their own text says. The splice cannot know: it does not decode.
 *   failure:    per output. An output fails with its own pointer code (NULL d_dst: KNZ_ERR_MISSING_PARAM ; d_dst off 4 bytes, on another device than the
 *               call's lane, or d_dst[0 .. dst_cap) overlapping a source of the call or another output's range, checked on the host from the pointers:
 *               KNZ_ERR_INVALID_PARAM), else with the code of its first failing part (lowest index ; a NULL d_src: KNZ_ERR_MISSING_PARAM, a d_src off
 *               4 bytes: KNZ_ERR_INVALID_PARAM, its header's, configuration's, range's or walk's code), else with KNZ_ERR_WRITE_FILE for a dst_cap
 *               too small. dst_cap follows the single calls' rule (whole big-endian words are stored, the stream plus up to 7 bytes must fit) and is
 *               checked on the device before any store. A failed output has out_bytes 0 and NO byte of its d_dst is written ; the other outputs
 *               complete. After a good output nothing behind the stream's last 32-bit word is written. The call returns 0 or the status of the first
 *               failed output (lowest index).
 *   arguments:  n_outs <= 0 returns 0 ; n_parts may be 0. NULL outs, or NULL parts with n_parts > 0: KNZ_ERR_MISSING_PARAM. Parts of one output are
 *               consecutive and in output order: an `out` that is out of range or decreases gives KNZ_ERR_INVALID_PARAM for the call (every output's
 *               status), and nothing is written. The same d_src may appear in any number of parts and outputs.
 *   lanes:      on a handle of several lanes the call runs on the lane that owns outs[0].d_dst.
 *   safety:     whatever a stream says, every read stays inside its own d_src[0 .. n_bytes) rounded up to 4 and every write inside its output's dst_cap.
 *   knz_dev_concat: n whole streams -> one (n <= 0: header + end marker). knz_dev_slice: one range -> one stream. Both are knz_dev_splice_many with one output.
 */
typedef struct {
    const void* d_src; uint64_t n_bytes;  /* one .knz stream, device, 4-byte aligned, readable to the next multiple of 4 */
    uint32_t from_block, to_block;        /* ids from 1, to exclusive, KNZ_BLOCK_END = through the last block (knz_block_range's meaning) */
    uint32_t out;                         /* index into outs[]; parts of one output are consecutive and in output order: out is non-decreasing */
    int32_t  status;                      /* result */
    uint64_t blocks, bits;                /* result: frames taken from this part, and their bits */
} knz_splice_part;
typedef struct {
    void* d_dst; uint64_t dst_cap;        /* 4-byte aligned; the single calls' rule for dst_cap */
    int64_t header_input_size;            /* as knz_dev_compress (0 = no field), or KNZ_HEADER_SIZE_KEEP */
    uint64_t out_bytes, out_blocks;       /* result */
    int32_t status, reserved;             /* result */
} knz_splice_out;
int knz_dev_splice_many(void* handle, knz_splice_part* parts, int n_parts, knz_splice_out* outs, int n_outs, void* hip_stream);
int knz_dev_concat(void* handle, const void* const* d_srcs, const uint64_t* n_bytes, int n, int64_t header_input_size,
                   void* d_dst, uint64_t dst_cap, uint64_t* out_bytes, void* hip_stream);
int knz_dev_slice(void* handle, const void* d_src, uint64_t n_bytes, uint32_t from_block, uint32_t to_block, int64_t header_input_size,
                  void* d_dst, uint64_t dst_cap, uint64_t* out_bytes, void* hip_stream);

/*
 * Multi-GPU block sharding: a rank encodes blocks [first_block, first_block+n_blocks) of a
 * stream whose blocks are block_size bytes each; d_src points at this rank's first block. The result is a
 * bit string (no stream header, no end marker): *out_bits bits, zero padded to a byte in d_dst.
 * knz_dev_assemble() then concatenates the ranks' bit strings, in rank order, behind the stream header
 * and appends the end marker (it is the device form of the ordered emission, :934-976).
 */
int knz_dev_compress_blocks(void* handle, const void* d_src, uint64_t n, void* d_dst, uint64_t dst_cap,
                            uint64_t* out_bits, void* hip_stream);
/* Decode side of the sharding: a rank decodes the framed blocks of its own segment (n_bits bits, no header). */
int knz_dev_decompress_blocks(void* handle, const void* d_src, uint64_t n_bits, void* d_dst, uint64_t dst_cap,
                              uint64_t* out_bytes, void* hip_stream);
int knz_dev_assemble(void* handle, int64_t header_input_size, const void* const* d_segments,
                     const uint64_t* segment_bits, int n_segments, void* d_dst, uint64_t dst_cap,
                     uint64_t* out_bytes, void* hip_stream);

/* Single kanzi.ByteTransform objects (v2/Definitions.go:78-91). type1 = one 6-bit transform id. Host pointers. */
int knz_transform_forward(void* handle, uint64_t type1, const uint8_t* src, uint32_t n,
                          uint8_t* dst, uint32_t cap, uint32_t* out_n);
int knz_transform_inverse(void* handle, uint64_t type1, const uint8_t* src, uint32_t n,
                          uint8_t* dst, uint32_t cap, uint32_t* out_n);
/* ByteTransform.MaxEncodedLen for a packed sequence (Sequence.go:189-205) */
uint32_t knz_max_encoded_len(uint64_t transform, uint32_t n);

/* Single kanzi.EntropyEncoder / EntropyDecoder objects (v2/Definitions.go:154-179). Host pointers.
 * encode: the shim then calls obs.WriteArray(bits, out_bits). decode: bits = the remaining payload. */
int knz_entropy_encode(void* handle, uint32_t type, const uint8_t* src, uint32_t n,
                       uint8_t* bits, uint64_t cap_bytes, uint64_t* out_bits);
int knz_entropy_decode(void* handle, uint32_t type, const uint8_t* bits, uint64_t n_bytes,
                       uint8_t* dst, uint32_t n, uint64_t* used_bits);

/* Timing of the last device batch, measured with HIP events on the stream the kernels ran on.
 * kernel_ms[] receives per-stage times, see KNZ_STAGE_*; returns the number of stages filled. */
enum { KNZ_STAGE_TRANSFORM = 0, KNZ_STAGE_ENTROPY = 1, KNZ_STAGE_LAYOUT = 2, KNZ_STAGE_GATHER = 3, KNZ_STAGE_COUNT = 4 };
int knz_last_timing(void* handle, float* stage_ms, int cap);

/* Per-kernel times of the last device batch: the launches that can dominate a batch (the per-block chains, the entropy
 * kernels) are bracketed by a HIP event pair on the launch stream. names receives the kernel names separated by '\n'
 * (launch order, a kernel launched several times appears several times), ms[i] the duration of launch i. Returns the
 * number of launches reported. bench.py's roofline line is built from these. */
int knz_last_kernel_times(void* handle, char* names, int names_cap, float* ms, int cap);

/* Diagnostic counters of the last device batch. KNZ_COUNTER_HUF_SERIAL_CHUNKS: Huffman chunks the wave-parallel decoder
 * handed back to the serial (reference-order) decoder; 0 for any stream a kanzi encoder wrote. Returns 0 or an error code. */
enum { KNZ_COUNTER_HUF_SERIAL_CHUNKS = 0, KNZ_COUNTER_POST_TRANSFORM_BYTES = 1 /* entropy coder input of the last encode batch */,
       KNZ_COUNTER_TEXT_CHAIN_BLOCKS = 2 /* blocks of the last TEXT stage scanned by the one-lane kernel instead of the parallel one */,
       KNZ_COUNTER_LZ_INV_SERIAL_BLOCKS = 3 /* blocks of the last LZ / LZX inverse stage decoded by the one-wave kernel instead of the parallel one */,
       KNZ_COUNTER_LZ_FWD_SERIAL_BLOCKS = 4 /* blocks of the last LZ / LZX forward stage whose segment-parallel parse did not settle (or that need a
                                               decision the parallel layout leaves to the one-wave kernel): parsed by the one-wave kernel */,
       KNZ_COUNTER_LZ_FWD_ROUNDS = 5 /* rounds the fixed point of the last segment-parallel LZ forward stage took */,
       KNZ_COUNTER_RANK_PIPE_BLOCKS = 6 /* blocks of the last decode batch whose ZRLT / RANK inverses ran as one chain under the order-1 rANS decoder */,
       KNZ_COUNTER_DECODE_BATCH_BLOCKS = 7 /* blocks that entered the last decode batch: a stream's block count after knz_dev_decompress, the blocks of
                                              the range after a range call ; after a many call the sum over its entries, however many batches it took ; after
                                              knz_dev_read_many / knz_dev_find_many the distinct (source, block) pairs its reads / queries touch */,
       KNZ_COUNTER_STAGE_BYTES0 = 8 /* 8 + i: bytes that entered transform stage i (0..7) of the last encode batch, summed over its blocks */,
       KNZ_COUNTER_ENCODE_BATCH_BLOCKS = 16 /* blocks that entered the encode batch of the last knz_dev_write_many / knz_dev_append: the touched and the new ones */ };
int knz_last_counter(void* handle, int id, uint64_t* value);

/* 1 when a transform/entropy id has a device implementation in this build */
int knz_supports(uint64_t transform, uint32_t entropy);

#ifdef __cplusplus
}
#endif
#endif /* KNZ_GPU_H */
