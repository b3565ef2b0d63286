"""ctypes binding of libknz_gpu.so + mirrors of the kanzi-go interfaces for the hot path."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_LIB = None
_LIB_PATH = None

# v2/transform/Factory.go:31-53 ; v2/entropy/EntropyCodecFactory.go:26-42
_TNAMES = {"NONE": 0, "BWT": 1, "LZ": 3, "ZRLT": 6, "MTFT": 7, "RANK": 8, "SRT": 13, "LZP": 14, "LZX": 16, "UTF": 17, "TEXT": 10, "PACK": 18, "DNA": 19}
_ENAMES = {"NONE": 0, "HUFFMAN": 1, "FPAQ": 2, "ANS0": 5, "ANS1": 8}


def transform_type(name):
    """transform.GetType (v2/transform/Factory.go:289-328)."""
    if isinstance(name, int):
        return name
    res, shift = 0, 42
    for tok in name.upper().split("+"):
        t = _TNAMES[tok]
        if t:
            res |= t << shift
            shift -= 6
    return res


def entropy_type(name):
    """entropy.GetType (v2/entropy/EntropyCodecFactory.go:173-206)."""
    return name if isinstance(name, int) else _ENAMES[name.upper()]


class KnzError(RuntimeError):
    """Mirrors io.IOError{msg, code} (v2/io/CompressedStream.go:56-60); code is a kanzi.ERR_* value."""

    def __init__(self, code, msg=""):
        super().__init__(f"kanzi error {code}: {msg}")
        self.code = code


class _Cfg(C.Structure):
    _fields_ = [("transform", C.c_uint64), ("entropy", C.c_uint32), ("block_size", C.c_uint32),
                ("checksum_bits", C.c_uint32), ("bs_version", C.c_uint32), ("device", C.c_int32), ("flags", C.c_uint32)]


class _Block(C.Structure):
    _fields_ = [("src", C.c_void_p), ("src_len", C.c_uint32), ("dst", C.c_void_p), ("dst_cap", C.c_uint32),
                ("out_bits", C.c_uint64), ("post_len", C.c_uint32), ("skip_flags", C.c_uint8), ("mode", C.c_uint8),
                ("reserved", C.c_uint16), ("checksum", C.c_uint64), ("status", C.c_int32), ("reserved2", C.c_int32)]


class _Stream(C.Structure):
    _fields_ = [("d_src", C.c_void_p), ("n", C.c_uint64), ("d_dst", C.c_void_p), ("dst_cap", C.c_uint64),
                ("header_input_size", C.c_int64), ("out_bytes", C.c_uint64), ("status", C.c_int32), ("reserved", C.c_int32)]


class _BlockPos(C.Structure):
    _fields_ = [("bit", C.c_uint64), ("bits", C.c_uint64)]


class _StreamInfo(C.Structure):
    _fields_ = [("transform", C.c_uint64), ("entropy", C.c_uint32), ("block_size", C.c_uint32), ("checksum_bits", C.c_uint32),
                ("bs_version", C.c_uint32), ("output_size", C.c_int64), ("header_bits", C.c_uint32), ("n_blocks", C.c_uint32), ("end_bit", C.c_uint64)]


class _BlockRange(C.Structure):
    _fields_ = [("from_block", C.c_uint32), ("to_block", C.c_uint32), ("from_bit", C.c_uint64)]


class _Source(C.Structure):
    _fields_ = [("d_src", C.c_void_p), ("n", C.c_uint64), ("pos", C.POINTER(_BlockPos)), ("n_pos", C.c_uint32), ("status", C.c_int32)]


class _Read(C.Structure):
    _fields_ = [("source", C.c_uint32), ("reserved", C.c_uint32), ("offset", C.c_uint64), ("length", C.c_uint64), ("d_dst", C.c_void_p),
                ("out_bytes", C.c_uint64), ("status", C.c_int32), ("reserved2", C.c_int32)]


class _Find(C.Structure):
    _fields_ = [("source", C.c_uint32), ("pattern_len", C.c_uint32), ("pattern", C.c_void_p), ("offset", C.c_uint64), ("length", C.c_uint64),
                ("d_hits", C.c_void_p), ("hits_cap", C.c_uint64), ("n_hits", C.c_uint64), ("scanned", C.c_uint64), ("status", C.c_int32), ("reserved", C.c_int32)]


class _Write(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("length", C.c_uint64), ("d_data", C.c_void_p), ("status", C.c_int32), ("reserved", C.c_int32)]


class _WriteTarget(C.Structure):
    _fields_ = [("d_src", C.c_void_p), ("n_bytes", C.c_uint64), ("d_dst", C.c_void_p), ("dst_cap", C.c_uint64), ("header_input_size", C.c_int64),
                ("out_bytes", C.c_uint64), ("status", C.c_int32), ("reserved", C.c_int32)]


class _WriteTo(C.Structure):
    _fields_ = [("target", C.c_uint32), ("reserved0", C.c_uint32), ("offset", C.c_uint64), ("length", C.c_uint64), ("d_data", C.c_void_p),
                ("status", C.c_int32), ("reserved", C.c_int32)]


class _SplicePart(C.Structure):
    _fields_ = [("d_src", C.c_void_p), ("n_bytes", C.c_uint64), ("from_block", C.c_uint32), ("to_block", C.c_uint32), ("out", C.c_uint32),
                ("status", C.c_int32), ("blocks", C.c_uint64), ("bits", C.c_uint64)]


class _SpliceOut(C.Structure):
    _fields_ = [("d_dst", C.c_void_p), ("dst_cap", C.c_uint64), ("header_input_size", C.c_int64), ("out_bytes", C.c_uint64), ("out_blocks", C.c_uint64),
                ("status", C.c_int32), ("reserved", C.c_int32)]


BLOCK_END = 0xFFFFFFFF       # KNZ_BLOCK_END: a range through the last block
OFFSET_END = 0xFFFFFFFFFFFFFFFF   # KNZ_OFFSET_END: a write at the end of the decoded stream as it stands when the write is applied
LENGTH_END = 0xFFFFFFFFFFFFFFFF   # KNZ_LENGTH_END: a find window that runs to the end of the stream
FIND_MAX_PATTERN = 256       # KNZ_FIND_MAX_PATTERN
HEADER_SIZE_KEEP = -1        # KNZ_HEADER_SIZE_KEEP: the source's size field, moved by the growth (splice: the sum of the whole sources' fields)


def library_path():
    return os.environ.get("KNZ_GPU_LIB", os.path.join(_HERE, "libknz_gpu.so"))


def build_library(verbose=False):
    """hipcc cross-compiles the gfx950 library in-tree (works without a GPU)."""
    src = os.path.join(_HERE, "csrc", "knz_gpu.hip")
    out = os.path.join(_HERE, "libknz_gpu.so")
    deps = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))]
    deps.append(os.path.join(_ROOT, "include", "knz_gpu.h"))
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-variable", "-Wno-unused-value",
           "-o", out, src]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


def load_library(path=None):
    """Loads libknz_gpu.so. Raises if it is missing: the product path never falls back to the CPU."""
    global _LIB, _LIB_PATH
    path = path or library_path()
    if _LIB is not None and _LIB_PATH == path:
        return _LIB
    if not os.path.exists(path):
        raise KnzError(4, f"{path} not found: build it with __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                          "there is no CPU fallback")
    L = C.CDLL(path)
    vp, u8p, u64p = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    L.knz_open.argtypes = [C.POINTER(_Cfg), C.POINTER(vp)]
    L.knz_open_devices.argtypes = [C.POINTER(_Cfg), C.POINTER(C.c_int32), C.c_int, C.POINTER(vp)]
    L.knz_device_count.argtypes = []
    L.knz_lane_count.argtypes = [vp]
    L.knz_last_lane_times.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int]
    L.knz_close.argtypes = [vp]
    L.knz_last_error.argtypes = [vp]
    L.knz_last_error.restype = C.c_char_p
    L.knz_encode_blocks.argtypes = [vp, C.POINTER(_Block), C.c_int]
    L.knz_decode_blocks.argtypes = [vp, C.POINTER(_Block), C.c_int]
    L.knz_dev_compress.argtypes = [vp, vp, C.c_uint64, C.c_int64, vp, C.c_uint64, u64p, vp]
    L.knz_dev_decompress.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, u64p, vp]
    L.knz_dev_compress_many.argtypes = [vp, C.POINTER(_Stream), C.c_int, vp]
    L.knz_dev_decompress_many.argtypes = [vp, C.POINTER(_Stream), C.c_int, vp]
    L.knz_dev_stream_index.argtypes = [vp, vp, C.c_uint64, C.POINTER(_StreamInfo), C.POINTER(_BlockPos), C.c_uint32, vp]
    L.knz_dev_decompress_range.argtypes = [vp, vp, C.c_uint64, C.POINTER(_BlockRange), vp, C.c_uint64, u64p, vp]
    L.knz_dev_decompress_many_range.argtypes = [vp, C.POINTER(_Stream), C.POINTER(_BlockRange), C.c_int, vp]
    L.knz_dev_read_many.argtypes = [vp, C.POINTER(_Source), C.c_int, C.POINTER(_Read), C.c_int, vp]
    L.knz_dev_read.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, u64p, vp]
    L.knz_dev_find_many.argtypes = [vp, C.POINTER(_Source), C.c_int, C.POINTER(_Find), C.c_int, vp]
    L.knz_dev_find.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, vp, C.c_uint64, u64p, vp]
    L.knz_dev_write_many.argtypes = [vp, vp, C.c_uint64, C.POINTER(_Write), C.c_int, C.c_int64, vp, C.c_uint64, u64p, vp]
    L.knz_dev_append.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.c_int64, vp, C.c_uint64, u64p, vp]
    L.knz_dev_write_streams.argtypes = [vp, C.POINTER(_WriteTarget), C.c_int, C.POINTER(_WriteTo), C.c_int, vp]
    L.knz_dev_splice_many.argtypes = [vp, C.POINTER(_SplicePart), C.c_int, C.POINTER(_SpliceOut), C.c_int, vp]
    L.knz_dev_concat.argtypes = [vp, C.POINTER(vp), u64p, C.c_int, C.c_int64, vp, C.c_uint64, u64p, vp]
    L.knz_dev_slice.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int64, vp, C.c_uint64, u64p, vp]
    L.knz_dev_compress_blocks.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, u64p, vp]
    L.knz_dev_decompress_blocks.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, u64p, vp]
    L.knz_dev_assemble.argtypes = [vp, C.c_int64, C.POINTER(vp), u64p, C.c_int, vp, C.c_uint64, u64p, vp]
    L.knz_transform_forward.argtypes = [vp, C.c_uint64, u8p, C.c_uint32, u8p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.knz_transform_inverse.argtypes = [vp, C.c_uint64, u8p, C.c_uint32, u8p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.knz_max_encoded_len.argtypes = [C.c_uint64, C.c_uint32]
    L.knz_max_encoded_len.restype = C.c_uint32
    L.knz_entropy_encode.argtypes = [vp, C.c_uint32, u8p, C.c_uint32, u8p, C.c_uint64, u64p]
    L.knz_entropy_decode.argtypes = [vp, C.c_uint32, u8p, C.c_uint64, u8p, C.c_uint32, u64p]
    L.knz_last_timing.argtypes = [vp, C.POINTER(C.c_float), C.c_int]
    L.knz_last_counter.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64)]
    L.knz_last_counter.restype = C.c_int
    L.knz_supports.argtypes = [C.c_uint64, C.c_uint32]
    L.knz_last_kernel_times.argtypes = [vp, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int]
    _LIB, _LIB_PATH = L, path
    return L


def _u8(a):
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(a), dtype=np.uint8)
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint8))


class Codec:
    """One GPU batch scheduler handle (knz_open): what an io.Writer/io.Reader owns in the drop-in."""

    def __init__(self, transform="NONE", entropy="NONE", block_size=4 << 20, checksum_bits=0, device=-1, lib=None, skip_blocks=False, devices=None):
        """skip_blocks = the CLI's -s / ctx["skipBlocks"] (KNZ_FLAG_SKIP_BLOCKS): incompressible blocks become copy blocks.
        devices = a list of HIP ordinals (knz_open_devices): one lane each, the block batches fan out over them; an ordinal may repeat."""
        self.L = load_library(lib)
        self.cfg = _Cfg(transform_type(transform), entropy_type(entropy), block_size, checksum_bits, 6, device, 1 if skip_blocks else 0)
        self.h = C.c_void_p()
        if devices is not None:
            ords = (C.c_int32 * len(devices))(*devices)
            rc = self.L.knz_open_devices(C.byref(self.cfg), ords, len(devices), C.byref(self.h))
        else:
            rc = self.L.knz_open(C.byref(self.cfg), C.byref(self.h))
        if rc:
            raise KnzError(rc, "knz_open failed: " + self.L.knz_last_error(None).decode() + " (no CPU fallback exists)")

    def lane_times(self):
        """[(device ordinal, blocks taken, wall-clock ms)] per lane of the last batch call of a knz_open_devices handle."""
        n = self.L.knz_lane_count(self.h)
        dev, blk, ms = (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_float * n)()
        k = self.L.knz_last_lane_times(self.h, dev, blk, ms, n)
        return [(int(dev[i]), int(blk[i]), float(ms[i])) for i in range(k)]

    def close(self):
        if self.h:
            self.L.knz_close(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise KnzError(rc, self.L.knz_last_error(self.h).decode())

    # ---- device-resident whole-stream calls (pointers are integers: tensor.data_ptr()) ----
    def dev_compress(self, d_src, n, d_dst, dst_cap, header_input_size=None, stream=0):
        out = C.c_uint64()
        hs = n if header_input_size is None else header_input_size
        self._chk(self.L.knz_dev_compress(self.h, d_src, n, hs, d_dst, dst_cap, C.byref(out), stream))
        return out.value

    def dev_decompress(self, d_src, n_bytes, d_dst, dst_cap, stream=0):
        out = C.c_uint64()
        self._chk(self.L.knz_dev_decompress(self.h, d_src, n_bytes, d_dst, dst_cap, C.byref(out), stream))
        return out.value

    def dev_stream_index(self, d_src, n_bytes, stream=0, pos_cap=None):
        """The index of the .knz stream at d_src (knz_dev_stream_index) -> (info dict, [(bit, bits), ...]): the header's fields, header_bits, n_blocks and
        end_bit, and per block the bit of its frame and its payload bits. pos_cap: rows to bring back (default: all, a second call sizes the array;
        0 passes a NULL array); info["n_blocks"] is the true count either way."""
        info = _StreamInfo()
        if pos_cap is None:
            self._chk(self.L.knz_dev_stream_index(self.h, d_src, n_bytes, C.byref(info), None, 0, stream))
            pos_cap = info.n_blocks
        pos = (_BlockPos * max(pos_cap, 1))()
        self._chk(self.L.knz_dev_stream_index(self.h, d_src, n_bytes, C.byref(info), pos if pos_cap else None, pos_cap, stream))
        d = {name: int(getattr(info, name)) for name, _t in _StreamInfo._fields_}
        return d, [(int(pos[i].bit), int(pos[i].bits)) for i in range(min(pos_cap, info.n_blocks))]

    def dev_decompress_range(self, d_src, n_bytes, d_dst, dst_cap, from_block, to_block=None, from_bit=0, stream=0):
        """Blocks from_block .. to_block - 1 of the stream (the first block is 1; to_block None: through the last) decoded to d_dst from offset 0
        (knz_dev_decompress_range). from_bit: 0, or the bit of block from_block's frame from dev_stream_index. Returns the bytes written."""
        out = C.c_uint64()
        rg = _BlockRange(from_block, BLOCK_END if to_block is None else to_block, from_bit)
        self._chk(self.L.knz_dev_decompress_range(self.h, d_src, n_bytes, C.byref(rg), d_dst, dst_cap, C.byref(out), stream))
        return out.value

    def _many(self, fn, items, check, stream, ranged=False):
        n = len(items)
        arr = (_Stream * max(n, 1))()
        rgs = (_BlockRange * max(n, 1))()
        for i, it in enumerate(items):
            arr[i].d_src, arr[i].n, arr[i].d_dst, arr[i].dst_cap = it[0], it[1], it[2], it[3]
            if ranged:
                rgs[i].from_block, rgs[i].to_block = it[4], BLOCK_END if (len(it) < 6 or it[5] is None) else it[5]
                rgs[i].from_bit = it[6] if len(it) > 6 else 0
                continue
            arr[i].header_input_size = it[4] if len(it) > 4 and it[4] is not None else (it[1] if fn is self.L.knz_dev_compress_many else 0)
        rc = fn(self.h, arr, rgs, n, stream) if ranged else fn(self.h, arr, n, stream)
        self.last_many_rc = rc
        if check:
            self._chk(rc)
        return [(int(arr[i].out_bytes), int(arr[i].status)) for i in range(n)]

    def dev_compress_many(self, items, check=False, stream=0):
        """items: [(d_src, n, d_dst, dst_cap[, header_input_size])], one .knz stream each, all their blocks in one device batch
        (knz_dev_compress_many). Returns [(out_bytes, status)] per stream; the call's own return value is in last_many_rc. Raises only with
        check=True (the first failing stream's code). header_input_size defaults to n, as in dev_compress."""
        return self._many(self.L.knz_dev_compress_many, items, check, stream)

    def dev_decompress_many(self, items, check=False, stream=0):
        """items: [(d_src, n_bytes, d_dst, dst_cap)], one .knz stream each (knz_dev_decompress_many). Returns [(out_bytes, status)]."""
        return self._many(self.L.knz_dev_decompress_many, items, check, stream)

    def dev_decompress_many_range(self, items, check=False, stream=0):
        """items: [(d_src, n_bytes, d_dst, dst_cap, from_block[, to_block[, from_bit]])], entry k as dev_decompress_range of it alone, all their blocks in one
        device batch (knz_dev_decompress_many_range); the same d_src may appear in several entries. Returns [(out_bytes, status)]."""
        return self._many(self.L.knz_dev_decompress_many_range, items, check, stream, ranged=True)

    def dev_read(self, d_src, n_bytes, offset, length, d_dst, stream=0):
        """Bytes [offset, offset + length) of the decoded stream at d_src to d_dst, any alignment (knz_dev_read): only the covering blocks are decoded.
        Returns the bytes written: fewer than length where the stream, or a short inner block, ends."""
        out = C.c_uint64()
        self._chk(self.L.knz_dev_read(self.h, d_src, n_bytes, offset, length, d_dst, C.byref(out), stream))
        return out.value

    @staticmethod
    def _sources(sources):
        """[(d_src, n_bytes[, index_rows])] -> the knz_source array of a read or find call, and what has to stay alive while it runs"""
        ns = len(sources)
        src, keep = (_Source * max(ns, 1))(), []
        for i, it in enumerate(sources):
            src[i].d_src, src[i].n = it[0], it[1]
            rows = it[2] if len(it) > 2 and it[2] else None
            if rows:
                pos = (_BlockPos * len(rows))()
                for j, (bit, bits) in enumerate(rows):
                    pos[j].bit, pos[j].bits = bit, bits
                keep.append(pos)
                src[i].pos, src[i].n_pos = pos, len(rows)
        return src, keep

    def dev_read_many(self, sources, reads, check=False, stream=0):
        """sources: [(d_src, n_bytes[, index_rows])], index_rows the [(bit, bits)] of dev_stream_index (or its first rows) as hints; reads: [(source, offset,
        length, d_dst)]. Every distinct (source, block) the reads touch is decoded once, in one device batch (knz_dev_read_many). Returns
        [(out_bytes, status)] per read; the call's own return value is in last_many_rc, the sources' statuses in last_source_status. Raises only with
        check=True (the first failing read's code)."""
        ns, nr = len(sources), len(reads)
        rd = (_Read * max(nr, 1))()
        src, keep = self._sources(sources)
        for i, (s, offset, length, d_dst) in enumerate(reads):
            rd[i].source, rd[i].offset, rd[i].length, rd[i].d_dst = s, offset, length, d_dst
        rc = self.L.knz_dev_read_many(self.h, src, ns, rd, nr, stream)
        self.last_many_rc = rc
        self.last_source_status = [int(src[i].status) for i in range(ns)]
        if check:
            self._chk(rc)
        return [(int(rd[i].out_bytes), int(rd[i].status)) for i in range(nr)]

    def dev_find(self, d_src, n_bytes, pattern, d_hits=None, hits_cap=0, stream=0):
        """Where `pattern` (bytes, 1 .. FIND_MAX_PATTERN of them) starts in the decoded stream at d_src (knz_dev_find): returns the number of matches,
        overlapping ones included; the first min(that, hits_cap) decoded offsets go to the uint64 array d_hits on the device, in ascending order."""
        pat = bytes(pattern)
        out = C.c_uint64()
        self._chk(self.L.knz_dev_find(self.h, d_src, n_bytes, C.c_char_p(pat) if pat else None, len(pat), d_hits, hits_cap, C.byref(out), stream))
        return out.value

    def dev_find_many(self, sources, finds, check=False, stream=0):
        """sources: as dev_read_many's; finds: [(source, pattern, offset, length, d_hits, hits_cap)], matches of `pattern` that START in [offset, offset + length)
        of the decoded stream (length None: to the end), d_hits a uint64 device array of hits_cap words (None / 0: count only). Every distinct
        (source, block) the queries touch is decoded once, in one device batch, and searched in the workspace (knz_dev_find_many). Returns
        [(n_hits, scanned, status)] per query; the call's own return value is in last_many_rc, the sources' statuses in last_source_status. Raises
        only with check=True (the first failing query's code)."""
        ns, nf = len(sources), len(finds)
        fd = (_Find * max(nf, 1))()
        src, keep = self._sources(sources)
        for i, (s, pattern, offset, length, d_hits, hits_cap) in enumerate(finds):
            buf = None if pattern is None else C.create_string_buffer(bytes(pattern), max(len(pattern), 1))
            keep.append(buf)
            fd[i].source, fd[i].pattern_len, fd[i].pattern = s, 0 if pattern is None else len(pattern), None if buf is None else C.addressof(buf)
            fd[i].offset, fd[i].length, fd[i].d_hits, fd[i].hits_cap = offset, LENGTH_END if length is None else length, d_hits, hits_cap
        rc = self.L.knz_dev_find_many(self.h, src, ns, fd, nf, stream)
        self.last_many_rc = rc
        self.last_source_status = [int(src[i].status) for i in range(ns)]
        if check:
            self._chk(rc)
        return [(int(fd[i].n_hits), int(fd[i].scanned), int(fd[i].status)) for i in range(nf)]

    def dev_write_many(self, d_src, n_bytes, writes, d_dst, dst_cap, header_input_size=HEADER_SIZE_KEEP, check=False, stream=0):
        """writes: [(offset, length, d_data)], bytes of the decoded stream at d_src (offset may be OFFSET_END), applied in order; the new stream goes to
        d_dst (knz_dev_write_many): only the blocks the writes touch are decoded and encoded again, every other frame is copied bit for bit. Returns
        (out_bytes, [status] per write); the call's own return value is in last_many_rc. All or nothing: a failing write fails the call, out_bytes is 0
        and d_dst is untouched. Raises only with check=True."""
        n = len(writes)
        arr = (_Write * max(n, 1))()
        for i, (offset, length, d_data) in enumerate(writes):
            arr[i].offset, arr[i].length, arr[i].d_data = offset, length, d_data
        out = C.c_uint64()
        rc = self.L.knz_dev_write_many(self.h, d_src, n_bytes, arr, n, header_input_size, d_dst, dst_cap, C.byref(out), stream)
        self.last_many_rc = rc
        if check:
            self._chk(rc)
        return out.value, [int(arr[i].status) for i in range(n)]

    def dev_append(self, d_src, n_bytes, d_data, length, d_dst, dst_cap, header_input_size=HEADER_SIZE_KEEP, check=False, stream=0):
        """length bytes at d_data behind the end of the decoded stream at d_src, the new stream to d_dst (knz_dev_append). Returns out_bytes (0 where the
        call fails); the return value is in last_many_rc. Raises only with check=True."""
        out = C.c_uint64()
        rc = self.L.knz_dev_append(self.h, d_src, n_bytes, d_data, length, header_input_size, d_dst, dst_cap, C.byref(out), stream)
        self.last_many_rc = rc
        if check:
            self._chk(rc)
        return out.value

    def dev_write_streams(self, targets, writes, check=False, stream=0):
        """targets: [(d_src, n_bytes, d_dst, dst_cap[, header_input_size])], one source stream and one new stream each (header size default
        HEADER_SIZE_KEEP); writes: [(target, offset, length, d_data)], each into the decoded stream of its target, applied per target in index order
        (knz_dev_write_streams). Every target gets what dev_write_many gives for it alone, all of them through one decode batch, one encode batch and
        one splice. Returns ([(out_bytes, status)] per target, [status] per write); the call's own return value is in last_many_rc. A failed target has
        out_bytes 0 and its d_dst untouched, the others complete. Raises only with check=True."""
        n, m = len(targets), len(writes)
        ta, wa = (_WriteTarget * max(n, 1))(), (_WriteTo * max(m, 1))()
        for i, it in enumerate(targets):
            ta[i].d_src, ta[i].n_bytes, ta[i].d_dst, ta[i].dst_cap = it[0], it[1], it[2], it[3]
            ta[i].header_input_size = it[4] if len(it) > 4 and it[4] is not None else HEADER_SIZE_KEEP
        for i, (target, offset, length, d_data) in enumerate(writes):
            wa[i].target, wa[i].offset, wa[i].length, wa[i].d_data = target, offset, length, d_data
        rc = self.L.knz_dev_write_streams(self.h, ta, n, wa, m, stream)
        self.last_many_rc = rc
        if check:
            self._chk(rc)
        return [(int(ta[i].out_bytes), int(ta[i].status)) for i in range(n)], [int(wa[i].status) for i in range(m)]

    def dev_splice_many(self, parts, outs, check=False, stream=0):
        """parts: [(d_src, n_bytes, from_block, to_block, out)], blocks from_block .. to_block - 1 (ids from 1; to_block None: through the last) of the stream at
        d_src go to output `out`; the parts of one output are consecutive and in output order. outs: [(d_dst, dst_cap[, header_input_size])], the header
        size as dev_compress's (0: no field; default HEADER_SIZE_KEEP). Whole frames move bit for bit, nothing is decoded or encoded
        (knz_dev_splice_many). Returns ([(out_bytes, out_blocks, status)] per output, [(blocks, bits, status)] per part); the call's own return value
        is in last_many_rc. A failed output has out_bytes 0 and its d_dst untouched, the others complete. Raises only with check=True."""
        n, m = len(parts), len(outs)
        pa, oa = (_SplicePart * max(n, 1))(), (_SpliceOut * max(m, 1))()
        for i, (d_src, n_bytes, from_block, to_block, out) in enumerate(parts):
            pa[i].d_src, pa[i].n_bytes, pa[i].from_block, pa[i].out = d_src, n_bytes, from_block, out
            pa[i].to_block = BLOCK_END if to_block is None else to_block
        for i, it in enumerate(outs):
            oa[i].d_dst, oa[i].dst_cap = it[0], it[1]
            oa[i].header_input_size = it[2] if len(it) > 2 and it[2] is not None else HEADER_SIZE_KEEP
        rc = self.L.knz_dev_splice_many(self.h, pa, n, oa, m, stream)
        self.last_many_rc = rc
        if check:
            self._chk(rc)
        return ([(int(oa[i].out_bytes), int(oa[i].out_blocks), int(oa[i].status)) for i in range(m)],
                [(int(pa[i].blocks), int(pa[i].bits), int(pa[i].status)) for i in range(n)])

    def dev_concat(self, d_srcs, n_bytes, d_dst, dst_cap, header_input_size=HEADER_SIZE_KEEP, check=False, stream=0):
        """The whole streams at d_srcs[i] (n_bytes[i] bytes each), in order, as one stream at d_dst (knz_dev_concat). Returns out_bytes (0 where the call
        fails); the return value is in last_many_rc. Raises only with check=True."""
        n = len(d_srcs)
        srcs = (C.c_void_p * max(n, 1))(*d_srcs)
        lens = (C.c_uint64 * max(n, 1))(*n_bytes)
        out = C.c_uint64()
        rc = self.L.knz_dev_concat(self.h, srcs, lens, n, header_input_size, d_dst, dst_cap, C.byref(out), stream)
        self.last_many_rc = rc
        if check:
            self._chk(rc)
        return out.value

    def dev_slice(self, d_src, n_bytes, from_block, to_block, d_dst, dst_cap, header_input_size=HEADER_SIZE_KEEP, check=False, stream=0):
        """Blocks from_block .. to_block - 1 (to_block None: through the last) of the stream at d_src as a stream of their own at d_dst (knz_dev_slice).
        Returns out_bytes (0 where the call fails); the return value is in last_many_rc. Raises only with check=True."""
        out = C.c_uint64()
        rc = self.L.knz_dev_slice(self.h, d_src, n_bytes, from_block, BLOCK_END if to_block is None else to_block, header_input_size, d_dst, dst_cap,
                                  C.byref(out), stream)
        self.last_many_rc = rc
        if check:
            self._chk(rc)
        return out.value

    def dev_compress_blocks(self, d_src, n, d_dst, dst_cap, stream=0):
        out = C.c_uint64()
        self._chk(self.L.knz_dev_compress_blocks(self.h, d_src, n, d_dst, dst_cap, C.byref(out), stream))
        return out.value

    def dev_decompress_blocks(self, d_src, n_bits, d_dst, dst_cap, stream=0):
        out = C.c_uint64()
        self._chk(self.L.knz_dev_decompress_blocks(self.h, d_src, n_bits, d_dst, dst_cap, C.byref(out), stream))
        return out.value

    def dev_assemble(self, header_input_size, segments, segment_bits, d_dst, dst_cap, stream=0):
        n = len(segments)
        segs = (C.c_void_p * n)(*segments)
        bits = (C.c_uint64 * n)(*segment_bits)
        out = C.c_uint64()
        self._chk(self.L.knz_dev_assemble(self.h, header_input_size, segs, bits, n, d_dst, dst_cap, C.byref(out), stream))
        return out.value

    def last_counter(self, cid=0):
        v = C.c_uint64()
        self._chk(self.L.knz_last_counter(self.h, cid, C.byref(v)))
        return v.value

    def last_timing(self):
        t = (C.c_float * 4)()
        n = self.L.knz_last_timing(self.h, t, 4)
        return [t[i] for i in range(n)]

    def last_kernel_times(self):
        """[(kernel name, ms)] of the probed launches of the last device batch (HIP events on the launch stream)."""
        names = C.create_string_buffer(16384)
        ms = (C.c_float * 128)()
        n = self.L.knz_last_kernel_times(self.h, names, 16384, ms, 128)
        nm = names.value.decode().split("\n")
        return [(nm[i], float(ms[i])) for i in range(n)]


class BlockBatch:
    """Writer.processBlock / Reader.processBlock re-pointed at the GPU (host buffers in, host buffers out)."""

    def __init__(self, codec: Codec):
        self.c = codec

    def encode(self, blocks):
        """blocks: list of bytes. Returns [(block_local_stream_bytes, written_bits, mode, post_len, skip_flags)] like
        encodingTask.encode up to obs.Close() (v2/io/CompressedStream.go:729-914)."""
        n = len(blocks)
        arr = (_Block * n)()
        keep = []
        for i, b in enumerate(blocks):
            a, _ = _u8(b)
            cap = int(self.c.L.knz_max_encoded_len(self.c.cfg.transform, len(a))) * 2 + 262144
            o = np.zeros(cap, dtype=np.uint8)
            keep.append((a, o))
            arr[i].src = a.ctypes.data
            arr[i].src_len = len(a)
            arr[i].dst = o.ctypes.data
            arr[i].dst_cap = cap
        self.c._chk(self.c.L.knz_encode_blocks(self.c.h, arr, n))
        return [(keep[i][1][: (arr[i].out_bits + 7) // 8].tobytes(), int(arr[i].out_bits), int(arr[i].mode), int(arr[i].post_len),
                 int(arr[i].skip_flags)) for i in range(n)]

    def decode(self, payloads):
        """payloads: list of block-local streams. Returns the decoded blocks (decodingTask.decode :1875-2011)."""
        n = len(payloads)
        arr = (_Block * n)()
        keep = []
        cap = self.c.cfg.block_size + max(512, self.c.cfg.block_size >> 4)
        for i, b in enumerate(payloads):
            a, _ = _u8(b)
            o = np.zeros(cap, dtype=np.uint8)
            keep.append((a, o))
            arr[i].src = a.ctypes.data
            arr[i].src_len = len(a)
            arr[i].dst = o.ctypes.data
            arr[i].dst_cap = cap
        self.c._chk(self.c.L.knz_decode_blocks(self.c.h, arr, n))
        return [keep[i][1][: arr[i].out_bits].tobytes() for i in range(n)]


class EntropyEncoder:
    """kanzi.EntropyEncoder (v2/Definitions.go:154-165) over knz_entropy_encode: Write returns the bit string the
    Go shim hands to obs.WriteArray."""

    def __init__(self, codec: Codec, etype):
        self.c, self.t = codec, entropy_type(etype)

    def write(self, block):
        a, p = _u8(block)
        cap = len(a) * 2 + 262144
        out = np.zeros(cap, dtype=np.uint8)
        bits = C.c_uint64()
        self.c._chk(self.c.L.knz_entropy_encode(self.c.h, self.t, p, len(a), out.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(bits)))
        return out[: (bits.value + 7) // 8].tobytes(), bits.value


class EntropyDecoder:
    """kanzi.EntropyDecoder (v2/Definitions.go:168-179) over knz_entropy_decode."""

    def __init__(self, codec: Codec, etype):
        self.c, self.t = codec, entropy_type(etype)

    def read(self, payload, n):
        a, p = _u8(payload)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        used = C.c_uint64()
        self.c._chk(self.c.L.knz_entropy_decode(self.c.h, self.t, p, len(a), out.ctypes.data_as(C.POINTER(C.c_uint8)), n, C.byref(used)))
        return out[:n].tobytes(), used.value


class ByteTransform:
    """kanzi.ByteTransform (v2/Definitions.go:78-91) over knz_transform_forward/inverse. forward() returns None
    when the transform declines (a Forward error means "skip", v2/transform/Sequence.go:86-91)."""

    def __init__(self, codec: Codec, ttype):
        self.c = codec
        self.t = _TNAMES[ttype.upper()] if isinstance(ttype, str) else ttype

    def max_encoded_len(self, n):
        return int(self.c.L.knz_max_encoded_len(self.t << 42, n))

    def forward(self, src):
        a, p = _u8(src)
        cap = self.max_encoded_len(len(a)) + 64
        out = np.zeros(cap, dtype=np.uint8)
        n = C.c_uint32()
        rc = self.c.L.knz_transform_forward(self.c.h, self.t, p, len(a), out.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(n))
        if rc == -1:
            return None
        self.c._chk(rc)
        return out[: n.value].tobytes()

    def inverse(self, src, cap):
        a, p = _u8(src)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        n = C.c_uint32()
        self.c._chk(self.c.L.knz_transform_inverse(self.c.h, self.t, p, len(a), out.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(n)))
        return out[: n.value].tobytes()
