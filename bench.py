#!/usr/bin/env python3
"""bench.py — encode+decode throughput of the MI355X-native Kanzi hot path (BASELINE.json metric).

Workload (N=1, default): BASELINE.json configs[3] = `-t BWT+RANK+ZRLT -e ANS1 -b 8m` on S-silesia (211,957,760 synthetic
bytes shaped like silesia.tar, bench_corpus.py; 26 blocks) — the configuration the north-star target is quoted on.
One step = compress the whole stream on the device (bit-exact .knz) and decompress it back, inputs resident in HBM.
value = uncompressed MB (10^6 B) per second of a whole round trip; encode-only and decode-only rates are reported next to
it. The other BASELINE configs are reachable with --config (huffman = configs[1], lz / ans0 = configs[2], fpaq = configs[4]).

N>1: `--scaling weak` (default): the blocks of a stream are independent units, so the ranks are handed one corpus copy each (per-GPU work fixed:
N copies of the corpus back to back in ONE stream, split into contiguous balanced block ranges: about one copy per rank), every rank encodes / decodes its own
blocks, the compressed segments are gathered to rank 0 over RCCL with their exact sizes (grouped send/recv, no padding) and assembled
bit-granularly there; the gather stays in flight while each rank decodes its own segment. value = bytes of all ranks / step time (max over
ranks). This is the mode the path scales in: its time is set by per-block chains whose cost does not depend on how many run side by side
(DESIGN.md sections 4.9 and 5).
`--scaling strong`: the SAME job (one S-silesia stream, 26 blocks) split over the ranks (26 blocks over 8 GPUs = 4,4,3,3,3,3,3,3). A rank's step
is never shorter than its slowest block's chains, so this mode cannot go much above 1x for the chain-bound configurations; it is kept
for the configurations that are not (--config lz, huffman, ans0).

Also on the line: roofline of the dominant KERNEL (HIP-event time of its launches inside the library, `knz_last_kernel_times`,
recorded during the timed steps). A plain run does nothing else: it sets up, warms up, times the steps and prints the line.
`--full` adds what takes work of its own (N=1): HBM traffic from two live rocprofv3 PMC passes of this same command when
rocprofv3 is present, the PCIe-inclusive rate of the host-pointer batch hook the cgo shim calls (`host_hook_MBps`), the CPU
baseline (the reference's own code translated, beside the oracle = C++ restatement of the kanzi-go CPU path, bounded sample),
the FPAQ stage comparison, and the checks of the timed stream against the oracle (`bit_exact_vs_oracle`) and the reference-written
stream (`bit_exact_vs_reference`); N>1, strong: the weak-scaling region.

`--dump-outputs DIR` writes what the last timed step handed its caller (the .knz stream, the decoded bytes) as .npy files
(dump_outputs): the inputs are the same on every run, so two builds can be compared output for output.

Other modes (one JSON object instead of the line): `--handles 1,2,4,8` = K host threads x one handle each at the host-pointer boundary; `--in-process-devices 1,2,4,8
[--depth N]` = ONE handle of knz_open_devices over K lanes (what Writer / Reader.EnableGPUDevices binds: lane i on device i % devices present, so an 8-GPU box measures one
lane per GPU and a one-GPU box K logical devices); `--copies K` = K corpus copies in one stream (single-GPU saturation). `--corpus PATH` runs the line on a file (the real
silesia.tar / enwik9 where a driver has them; `data` then says "file").

KNZ_BENCH_EMU=1 is a TEST HARNESS switch (tests/test_bench_ranks.py): the same control flow on CPU tensors with the kernels
compiled against tests/emu and gloo instead of RCCL, so that the N>1 step can be exercised without GPUs. It is not a
product path and its JSON says so.

Prints ONE JSON line on rank 0.
"""
import argparse
import glob
import importlib.util
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)

CONFIGS = {
    # name: (transform, entropy, block size, BASELINE.json config index, corpus)
    "huffman": ("NONE", "HUFFMAN", 4 << 20, 1, "silesia"),
    "ans0": ("NONE", "ANS0", 4 << 20, 2, "silesia"),       # entropy half of configs[2]
    "lz": ("LZ", "ANS0", 4 << 20, 2, "silesia"),
    "bwt": ("BWT+RANK+ZRLT", "ANS1", 8 << 20, 3, "silesia"),
    "l5": ("TEXT+UTF+BWT+RANK+ZRLT", "ANS0", 4 << 20, 3, "silesia"),    # the reference's `-l 5` preset itself (the published 225 / 533 MB/s)
    "fpaq": ("BWT+RANK+ZRLT", "FPAQ", 32 << 20, 4, "enwik"),   # configs[4]: S-enwik, 10^9 B = 30 blocks (the stated size; --size shrinks it for debugging)
}

# what the reference publishes for the nearest shipped preset (other hardware; context only)
PUBLISHED = {
    "bwt": {"preset": "-l 5 = TEXT+UTF+BWT+RANK+ZRLT&ANS0, 4 MiB blocks", "encode_MBps": 225, "decode_MBps": 533,
            "hardware": "AMD Ryzen 9950X, 16 jobs", "source": "kanzi-go README.md:79"},
    "l5": {"preset": "-l 5 = TEXT+UTF+BWT+RANK+ZRLT&ANS0, 4 MiB blocks (this configuration)", "encode_MBps": 225, "decode_MBps": 533,
           "hardware": "AMD Ryzen 9950X, 16 jobs", "source": "kanzi-go README.md:79"},
    "fpaq": {"preset": "-l 6 = TEXT+UTF+BWT+SRT+ZRLT&FPAQ, 8 MiB blocks", "encode_MBps": 169, "decode_MBps": 218,
             "hardware": "AMD Ryzen 9950X, 16 jobs", "source": "kanzi-go README.md:81"},
    "lz": {"preset": "-l 2 = DNA+LZ&HUFFMAN, 4 MiB blocks", "encode_MBps": 1547, "decode_MBps": 2409,
           "hardware": "AMD Ryzen 9950X, 16 jobs", "source": "kanzi-go README.md:68"},
}

# algorithmic HBM bytes of one launch over a batch: n = bytes in front of the transforms, m = bytes behind them (entropy
# coder input), c = compressed bytes (every stage reads its input once and writes its output once)
KERNEL_BYTES = {
    "knz_rank_inverse_chain_kernel": lambda n, m, c: 2 * n, "knz_sbrt_inverse_kernel": lambda n, m, c: 2 * n,
    # the fused ZRLT / RANK inverse does both stages' algorithmic work: ZRLT stream m in, n ranks out, n ranks in, n symbols out ("ZRLT/RANK N + N'")
    "knz_zrlti_rank_pipe_kernel": lambda n, m, c: m + 3 * n,
    "knz_sbrt_apply_kernel": lambda n, m, c: 2 * n, "knz_bwt_inv_chains_kernel": lambda n, m, c: 2 * n,
    "knz_bwt_inv_walk_kernel": lambda n, m, c: 2 * n, "knz_bwt_inv_emit_kernel": lambda n, m, c: 2 * n,
    "knz_ans1_decode_lds_kernel": lambda n, m, c: c + m, "knz_ans1_decode_kernel": lambda n, m, c: c + m,
    "knz_ans1_encode_kernel": lambda n, m, c: m + c, "knz_ans1_expand_kernel": lambda n, m, c: m, "knz_ans1_hist_kernel": lambda n, m, c: m,
    "knz_fpaq_encode_kernel": lambda n, m, c: m + c, "knz_fpaq_decode_kernel": lambda n, m, c: c + m,
    "knz_fpaq_probs_kernel": lambda n, m, c: m, "knz_fpaq_code_kernel": lambda n, m, c: m + c,
    "knz_lz_forward_kernel": lambda n, m, c: n + m, "knz_lz_inverse_kernel": lambda n, m, c: m + n,
    "knz_lz_forward_par_kernel": lambda n, m, c: n + m, "knz_lzi_litext_chain_kernel": lambda n, m, c: m, "knz_lzi_jump_kernel": lambda n, m, c: 2 * n,
    "knz_lzi_map_kernel": lambda n, m, c: m + n, "knz_lzi_gather_kernel": lambda n, m, c: m + n, "knz_lzi_b_apply_kernel": lambda n, m, c: m,
    "knz_lz_parse_kernel": lambda n, m, c: n + m, "knz_lz_candidates_kernel": lambda n, m, c: n,
    "knz_lzp_forward_kernel": lambda n, m, c: n + m, "knz_lzp_inverse_kernel": lambda n, m, c: m + n,
    "knz_srt_inverse_kernel": lambda n, m, c: 2 * n,
    "knz_huf_hist_kernel": lambda n, m, c: m, "knz_huf_lengths_kernel": lambda n, m, c: 768 * ((m + 16383) // 16384),
    "knz_huf_encode_kernel": lambda n, m, c: m + c, "knz_huf_encode_kernel<false>": lambda n, m, c: m + c,
    "knz_huf_encode_kernel<true>": lambda n, m, c: 2048 * ((m + 16383) // 16384), "knz_huf_walk_decode_kernel": lambda n, m, c: c + m,
    "knz_huf_decode_par_kernel": lambda n, m, c: c + m, "knz_ans0_encode_kernel": lambda n, m, c: m + c,
    "knz_ans0_walk_decode_kernel": lambda n, m, c: c + m, "knz_ans0_decode_kernel": lambda n, m, c: c + m,
    "knz_gather_kernel": lambda n, m, c: 2 * c, "knz_utf_forward_kernel": lambda n, m, c: 2 * n, "knz_utf_inverse_kernel": lambda n, m, c: 2 * n,
    "knz_text_forward_chain_kernel": lambda n, m, c: 2 * n, "knz_text_inverse_chain_kernel": lambda n, m, c: 2 * n,
    "knz_ans1_encode_asm_kernel": lambda n, m, c: m + c, "knz_ans1_decode_lds2_kernel": lambda n, m, c: c + m,
    "knz_bwt_output_kernel": lambda n, m, c: 2 * n, "knz_zrlt_seg_kernel": lambda n, m, c: n, "knz_zrlti_seg_kernel": lambda n, m, c: n,
    "knz_lzs_parse_kernel": lambda n, m, c: n + m, "knz_huf_decode_kernel": lambda n, m, c: c + m,
    # the suffix sort's working kernels move (key, value) pairs, not stream bytes: their rows carry the counter bytes only
}


# rocprofv3's FETCH_SIZE on gfx950 tallies 128-byte requests at 64 bytes (MI355X_MICROARCH.md, HBM section: "exactly half of the bytes of a wide
# coalesced streaming read ... other access widths are uncalibrated: calibrate on a known byte count in your own access pattern"). Default factor 2
# (vector loads of 16 B per lane). Kernels that read their input through the SCALAR cache fetch 64-byte lines that are tallied in full: calibrated on
# knz_rank_inverse_chain_kernel, which reads its n input bytes exactly once with s_load_dwordx4 and stores n bytes: raw FETCH_SIZE = 1.001 n, raw
# WRITE_SIZE = 1.000 n (profiles/r03_final_config4_bench.json). With the factor 2 that kernel showed "1.50x algorithmic" in round 2: an artefact.
FETCH_FACTOR = {"knz_rank_inverse_chain_kernel": 1.0,
                "knz_zrlti_rank_pipe_kernel": 1.0}   # (its chain wave reads the ranks through the scalar cache like the kernel above; the expander wave's 16-byte vector reads of the
                                                     #  ZRLT stream - m of the m + 3 n bytes - are tallied at half: at most m / 2 under-counted)


def kernel_key(name):
    m = re.search(r"knz_\w+(?:<(?:true|false)>)?", name)        # (the bool of a template is part of the name: sizes pass / encoder of the Huffman kernel)
    if not m:
        return name
    k = m.group(0)
    return k if k.startswith("knz_huf_encode_kernel") else k.split("<")[0]


def fpaq_stage_comparison(base, nblocks, enc_ms, dec_ms, m_bytes):
    """FPAQ is one serial chain per block on either side: the honest comparison is chain against chain. The oracle's FPAQ stage alone
    (knzo_entropy_encode / decode) on min(cores, blocks) slices of 4 MiB side by side, one per host thread, against the device kernels'
    rate per chain (the kernels' time is that of the longest chain: every block of the stream in flight at once)."""
    import concurrent.futures as cf
    import oracle_lib as O
    threads = max(1, min(os.cpu_count() or 1, nblocks))
    slices = [np.ascontiguousarray(base[(i * (4 << 20)) % max(len(base) - (4 << 20), 1):][: 4 << 20]) for i in range(threads)]
    O.lib()
    with cf.ThreadPoolExecutor(threads) as ex:                        # (ctypes releases the GIL inside the calls)
        t0 = time.perf_counter()
        enc = list(ex.map(lambda a: O.entropy_encode(O.E_FPAQ, a), slices))
        t1 = time.perf_counter()
        list(ex.map(lambda pr: O.entropy_decode(O.E_FPAQ, pr[0][0], len(pr[1])), zip(enc, slices)))
        t2 = time.perf_counter()
    per = (4 << 20) / 1e6
    cpu_enc, cpu_dec = per / (t1 - t0), per / (t2 - t1)               # MB/s of one thread while all `threads` run
    gpu_enc = m_bytes / nblocks / 1e6 / (enc_ms / 1e3) if enc_ms else 0.0
    gpu_dec = m_bytes / nblocks / 1e6 / (dec_ms / 1e3) if dec_ms else 0.0
    return {"gpu_MBps_per_chain": {"encode": round(gpu_enc, 2), "decode": round(gpu_dec, 2)},
            "cpu_port_MBps_per_thread": {"encode": round(cpu_enc, 2), "decode": round(cpu_dec, 2)}, "cpu_threads_side_by_side": threads,
            "chains_in_flight_on_the_gpu": nblocks,
            "gpu_slower_than_host_per_chain": bool(gpu_enc < cpu_enc or gpu_dec < cpu_dec),
            "gpu_chains_needed_to_match_the_host_threads": {"encode": int(np.ceil(threads * cpu_enc / max(gpu_enc, 1e-9))), "decode": int(np.ceil(threads * cpu_dec / max(gpu_dec, 1e-9)))},
            "what": "FPAQ stage alone, 4 MiB slices of the corpus, one per host thread, against the device kernels (whole blocks behind BWT+RANK+ZRLT, time of the "
                    "longest chain). The device loses per chain (a lone wave issues one instruction per ~2.5 ns); it only wins on blocks in flight"}


def load_pkg():
    spec = importlib.util.spec_from_file_location("kanzi_go_amd", os.path.join(ROOT, "kanzi-go_amd", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(ROOT, "kanzi-go_amd")])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["kanzi_go_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def cpu_baseline(data, transform, entropy, bs, budget_s=20.0):
    """The oracle (C++ restatement of the kanzi-go CPU path, kind 'port') on the host cores, bounded sample."""
    import oracle_lib as O
    cores = os.cpu_count() or 1
    probe = data[: min(len(data), max(bs, 32 << 20))]
    t0 = time.perf_counter()
    c = O.compress(probe, transform, entropy, bs, 0, jobs=cores)
    O.decompress(c, len(probe) + 64, jobs=cores)
    dt = time.perf_counter() - t0
    rate = len(probe) / dt
    n = int(min(len(data), max(len(probe), rate * budget_s)))
    n = max(bs, (n // bs) * bs) if n >= bs else n
    sample = data[:n]
    nblk = (len(sample) + bs - 1) // bs
    t0 = time.perf_counter()
    c = O.compress(sample, transform, entropy, bs, 0, jobs=cores)
    t1 = time.perf_counter()
    back = O.decompress(c, len(sample) + 64, jobs=cores)
    t2 = time.perf_counter()
    assert back == sample.tobytes()
    busy = min(cores, nblk)
    bwt_label = O.bwt_kind() if hasattr(O, "bwt_kind") else "SA-IS (not the reference's divsufsort)"
    return {
        "value": round(len(sample) / 1e6 / (t2 - t0), 2), "unit": "MB/s", "cores": busy, "kind": "port",
        "encode_MBps": round(len(sample) / 1e6 / (t1 - t0), 2), "decode_MBps": round(len(sample) / 1e6 / (t2 - t1), 2),
        "encode_MBps_per_thread": round(len(sample) / 1e6 / (t1 - t0) / busy, 2),
        "sample": f"first {len(sample)} bytes of the corpus ({nblk} blocks), {transform}/{entropy} -b {bs}, round trip, one block per thread "
                  f"({busy} of {cores} host threads busy)",
        "note": "C++ restatement of the kanzi-go CPU path (the Go toolchain is absent from the image: not the Go binary)"
                + (f"; forward BWT stage = {bwt_label}" if "BWT" in transform else ""),
    }


def cpu_baseline_reference(data, transform, entropy, bs, budget_s=14.0):
    """oracle/_ref on the host cores: the reference's OWN code (kanzi-go's .go sources translated mechanically to C++ by tools/go2cpp and compiled
    -O2; bounds checks and panics kept) = kind "reference". One block per thread, as the reference's Writer / Reader run one goroutine per block
    (io/CompressedStream.go:658-698, 1657-1692): every block goes through io.NewWriterWithCtx / io.NewReader on its own thread (ctypes releases the GIL).
    Both directions are the reference's algorithms: DivSufSort forward, inverseBiPSIv2 / inverseMergeTPSI inverse (transform/BWT.go:211-628)."""
    from concurrent.futures import ThreadPoolExecutor
    import ref_lib as R
    R.lib()
    cores = os.cpu_count() or 1
    blocks_all = [data[i:i + bs] for i in range(0, len(data), bs)]

    import ctypes as C
    L = R.lib()
    u8p = C.POINTER(C.c_uint8)
    L.kref_compress.argtypes = [u8p, C.c_uint64, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int64, C.c_int, u8p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.kref_decompress.argtypes = [u8p, C.c_uint64, C.c_uint32, u8p, C.c_uint64, C.POINTER(C.c_uint64)]
    tr, en = transform.encode(), entropy.encode()

    # Only the reference's Writer / Reader are inside the timed calls: the buffers are allocated and touched before (a fresh 6 MiB numpy buffer per call
    # costs about as much as the Huffman codec needs for a block; rounds 1-5a timed it with the call)
    class Job:
        def __init__(self, b):
            self.src = np.ascontiguousarray(b)
            self.cap = len(b) + len(b) // 2 + (1 << 20)
            self.out = np.ones(self.cap, dtype=np.uint8)
            self.back = np.ones(len(b) + 64, dtype=np.uint8)
            self.n = C.c_uint64()
            self.m = C.c_uint64()

    def enc(j):
        rc = L.kref_compress(j.src.ctypes.data_as(u8p), len(j.src), tr, en, bs, 0, 1, len(j.src), 0, j.out.ctypes.data_as(u8p), j.cap, C.byref(j.n))
        if rc != 0:
            raise RuntimeError(f"oracle/_ref compress: rc {rc}")

    def dec(j):
        rc = L.kref_decompress(j.out.ctypes.data_as(u8p), j.n.value, 1, j.back.ctypes.data_as(u8p), len(j.back), C.byref(j.m))
        if rc != 0:
            raise RuntimeError(f"oracle/_ref decompress: rc {rc}")

    # one block on one thread sets the sample: about budget_s of wall clock with every core busy
    j0 = Job(blocks_all[0])
    t0 = time.perf_counter()
    enc(j0)
    dec(j0)
    per_block = max(time.perf_counter() - t0, 1e-3)
    nblk = int(max(1, min(len(blocks_all), (budget_s / per_block) * min(cores, len(blocks_all)))))
    blocks = blocks_all[:nblk]
    nbytes = sum(len(b) for b in blocks)
    busy = min(cores, nblk)
    jobs = [Job(b) for b in blocks]
    with ThreadPoolExecutor(max_workers=busy) as ex:
        list(ex.map(lambda j: None, jobs))                                   # (the pool's threads exist before the clock starts)
        t0 = time.perf_counter()
        list(ex.map(enc, jobs))
        t1 = time.perf_counter()
        list(ex.map(dec, jobs))
        t2 = time.perf_counter()
    backs = [j.back[: j.m.value].tobytes() for j in jobs]
    assert all(bk == b.tobytes() for bk, b in zip(backs, blocks))
    return {
        "value": round(nbytes / 1e6 / (t2 - t0), 2), "unit": "MB/s", "cores": busy, "kind": "reference",
        "encode_MBps": round(nbytes / 1e6 / (t1 - t0), 2), "decode_MBps": round(nbytes / 1e6 / (t2 - t1), 2),
        "encode_MBps_per_thread": round(nbytes / 1e6 / (t1 - t0) / busy, 2), "decode_MBps_per_thread": round(nbytes / 1e6 / (t2 - t1) / busy, 2),
        "sample": f"first {nbytes} bytes of the corpus ({nblk} blocks), {transform}/{entropy} -b {bs}, round trip, one block per thread through the reference's "
                  f"Writer / Reader ({busy} of {cores} host threads busy)",
        "note": "oracle/_ref = kanzi-go's own sources (v2/io, transform, entropy, bitstream, hash) translated mechanically to C++ by tools/go2cpp, g++ -O2, "
                "Go's bounds checks kept; not the Go compiler's code generation (no Go toolchain in the image). Forward BWT = the reference's DivSufSort, "
                "inverse BWT = the reference's inverseBiPSIv2 (8 interleaved chains, int32 links) / inverseMergeTPSI",
    }


def host_hook_rate(K, codec_args, data, bs):
    """PCIe-inclusive rate of knz_encode_blocks / knz_decode_blocks (the calls the cgo shim of Writer.processBlock /
    Reader.processBlock makes): blocks in pageable host memory in, block-local streams in host memory out. Second call timed."""
    from kanzi_go_amd import api as A
    c = K.Codec(*codec_args)
    blocks = [data[i:i + bs] for i in range(0, len(data), bs)]

    def batch(srcs, cap):
        arr = (A._Block * len(srcs))()
        keep = []
        for i, b in enumerate(srcs):
            a = np.ascontiguousarray(b)
            o = np.zeros(cap, dtype=np.uint8)
            keep.append((a, o))
            arr[i].src = a.ctypes.data; arr[i].src_len = len(a); arr[i].dst = o.ctypes.data; arr[i].dst_cap = cap
        return arr, keep

    def timed(fn, arr, n):
        c._chk(fn(c.h, arr, n))
        t0 = time.perf_counter()
        c._chk(fn(c.h, arr, n))
        return time.perf_counter() - t0

    arr, keep = batch(blocks, int(c.L.knz_max_encoded_len(c.cfg.transform, bs)) * 2 + 262144)
    te = timed(c.L.knz_encode_blocks, arr, len(blocks))
    payloads = [keep[i][1][: (arr[i].out_bits + 7) // 8].copy() for i in range(len(blocks))]
    arr2, keep2 = batch(payloads, bs + max(512, bs >> 4))
    td = timed(c.L.knz_decode_blocks, arr2, len(blocks))
    ok = all(bytes(keep2[i][1][: arr2[i].out_bits]) == bytes(blocks[i]) for i in range(len(blocks)))
    c.close()
    n = len(data)
    return {"encode": round(n / 1e6 / te, 1), "decode": round(n / 1e6 / td, 1), "round_trip": round(n / 1e6 / (te + td), 1), "ok": ok,
            "what": "knz_encode_blocks + knz_decode_blocks, all blocks of the stream in pageable host memory (H2D and D2H inside the timed call)"}


def multi_handle_curve(K, codec_args, data, bs, ks, per_handle_blocks=51, rounds=2):
    """The boundary the Go host has: every io.Writer / io.Reader owns one handle and hands it at most `jobs` <= 64 blocks per call
    (io/CompressedStream.go:52,285,621-710). k host threads, one handle each, each calling knz_encode_blocks / knz_decode_blocks on its own batch of
    `per_handle_blocks` blocks in pageable host memory, all at the same time: aggregate MB/s against the number of handles (= blocks in flight)."""
    import threading
    from kanzi_go_amd import api as A
    nb_total = (len(data) + bs - 1) // bs
    out = []
    for k in ks:
        codecs = [K.Codec(*codec_args) for _ in range(k)]
        batches = []
        for t in range(k):                                   # handle t takes blocks [t * per, (t + 1) * per) of the corpus, wrapping around
            blks = []
            for j in range(per_handle_blocks):
                b = (t * per_handle_blocks + j) % nb_total
                a = np.ascontiguousarray(data[b * bs:(b + 1) * bs])
                if len(a) < bs:                               # (a short block may only be the last of a batch: take a full one instead)
                    a = np.ascontiguousarray(data[:bs])
                blks.append(a)
            batches.append(blks)
        cap = int(codecs[0].L.knz_max_encoded_len(codecs[0].cfg.transform, bs)) * 2 + 262144
        enc_arr, keep = [], []
        for t in range(k):
            arr = (A._Block * per_handle_blocks)()
            outs = [np.zeros(cap, dtype=np.uint8) for _ in range(per_handle_blocks)]
            for i, a in enumerate(batches[t]):
                arr[i].src = a.ctypes.data; arr[i].src_len = len(a); arr[i].dst = outs[i].ctypes.data; arr[i].dst_cap = cap
            enc_arr.append(arr); keep.append(outs)

        def run(fn_name, arrs):
            errs = []
            barrier = threading.Barrier(k + 1)

            def work(t):
                c = codecs[t]
                fn = getattr(c.L, fn_name)
                barrier.wait()
                rc = fn(c.h, arrs[t], per_handle_blocks)
                if rc:
                    errs.append(rc)
            ths = [threading.Thread(target=work, args=(t,)) for t in range(k)]
            for th in ths:
                th.start()
            barrier.wait()
            t0 = time.perf_counter()
            for th in ths:
                th.join()
            dt = time.perf_counter() - t0
            assert not errs, errs
            return dt
        te = td = None
        dec_arr, keep2 = [], []
        for r in range(rounds + 1):                           # (round 0 grows the workspaces: untimed)
            dt = run("knz_encode_blocks", enc_arr)
            if r and (te is None or dt < te):                 # (best of the timed rounds, as for the decode below)
                te = dt
            if r == 0:
                for t in range(k):
                    arr = (A._Block * per_handle_blocks)()
                    pays = [keep[t][i][: (enc_arr[t][i].out_bits + 7) // 8].copy() for i in range(per_handle_blocks)]
                    outs = [np.zeros(bs + max(512, bs >> 4), dtype=np.uint8) for _ in range(per_handle_blocks)]
                    for i in range(per_handle_blocks):
                        arr[i].src = pays[i].ctypes.data; arr[i].src_len = len(pays[i]); arr[i].dst = outs[i].ctypes.data; arr[i].dst_cap = len(outs[i])
                    dec_arr.append(arr); keep2.append((pays, outs))
            dt = run("knz_decode_blocks", dec_arr)
            if r and (td is None or dt < td):
                td = dt
        ok = all(bytes(keep2[t][1][i][: dec_arr[t][i].out_bits]) == batches[t][i].tobytes() for t in range(k) for i in range(per_handle_blocks))
        n = k * per_handle_blocks * bs
        out.append({"handles": k, "blocks_in_flight": k * per_handle_blocks, "encode_MBps": round(n / 1e6 / te, 1), "decode_MBps": round(n / 1e6 / td, 1),
                    "round_trip_MBps": round(n / 1e6 / (te + td), 1), "ok": ok})
        for c in codecs:
            c.close()
    return out


def in_process_devices_curve(K, transform, entropy, bs, data, ks, depth, rounds=2):
    """The boundary the Go host has, over several GPUs (row e' of the round-5 verdict): ONE handle of knz_open_devices with k lanes, ONE host thread calling
    knz_encode_blocks / knz_decode_blocks on a batch of `depth` blocks in pageable host memory (what Writer / Reader.EnableGPUDevices(devices, depth) does per
    batch). The library cuts the batch into k contiguous balanced ranges; every lane uploads, runs and downloads its own range at the same time as the others.
    Lane i sits on device i % (devices present): on a one-GPU box the lanes are logical devices of that GPU, on an 8-GPU box k = 8 is one lane per GPU."""
    from kanzi_go_amd import api as A
    L = K.load_library()
    ndev = max(int(L.knz_device_count()), 1)
    nb_total = (len(data) + bs - 1) // bs
    blks = []
    for j in range(depth):
        b = j % nb_total
        a = np.ascontiguousarray(data[b * bs:(b + 1) * bs])
        blks.append(a if len(a) == bs else np.ascontiguousarray(data[:bs]))      # (a short block may only be the last of a batch: take a full one instead)
    out = []
    for k in ks:
        devices = [i % ndev for i in range(k)]
        c = K.Codec(transform, entropy, bs, devices=devices)
        cap = int(c.L.knz_max_encoded_len(c.cfg.transform, bs)) * 2 + 262144
        arr = (A._Block * depth)()
        outs = [np.zeros(cap, dtype=np.uint8) for _ in range(depth)]
        for i, a in enumerate(blks):
            arr[i].src = a.ctypes.data; arr[i].src_len = len(a); arr[i].dst = outs[i].ctypes.data; arr[i].dst_cap = cap
        te = td = None
        lanes_e = lanes_d = None
        arr2 = keep2 = None
        for r in range(rounds + 1):                           # (round 0 grows the workspaces: untimed)
            t0 = time.perf_counter()
            c._chk(c.L.knz_encode_blocks(c.h, arr, depth))
            dt = time.perf_counter() - t0
            if r and (te is None or dt < te):
                te, lanes_e = dt, c.lane_times()
            if r == 0:
                pays = [outs[i][: (arr[i].out_bits + 7) // 8].copy() for i in range(depth)]
                backs = [np.zeros(bs + max(512, bs >> 4), dtype=np.uint8) for _ in range(depth)]
                arr2 = (A._Block * depth)()
                for i in range(depth):
                    arr2[i].src = pays[i].ctypes.data; arr2[i].src_len = len(pays[i]); arr2[i].dst = backs[i].ctypes.data; arr2[i].dst_cap = len(backs[i])
                keep2 = (pays, backs)
            t0 = time.perf_counter()
            c._chk(c.L.knz_decode_blocks(c.h, arr2, depth))
            dt = time.perf_counter() - t0
            if r and (td is None or dt < td):
                td, lanes_d = dt, c.lane_times()
        ok = all(bytes(keep2[1][i][: arr2[i].out_bits]) == blks[i].tobytes() for i in range(depth))
        n = depth * bs
        out.append({"lanes": k, "devices": devices, "blocks_per_call": depth, "encode_MBps": round(n / 1e6 / te, 1), "decode_MBps": round(n / 1e6 / td, 1),
                    "round_trip_MBps": round(n / 1e6 / (te + td), 1), "ok": ok,
                    "lane_ms_encode": [round(t[2], 1) for t in lanes_e], "lane_ms_decode": [round(t[2], 1) for t in lanes_d], "lane_blocks": [t[1] for t in lanes_e]})
        c.close()
    return {"devices_present": ndev, "curve": out}


def pmc_traffic(argv_child, timeout_s=900):
    """HBM bytes per launch for every knz_ kernel: two rocprofv3 passes of THIS command (--kernel-trace --pmc FETCH_SIZE, then
    WRITE_SIZE: separate passes as MI355X_MICROARCH.md prescribes), rocpd databases read with tools/pmc_traffic.py.
    gfx950 correction from the same guide: fetch bytes = 2 * FETCH_SIZE * 1024, WRITE_SIZE (KB) as is."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, "rocprofv3 not found"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pmc_traffic as P
    tmp = tempfile.mkdtemp(prefix="knz_pmc_", dir=os.environ.get("TMPDIR", "/tmp"))
    res = {}
    times = {}
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, counter)
            cmd = [exe, "--kernel-trace", "--pmc", counter, "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__)] + argv_child
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout_s, cwd=tmp,
                               env=dict(os.environ, TMPDIR=os.environ.get("TMPDIR", "/tmp")))
            dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
            if p.returncode != 0 or not dbs:
                return None, f"rocprofv3 --pmc {counter} failed (rc {p.returncode}): {p.stderr[-300:]}"
            res[counter] = P.per_kernel(dbs[0], counter)
            if counter == "FETCH_SIZE":
                try:
                    times = dict(P.per_kernel_time(dbs[0]).items())
                except Exception:   # noqa: BLE001
                    times = {}
        out = {}
        # one entry per kernel INSTANCE (template arguments kept: the instances of a kernel move different amounts); "key" = the name the events use
        for k in set(res["FETCH_SIZE"]) | set(res["WRITE_SIZE"]):
            f, w = res["FETCH_SIZE"].get(k, 0.0), res["WRITE_SIZE"].get(k, 0.0)
            key = kernel_key(k)
            fac = FETCH_FACTOR.get(key, 2.0)
            full = k.replace("void ", "").strip()
            o = {"key": key, "bytes": int(fac * f * 1024 + w * 1024), "fetch_KB_raw": round(f, 1), "write_KB_raw": round(w, 1), "fetch_factor": fac}
            if k in times:
                o["avg_us_under_counters"] = round(times[k][0], 1); o["launches"] = times[k][1]
            out[full] = o
        return out, ("live: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE passes of this command, per-launch averages; bytes = fetch_factor x "
                     "FETCH_SIZE + WRITE_SIZE (factor 2 = the guide's gfx950 correction for wide vector loads, 1 = calibrated scalar-cache reads)")
    except Exception as e:   # noqa: BLE001 (a profiler problem must not cost the bench line)
        return None, f"rocprofv3 pass failed: {e}"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


DUMP_SAMPLE = 4 << 20    # bytes of an output written as they are (float32: 16 MiB per output)
DUMP_CHUNK = 1 << 16     # every byte of it also enters the sum of its 64 KiB chunk (float64)


def dump_outputs(dirname, outputs):
    """--dump-outputs: the byte tensors the timed path handed its caller in the last step, as DIR/<name>.npy (float32 byte values: all of them up to
    DUMP_SAMPLE bytes, else DUMP_SAMPLE positions drawn with a fixed seed, sorted), DIR/<name>_chunk_sums.npy (float64 sums of every DUMP_CHUNK bytes,
    the last chunk short) and DIR/sizes.npy (float64 byte count of each output, in the order given). Two builds that write the same bytes write the
    same files; about 33 MB for the two outputs of a step."""
    import torch
    os.makedirs(dirname, exist_ok=True)
    sizes = []
    for name, t in outputs.items():
        n = int(t.numel())
        sizes.append(n)
        if n > DUMP_SAMPLE:
            idx = np.sort(np.random.default_rng(20240607).integers(0, n, DUMP_SAMPLE))
            sample = t[torch.from_numpy(idx).to(t.device)]
        else:
            sample = t
        np.save(os.path.join(dirname, f"{name}.npy"), sample.cpu().numpy().astype(np.float32))
        full = n - n % DUMP_CHUNK
        sums = t[:full].view(-1, DUMP_CHUNK).sum(dim=1, dtype=torch.int64)
        if full < n:
            sums = torch.cat([sums, t[full:].sum(dtype=torch.int64).view(1)])
        np.save(os.path.join(dirname, f"{name}_chunk_sums.npy"), sums.cpu().numpy().astype(np.float64))
    np.save(os.path.join(dirname, "sizes.npy"), np.array(sizes, dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 10; 1 for --config fpaq, whose step takes half a minute): the chains of the default "
                                                            "configuration move by a few per cent from step to step, three steps were too few for a steady mean")
    ap.add_argument("--warmup", type=int, default=None, help="untimed steps in front (default 3; 0 for --config fpaq)")
    ap.add_argument("--config", default="bwt", choices=sorted(CONFIGS))
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"], help="N>1: ONE fixed job (the BASELINE corpus) split over the GPUs (strong, default: the figure BASELINE.json's "
                                                                                    "metric and north_star name; the weak figure rides along as roofline.weak_value_MBps) or one corpus copy per GPU in one stream (weak)")
    ap.add_argument("--no-weak", action="store_true", help="N>1, strong, --full: skip the second (weak-scaling) timed region")
    ap.add_argument("--size", type=int, default=0, help="override the corpus size (debug; the defaults are the BASELINE sizes: 211957760 / 10^9 for fpaq)")
    ap.add_argument("--block-size", type=int, default=0, help="override the block size (debug)")
    ap.add_argument("--transform", default="", help="override the transform sequence of the config, e.g. LZP or BWT+SRT+ZRLT (debug)")
    ap.add_argument("--entropy", default="", help="override the entropy codec of the config (debug)")
    ap.add_argument("--copies", type=int, default=1, help="corpus copies in the one stream (single-GPU saturation curve: MB/s against blocks in flight)")
    ap.add_argument("--force-dist", action="store_true", help="take the N > 1 code path (process group, sharded encode, gather, assembly, collectives) at world size 1: "
                                                              "puts RCCL under bench.py on a one-GPU box (debug / pre-flight of the driver's multi-GPU run)")
    ap.add_argument("--handles", default="", help="e.g. 1,2,4,8: instead of the step, the multi-handle curve of the host-pointer boundary (k threads x one handle x 51 blocks per call), one JSON object")
    ap.add_argument("--in-process-devices", default="", help="e.g. 1,2,4,8: instead of the step, the host-pointer boundary through ONE handle of knz_open_devices with k lanes "
                                                              "(lane i on device i %% devices present: logical devices on a one-GPU box, one lane per GPU on an 8-GPU box), one JSON object")
    ap.add_argument("--depth", type=int, default=0, help="--in-process-devices: blocks per knz_encode_blocks / knz_decode_blocks call (default: the blocks of the corpus)")
    ap.add_argument("--corpus", default="", help="a file to use instead of the synthetic corpus (the real silesia.tar / enwik9 where a driver has them); `data` says \"file\"")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--no-pmc", action="store_true", help="skip the two rocprofv3 PMC passes (roofline.traffic = null)")
    ap.add_argument("--no-host-hook", action="store_true", help="skip the PCIe-inclusive host-pointer measurement")
    ap.add_argument("--full", action="store_true", help="also measure and check what the headline figure does not need: the bit-exactness checks against the oracle and "
                                                        "the reference-written stream, the rocprofv3 PMC passes, the host-pointer hook, the CPU baselines, the FPAQ stage "
                                                        "comparison and (N > 1, strong) the weak-scaling region (each still subject to its --no-* switch)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="after the timed steps, write what the last step handed its caller (the .knz stream and the "
                                                                      "decoded bytes) to DIR/<name>.npy as float32 / float64 (a fixed, seeded sample of each plus "
                                                                      "the sums of its 64 KiB chunks)")
    args = ap.parse_args()
    if args.steps is None:
        args.steps = 1 if args.config == "fpaq" else 10
    if args.warmup is None:
        args.warmup = 0 if args.config == "fpaq" else 3
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.handles or args.in_process_devices:
        # several handles = several streams: the HIP runtime multiplexes all streams of a process onto GPU_MAX_HW_QUEUES (default 4) hardware queues and
        # kernels of streams that share a queue run one after the other. libknz_gpu asks for 32 when it is loaded (unless the host chose a value); under
        # this harness torch brings the HIP runtime up first, so the same request is made here, before that
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")

    import torch
    import torch.distributed as dist
    import bench_corpus

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    emu = os.environ.get("KNZ_BENCH_EMU") == "1"          # test harness only, see the module docstring
    multi = world > 1 or args.force_dist                  # the distributed code path
    # stdout carries ONE JSON line and nothing else: RCCL prints a version banner to the C stdout of every rank (seen behind the JSON line when the
    # buffer is flushed at exit), so with a process group every rank sends file descriptor 1 to stderr and rank 0 keeps the real one for its line
    json_out = sys.stdout
    if multi:
        sys.stdout.flush()
        real = os.dup(1)
        os.dup2(2, 1)
        json_out = os.fdopen(real, "w")
    if args.force_dist and world == 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
    if emu:
        import knz
        dev = torch.device("cpu")
        sync = lambda: None
        if multi:
            dist.init_process_group("gloo")
        K = knz.package()
        lib = knz.emu_library()
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU: the product path has no CPU fallback")
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        sync = torch.cuda.synchronize
        if multi:
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            dist.init_process_group("nccl", device_id=dev)
        K = load_pkg()
        K.build_library()
        lib = None
    from kanzi_go_amd import dist as kd
    transform, entropy, bs, cfg_idx, corpus = CONFIGS[args.config]
    transform, entropy = args.transform or transform, args.entropy or entropy
    bs = args.block_size or bs

    if args.corpus:
        base = np.fromfile(args.corpus, dtype=np.uint8)
        if args.size:
            base = base[:args.size]
        base_size = len(base)
        corpus_name = "file " + os.path.basename(args.corpus)
    elif corpus == "enwik":
        base_size = args.size or 1_000_000_000
        base = bench_corpus.s_enwik(base_size)
        corpus_name = "S-enwik"
    else:
        base_size = args.size or bench_corpus.SILESIA_SIZE
        base = bench_corpus.s_silesia(base_size)
        corpus_name = "S-silesia"
    from types import SimpleNamespace

    def tiled(a, b):                                         # bytes [a, b) of the corpus repeated back to back
        parts = []
        while a < b:
            o = a % base_size
            take = min(b - a, base_size - o)
            parts.append(base[o:o + take])
            a += take
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)

    def dev_zeros(n):                                        # 16-byte aligned (the emulator's "device" memory is host memory)
        t = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
        return t[(-t.data_ptr()) % 16:][:n]

    if args.handles:
        ks = [int(x) for x in args.handles.split(",") if x]
        per = 51 if bs <= (4 << 20) else 26                   # one Writer's batch: jobs <= 64 blocks (the default job's block count per call)
        curve = multi_handle_curve(K, (transform, entropy, bs, 0, local_rank), base, bs, ks, per_handle_blocks=per)
        print(json.dumps({"what": "knz_encode_blocks / knz_decode_blocks from k host threads, one handle each, pageable host memory, all calls at the same time",
                          "config": f"-t {transform} -e {entropy} -b {bs >> 20}m", "blocks_per_call": per, "curve": curve}), file=json_out, flush=True)
        return
    if args.in_process_devices:
        ks = [int(x) for x in args.in_process_devices.split(",") if x]
        depth = args.depth or (base_size + bs - 1) // bs * max(1, args.copies)
        res = in_process_devices_curve(K, transform, entropy, bs, base, ks, depth)
        res.update({"what": "ONE handle of knz_open_devices with k lanes, one host thread, knz_encode_blocks / knz_decode_blocks on `blocks_per_call` blocks in pageable host memory "
                            "(H2D and D2H inside the timed calls); lane i on device i % devices_present",
                    "config": f"-t {transform} -e {entropy} -b {bs >> 20}m", "corpus": corpus_name})
        print(json.dumps(res), file=json_out, flush=True)
        return
    codec = K.Codec(transform, entropy, bs, device=local_rank, lib=lib)

    def make_job(strong_):
        """The buffers of one workload: strong = ONE job (the BASELINE corpus) whatever N; weak = one corpus copy per GPU, still one stream."""
        j = SimpleNamespace()
        j.size = (base_size if strong_ else base_size * world) * max(1, args.copies)
        j.nblocks = (j.size + bs - 1) // bs
        lo_b, hi_b = kd.block_range(j.nblocks, rank, world)
        j.per = kd.max_blocks_per_rank(j.nblocks, world)
        lo, hi = min(lo_b * bs, j.size), min(hi_b * bs, j.size)
        my = tiled(lo, hi)
        j.n_my = len(my)
        j.d_src = dev_zeros(max(j.n_my, 16))
        if j.n_my:
            j.d_src[:j.n_my] = torch.from_numpy(np.ascontiguousarray(my)).to(dev)
        j.cap = (j.per * bs + (j.per * bs) // 2 + (1 << 20) + 15) & ~15
        j.d_seg = dev_zeros(j.cap)
        j.d_back = dev_zeros(j.n_my + 4096)
        j.d_stream = dev_zeros(j.size + j.size // 2 + (1 << 20)) if rank == 0 and multi else None
        j.stage = {"enc_transform": 0.0, "enc_entropy": 0.0, "enc_layout": 0.0, "enc_gather": 0.0, "dec_walk": 0.0, "dec_entropy": 0.0, "dec_transform": 0.0}
        j.kern_ms, j.kern_launches = {}, {}
        j.t_enc = j.t_dec = 0.0
        j.result = {}
        return j

    strong = args.scaling == "strong" or world == 1
    job = make_job(strong)
    # the steps run on a stream of their own (non-blocking): a NULL stream would mean the handle's own stream, which is ordered against
    # the legacy default stream and pays that ordering on every launch (visible on the microsecond-scale configs)
    bench_stream = None if emu else torch.cuda.Stream(device=dev)
    stream = 0 if emu else bench_stream.cuda_stream

    def add_kernels(j, codec_):
        for name, ms in codec_.last_kernel_times():
            k = kernel_key(name)
            j.kern_ms[k] = j.kern_ms.get(k, 0.0) + ms
            j.kern_launches[k] = j.kern_launches.get(k, 0) + 1

    def one_step(j, timed):
        result, stage = j.result, j.stage
        t0 = time.perf_counter()
        if not multi:
            nb = codec.dev_compress(j.d_src.data_ptr(), j.n_my, j.d_seg.data_ptr(), j.cap, header_input_size=j.size, stream=stream)
            result["stream_bytes"] = nb
        else:
            # every rank encodes its blocks; the gather of the segments to rank 0 over RCCL/xGMI is started and stays in flight
            # while the rank decodes its own segment (which needs nothing from the others); then rank 0 assembles the stream
            pending, nbits = kd.sharded_compress_begin(codec, j.d_src, j.n_my, j.d_seg, j.size, j.d_stream if rank == 0 else j.d_seg, stream=stream)
            result["seg_bits"] = nbits
        tm = codec.last_timing()
        if timed:
            add_kernels(j, codec)
        if not multi:
            sync()
        t1 = time.perf_counter()
        if not multi:
            nd = codec.dev_decompress(j.d_seg.data_ptr(), result["stream_bytes"], j.d_back.data_ptr(), j.d_back.numel(), stream=stream)
        else:
            nd = codec.dev_decompress_blocks(j.d_seg.data_ptr(), result["seg_bits"], j.d_back.data_ptr(), j.d_back.numel(), stream=stream) if j.n_my else 0
        td = codec.last_timing() if (not multi or j.n_my) else [0.0] * 4
        if timed and (not multi or j.n_my):
            add_kernels(j, codec)
        sync()
        t2 = time.perf_counter()
        if multi:
            nb, _ = pending.finish()
            sync()
            t3 = time.perf_counter()
            t0 -= (t3 - t2)                        # the assembly belongs to the encode side of the step
            if rank == 0:
                result["stream_bytes"] = nb
        assert nd == j.n_my, (nd, j.n_my)
        if timed:
            j.t_enc += t1 - t0
            j.t_dec += t2 - t1
            stage["enc_transform"] += tm[0]; stage["enc_entropy"] += tm[1]; stage["enc_layout"] += tm[2]; stage["enc_gather"] += tm[3]
            stage["dec_walk"] += td[0]; stage["dec_entropy"] += td[1]; stage["dec_transform"] += td[2]

    def timed_region(j):
        """W untimed steps, then EXACTLY K steps between barrier + synchronize on both sides; the MAX over the ranks."""
        for _ in range(args.warmup):
            one_step(j, False)
        if multi:
            dist.barrier()
        sync()
        t_start = time.perf_counter()
        for _ in range(args.steps):
            one_step(j, True)
        sync()
        if multi:
            dist.barrier()
        el = time.perf_counter() - t_start
        if multi:
            tt = torch.tensor([el, j.t_enc, j.t_dec], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            el, j.t_enc, j.t_dec = [float(x) for x in tt.tolist()]
        return el

    sync()
    if bench_stream is not None:
        torch.cuda.set_stream(bench_stream)                   # torch.distributed orders its collectives against the current stream
    elapsed = timed_region(job)
    size, nblocks, n_my, result, stage, kern_ms, kern_launches = job.size, job.nblocks, job.n_my, job.result, job.stage, job.kern_ms, job.kern_launches
    t_enc, t_dec, d_src, d_seg, d_back, d_stream = job.t_enc, job.t_dec, job.d_src, job.d_seg, job.d_back, job.d_stream
    if args.dump_outputs and rank == 0:
        # (N > 1: the assembled stream and rank 0's own decoded blocks)
        stream_out = (d_seg if not multi else d_stream)[:result["stream_bytes"]]
        dump_outputs(args.dump_outputs, {"stream": stream_out, "decoded": d_back[:n_my]})
    rank_kernel_max = None
    if multi:
        # the slowest rank's time per kernel: what the SCALE line's shape is made of (a chain kernel is flat in the number of blocks a rank owns)
        names = sorted(kern_ms)
        gathered = [None] * world
        dist.all_gather_object(gathered, {k: kern_ms[k] for k in names})
        allk = sorted(set().union(*[set(g) for g in gathered]))
        rank_kernel_max = {k: max(g.get(k, 0.0) for g in gathered) for k in allk}

    ok_roundtrip = bool(torch.equal(d_back[:n_my], d_src[:n_my])) if n_my else True
    if multi:                                            # every rank's decode must have come back right
        okt = torch.tensor([1 if ok_roundtrip else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(okt, op=dist.ReduceOp.MIN)
        ok_roundtrip = bool(int(okt.item()))

    # N > 1, strong, --full: the weak-scaling figure (one corpus copy per GPU in one stream) rides along as a second timed region of the same shape
    weak = None
    if args.full and multi and world > 1 and strong and not args.no_weak:
        wj = make_job(False)
        w_el = timed_region(wj)
        w_ok = bool(torch.equal(wj.d_back[:wj.n_my], wj.d_src[:wj.n_my])) if wj.n_my else True
        weak = {"value": round(wj.size / 1e6 / (w_el / max(args.steps, 1)), 2), "ms_per_step": round(w_el / max(args.steps, 1) * 1e3, 3), "size": wj.size,
                "blocks": wj.nblocks, "roundtrip_ok_rank0": w_ok}
        del wj

    if rank == 0:
        K_ = max(args.steps, 1)
        ms = elapsed / K_ * 1e3
        C_bytes = result["stream_bytes"]
        counts = kd.blocks_per_rank(nblocks, world)
        out = {
            "metric": "encode+decode MB/s (round trip of the whole stream, uncompressed 10^6 B per second)",
            "value": round(size / 1e6 / (elapsed / K_), 2), "unit": "MB/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True,
            "scaling": args.scaling, "vs_baseline": None, "dtype": "u8",
            "data": ("file" if args.corpus else "synthetic") if not emu else "synthetic (EMULATOR TEST HARNESS on CPU: not a measurement)",
            "config": {"workload": (f"BASELINE.json configs[{cfg_idx}]" if args.config != "l5" else "kanzi-go preset -l 5 (README.md:79; not a BASELINE.json config)") +
                                   f": -t {transform} -e {entropy} -b {bs >> 20}m on {corpus_name} "
                                   f"(one .knz stream of {size} B" + ("" if size == base_size else f" = {size // base_size} copies of {base_size} B") + (", bench_corpus.py)" if not args.corpus else ")"),
                       "blocks": nblocks, "block_size": bs,
                       "parallelism": f"contiguous block ranges over {world} GPU(s) ({','.join(str(x) for x in counts)} blocks), segments gathered to rank 0"},
            "encode_MBps": round(size / 1e6 / (t_enc / K_), 2), "decode_MBps": round(size / 1e6 / (t_dec / K_), 2),
            "compressed_bytes": int(C_bytes), "roundtrip_ok": ok_roundtrip,
        }
        if args.config in PUBLISHED and not (args.transform or args.entropy):
            out["reference_published"] = PUBLISHED[args.config]
        # roofline of the dominant KERNEL: HIP events around its launches on the launch stream (knz_last_kernel_times)
        n_local = n_my
        c_local = (result.get("seg_bits", C_bytes * 8) + 7) // 8 if multi else C_bytes
        try:
            m_local = codec.last_counter(1) or n_local            # bytes behind the transforms (entropy coder input) of the last encode batch
        except Exception:   # noqa: BLE001
            m_local = n_local
        per_launch = {k: v / K_ for k, v in stage.items()}
        roof = {"bound": "hbm", "kernel": None, "achieved": 0.0, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": 0.0, "traffic": None,
                "all_stage_ms": {k: round(v, 4) for k, v in per_launch.items()}}
        # probes named "phase:..." bracket several launches (the stages of the suffix sort): reported, never the dominant KERNEL
        phase_ms = {k[6:]: v for k, v in kern_ms.items() if k.startswith("phase:")}
        for k in list(kern_ms):
            if k.startswith("phase:"):
                del kern_ms[k]
        if phase_ms:
            roof["phase_ms_per_step"] = {k: round(v / K_, 3) for k, v in sorted(phase_ms.items(), key=lambda kv: -kv[1])}
        # bytes that entered each transform stage of the last encode batch (knz_last_counter 8 + i): a kernel is priced on what ITS stage saw
        stage_in = {}
        if not emu and transform != "NONE":
            for i, tok in enumerate(transform.split("+")):
                try:
                    stage_in[tok] = int(codec.last_counter(8 + i)) or n_local
                except Exception:   # noqa: BLE001
                    stage_in[tok] = n_local

        def n_for(kernel):
            for prefixes, toks in ((("knz_bwt_", "knz_ss_", "knz_sg_", "knz_sl_"), ("BWT",)), (("knz_rank_", "knz_sbrt_", "knz_mtft_", "knz_zrlti_rank_pipe"), ("RANK", "MTFT", "SRT")),
                                   (("knz_zrlt",), ("ZRLT",)), (("knz_lzp_",), ("LZP",)), (("knz_lz",), ("LZ", "LZX")), (("knz_text_",), ("TEXT",)),
                                   (("knz_utf_",), ("UTF",)), (("knz_srt_",), ("SRT",))):
                if kernel.startswith(prefixes):
                    for t in toks:
                        if t in stage_in:
                            return stage_in[t]
            return n_local

        def alg_bytes(kernel):
            f = KERNEL_BYTES.get(kernel)
            return None if f is None else f(n_for(kernel), m_local, c_local)
        if stage_in:
            roof["stage_input_bytes"] = stage_in
        if kern_ms:
            dom = max(kern_ms, key=lambda k: kern_ms[k])
            avg_ms = kern_ms[dom] / max(kern_launches[dom], 1)
            launches_per_step = kern_launches[dom] / K_
            alg = (alg_bytes(dom) if alg_bytes(dom) is not None else n_local + c_local) / max(launches_per_step, 1)
            ach = alg / 1e9 / (avg_ms / 1e3) if avg_ms > 0 else 0.0
            roof.update({"kernel": dom, "achieved": round(ach, 3), "frac": round(ach / HBM_PEAK_GBS, 6),
                         "algorithmic_bytes_per_launch": int(alg), "avg_launch_ms": round(avg_ms, 4), "launches_per_step": launches_per_step,
                         "timing": "HIP events around the kernel's launches on the launch stream (knz_last_kernel_times)",
                         "kernel_ms_per_step": {k: round(v / K_, 3) for k, v in sorted(kern_ms.items(), key=lambda kv: -kv[1])[:12]},
                         "kernel_launches_per_step": {k: round(kern_launches[k] / K_, 2) for k, v in sorted(kern_ms.items(), key=lambda kv: -kv[1])[:12]}})
            if args.full and not args.no_pmc and not multi and not emu:
                # (fpaq: one 10^9-byte step is ~35 s of two serial chains per block; its counter passes run a single step)
                child = ["--config", args.config, "--steps", "1" if args.config == "fpaq" else "2", "--warmup", "0" if args.config == "fpaq" else "1",
                         "--no-cpu-baseline", "--no-verify", "--no-pmc", "--no-host-hook"]
                for flag, val in (("--size", args.size), ("--block-size", args.block_size), ("--copies", args.copies if args.copies > 1 else 0)):
                    if val:
                        child += [flag, str(val)]
                for flag, val in (("--transform", args.transform), ("--entropy", args.entropy)):
                    if val:
                        child += [flag, val]
                tr, how = pmc_traffic(child)
                roof["traffic_source"] = how
                by_key = {}
                for full, t in (tr or {}).items():
                    by_key.setdefault(t["key"], []).append(full)
                if tr is not None and dom in by_key:
                    # (a kernel with several instances: launch-weighted mean of their per-launch bytes)
                    inst = by_key[dom]
                    wsum = sum(max(tr[f].get("launches", 1), 1) for f in inst)
                    domBytes = sum(tr[f]["bytes"] * max(tr[f].get("launches", 1), 1) for f in inst) / max(wsum, 1)
                    roof["traffic"] = int(domBytes)
                    roof["traffic_over_algorithmic"] = round(domBytes / max(alg, 1), 3)
                    roof["traffic_counters"] = {k: round(sum(tr[f][k] * max(tr[f].get("launches", 1), 1) for f in inst) / max(wsum, 1), 1) for k in ("fetch_KB_raw", "write_KB_raw")}
                    roof["traffic_counters"]["fetch_factor"] = tr[inst[0]]["fetch_factor"]
                if tr is not None:
                    # every kernel instance of the step that moves at least 1 MB per launch or runs for 50 us: time (HIP events of this run where the
                    # launch is probed and the kernel has one instance, else the trace of the counter pass), algorithmic bytes of ONE launch (the stage's
                    # bytes / launches per step), counter bytes per launch, and what the counters say about the HBM rate while the kernel runs
                    table = []
                    steps_child = 1 if args.config == "fpaq" else 3           # (the child runs warm-up + steps launches of everything)
                    for full, t in tr.items():
                        k = t["key"]
                        if not k.startswith("knz_"):
                            continue
                        single = len(by_key[k]) == 1
                        ev = single and k in kern_ms
                        lps = kern_launches[k] / K_ if ev else t.get("launches", 0) / steps_child
                        ms = kern_ms[k] / max(kern_launches[k], 1) if ev else t.get("avg_us_under_counters", 0.0) / 1e3
                        if ms <= 0 or (t["bytes"] < 1e6 and ms < 0.05):
                            continue
                        ab = alg_bytes(k) if single else None
                        row = {"kernel": full if not single else k, "avg_launch_ms": round(ms, 4), "launches_per_step": round(lps, 2), "ms_per_step": round(ms * lps, 3),
                               "timing": "events" if ev else "trace of the counter pass",
                               "counter_bytes_per_launch": int(t["bytes"]), "counter_GBps": round(t["bytes"] / 1e9 / (ms / 1e3), 1),
                               "counter_frac_of_peak": round(t["bytes"] / 1e9 / (ms / 1e3) / HBM_PEAK_GBS, 4)}
                        if ab is not None and lps > 0:
                            row["algorithmic_bytes_per_launch"] = int(ab / lps)
                            row["algorithmic_GBps"] = round(ab / lps / 1e9 / (ms / 1e3), 1)
                            row["frac"] = round(ab / lps / 1e9 / (ms / 1e3) / HBM_PEAK_GBS, 6)
                            row["traffic_over_algorithmic"] = round(t["bytes"] / max(ab / lps, 1), 3)
                        table.append(row)
                    roof["per_kernel"] = sorted(table, key=lambda r: -r["ms_per_step"])[:40]
        # the figures north_star's targets are quoted on, as scalars where the driver's parser keeps them
        roof["encode_MBps"] = out["encode_MBps"]; roof["decode_MBps"] = out["decode_MBps"]
        roof["encode_ms"] = round(t_enc / K_ * 1e3, 3); roof["decode_ms"] = round(t_dec / K_ * 1e3, 3)
        if weak is not None:
            roof["weak_value_MBps"] = weak["value"]; roof["weak_ms_per_step"] = weak["ms_per_step"]; roof["weak_blocks"] = weak["blocks"]
            out["weak_scaling"] = weak
        out["roofline"] = roof
        if rank_kernel_max:
            out["kernel_ms_per_step_max_over_ranks"] = {k: round(v / K_, 3) for k, v in sorted(rank_kernel_max.items(), key=lambda kv: -kv[1])[:10]}
        if not emu:
            # blocks the parallel kernels handed to their exact one-wave fallbacks in the last batch (0 on everything an encoder wrote so far)
            fb = {}
            toks = transform.split("+")
            if "TEXT" in toks:
                fb["text_chain_blocks"] = int(codec.last_counter(2))
            if "LZ" in toks or "LZX" in toks:
                fb["lz_inverse_one_wave_blocks"] = int(codec.last_counter(3))
                fb["lz_forward_one_wave_blocks"] = int(codec.last_counter(4))
                fb["lz_forward_rounds"] = int(codec.last_counter(5))
            if fb:
                out["fallback_counters_last_batch"] = fb
        if entropy == "FPAQ":
            out["chain_bound"] = True          # one binary arithmetic-coding chain per block by format: flat in the block count
            if args.full and not multi and not emu and not args.no_cpu_baseline:
                try:
                    out["fpaq_stage"] = fpaq_stage_comparison(base, nblocks, kern_ms.get("knz_fpaq_encode_kernel", 0.0) / K_, kern_ms.get("knz_fpaq_decode_kernel", 0.0) / K_, m_local)
                except Exception as e:   # noqa: BLE001
                    out["fpaq_stage"] = {"error": str(e)}
        if entropy == "HUFFMAN" and not emu:
            # the single-launch walk + decode hands a chunk to the serial kernel when a decoder gives up waiting for its walker:
            # 0 for every stream a kanzi encoder wrote unless the dispatch order went against the kernel
            out["huffman_serial_chunks_last_decode"] = int(codec.last_counter(0))
        if args.full and not args.no_verify:
            import oracle_lib as O
            exp = O.compress(tiled(0, size), transform, entropy, bs, 0, jobs=os.cpu_count() or 1)
            got = (d_seg if not multi else d_stream)[:C_bytes].cpu().numpy().tobytes()
            out["bit_exact_vs_oracle"] = bool(got == exp)
            # ... and with the stream the REFERENCE's Writer writes for this very input (tests/golden/ref_streams/fullsize_manifest.json: oracle/_ref over the same
            # corpus in the build container, by length + sha256; tools/make_ref_fullsize_vectors.py). null: no vector for this workload
            out["bit_exact_vs_reference"] = None
            try:
                import hashlib
                man = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_streams", "fullsize_manifest.json")))
                for c in man["cases"]:
                    if (c["transform"], c["entropy"], c["block_size"], c["input_bytes"]) == (transform, entropy, bs, size) and not args.corpus:
                        same_input = hashlib.sha256(tiled(0, size).tobytes()).hexdigest() == c["input_sha256"]
                        out["bit_exact_vs_reference"] = bool(same_input and len(got) == c["stream_bytes"] and hashlib.sha256(got).hexdigest() == c["sha256"])
                        out["reference_vector"] = {"case": c["name"], "sha256": c["sha256"], "stream_bytes": c["stream_bytes"], "producer": man["producer"]}
            except Exception as e:   # noqa: BLE001
                out["reference_vector_error"] = str(e)
            out["parity_note"] = ("oracle = in-repo C++ restatement of kanzi-go, pinned by oracle/_ref (the reference's own .go sources translated mechanically to C++ and compiled: "
                                  "tests/test_ref_build.py, tests/test_ref_streams.py; DESIGN.md section 2)")
        if args.full and not multi and not emu and not args.no_host_hook:
            try:
                out["host_hook_MBps"] = host_hook_rate(K, (transform, entropy, bs, 0, local_rank), base[:size] if size <= base_size else tiled(0, size), bs)
                # (the metric of SURVEY 8d "including H2D / D2H": never `value`, kept beside it)
                roof["host_hook_round_trip_MBps"] = out["host_hook_MBps"]["round_trip"]
                roof["host_hook_encode_MBps"] = out["host_hook_MBps"]["encode"]; roof["host_hook_decode_MBps"] = out["host_hook_MBps"]["decode"]
            except Exception as e:   # noqa: BLE001
                out["host_hook_MBps"] = {"error": str(e)}
        if args.full and not args.no_cpu_baseline and not multi:
            cb = None
            try:
                import ref_lib
                if ref_lib.available():
                    cb = cpu_baseline_reference(base, transform, entropy, bs)
                    port = cpu_baseline(base, transform, entropy, bs, budget_s=8.0)      # the hand-written oracle beside it (rounds 1-4 quoted this one)
                    cb["port"] = {k: port[k] for k in ("value", "encode_MBps", "decode_MBps", "cores", "sample")}
                    cb["port_encode_MBps"] = port["encode_MBps"]; cb["port_decode_MBps"] = port["decode_MBps"]
            except Exception as e:   # noqa: BLE001  (a missing oracle/_ref must not cost the bench line: the port is the fallback)
                cb = None
                out["cpu_baseline_reference_error"] = str(e)
            if cb is None:
                cb = cpu_baseline(base, transform, entropy, bs)
            out["cpu_baseline"] = cb
            # north_star's target: encode >= 10x the CPU encode of the same configuration (vs_baseline stays null: BASELINE.md holds no published number for this metric)
            cb["gpu_encode_MBps"] = out["encode_MBps"]; cb["gpu_decode_MBps"] = out["decode_MBps"]
            cb["gpu_encode_over_cpu_encode"] = round(out["encode_MBps"] / max(cb["encode_MBps"], 1e-9), 2)
            cb["gpu_decode_over_cpu_decode"] = round(out["decode_MBps"] / max(cb["decode_MBps"], 1e-9), 2)
        print(json.dumps(out), file=json_out, flush=True)
    if multi:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
