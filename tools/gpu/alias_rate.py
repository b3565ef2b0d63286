#!/usr/bin/env python3
"""Rates of the PACK / DNA stage (alias.hip) on the device, next to two yardsticks taken in the same run: the ZRLT stage on the same bytes
and the reference's AliasCodec (oracle/_ref) on 16 host processes, one block each at a time. Then the -l 2 preset DNA+LZ&HUFFMAN at 4 MiB
blocks against the reference's Writer / Reader with 16 jobs and against LZ&HUFFMAN on the device. Device figures: HIP events around the
batch's transform stage (knz_last_timing), data resident on the device, median of 10 after 3 warm-ups. Prints one JSON object.
  python tools/gpu/alias_rate.py [--reps 10] [--warmup 3] [--quick]"""
import argparse
import json
import multiprocessing as mp
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

BS = 4 << 20
_BLOCKS = None


def dna_input(nblocks=64):
    rng = np.random.default_rng(2)
    a = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), nblocks * BS)
    a[60::61] = 10
    return a


def _ref_job(args):
    import ref_lib as R
    tid, i = args
    R.set_ctx(BS, R.entropy_type("NONE"), 0)
    blk = _BLOCKS[i]
    t0 = time.perf_counter()
    f = R.transform_forward(tid, blk)
    t1 = time.perf_counter()
    if f is not None:
        R.transform_inverse(tid, f, len(blk) + 1024)
    return t1 - t0, time.perf_counter() - t1, f is not None


def ref_rates(data, tid):
    """wall time of all blocks over 16 worker processes (forked before the GPU is touched)"""
    global _BLOCKS
    _BLOCKS = [data[i: i + BS] for i in range(0, len(data), BS)]
    with mp.get_context("fork").Pool(16) as pool:
        pool.map(_ref_job, [(tid, 0)] * 16)                                # workers up, library loaded
        t0 = time.perf_counter()
        res = pool.map(_ref_job, [(tid, i) for i in range(len(_BLOCKS))], chunksize=1)
        wall = time.perf_counter() - t0
    fw, iv = sum(r[0] for r in res), sum(r[1] for r in res)
    # the pool ran forward and inverse of a block back to back: split the wall time by the shares of the summed times
    return {"forward_GBps": len(data) / 1e9 / (wall * fw / (fw + iv)), "inverse_GBps": (len(data) / 1e9 / (wall * iv / (fw + iv))) if iv > 0 else None,
            "blocks_applied": sum(1 for r in res if r[2]), "blocks": len(res)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="8 blocks per input, no host yardsticks (for a profiler run)")
    a = ap.parse_args()
    import bench_corpus
    inputs = {"dna_64x4MiB": dna_input(8 if a.quick else 64), "s_silesia": bench_corpus.s_silesia()[: 8 * BS] if a.quick else bench_corpus.s_silesia()}
    out = {"block_size": BS, "reps": a.reps, "warmup": a.warmup, "inputs": {k: int(len(v)) for k, v in inputs.items()}, "stage": {}, "preset": {}}
    import ref_lib as R
    if not a.quick:                                                        # host yardsticks first: the workers are forked while no GPU is open
        for name, data in inputs.items():
            for tname, tid in (("PACK", 18), ("DNA", 19)):
                out["stage"].setdefault(name, {})[tname + "_reference_16_processes"] = ref_rates(data, tid)
        for name, data in inputs.items():
            t0 = time.perf_counter(); s = R.compress(data, "DNA+LZ", "HUFFMAN", BS, 0, 16); t1 = time.perf_counter()
            back = R.decompress(s, len(data) + 64, 16); t2 = time.perf_counter()
            assert back == data.tobytes()
            out["preset"].setdefault(name, {})["reference_16_jobs"] = {"encode_MBps": len(data) / 1e6 / (t1 - t0), "decode_MBps": len(data) / 1e6 / (t2 - t1), "bytes": len(s)}
    import torch
    import knz
    K = knz.package()
    K.build_library()
    dev = torch.device("cuda", 0)

    def stage(transform, entropy, data, whole=False):
        n = len(data)
        c = K.Codec(transform, entropy, BS)
        src = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
        dst = torch.zeros(n + n // 2 + (1 << 20), dtype=torch.uint8, device=dev)
        back = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
        enc, dec, encw, decw, kern = [], [], [], [], {}
        for it in range(a.warmup + a.reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            nb = c.dev_compress(src.data_ptr(), n, dst.data_ptr(), dst.numel())
            torch.cuda.synchronize(); t1 = time.perf_counter()
            te = c.last_timing()[0]
            kt = c.last_kernel_times()
            torch.cuda.synchronize(); t2 = time.perf_counter()
            m = c.dev_decompress(dst.data_ptr(), nb, back.data_ptr(), n + 64)
            torch.cuda.synchronize(); t3 = time.perf_counter()
            td = c.last_timing()[2]
            if it >= a.warmup:
                enc.append(te); dec.append(td); encw.append(t1 - t0); decw.append(t3 - t2)
                for k, v in kt:
                    if k.startswith("knz_alias") or k.startswith("knz_zrlt"):
                        kern.setdefault(k, []).append(v)
        assert m == n and bool(torch.equal(back[:n], src)), (transform, "round trip")
        applied = int(nb) < n - n // 100
        c.close()
        r = {"forward_ms": statistics.median(enc), "inverse_ms": statistics.median(dec), "forward_GBps": n / 1e6 / statistics.median(enc),
             "inverse_GBps": n / 1e6 / statistics.median(dec), "stream_bytes": int(nb), "shrank": applied}
        if kern:
            r["kernels_ms"] = {k: round(statistics.median(v), 4) for k, v in kern.items()}
        if whole:
            r = {"encode_MBps": n / 1e6 / statistics.median(encw), "decode_MBps": n / 1e6 / statistics.median(decw), "bytes": int(nb),
                 "transform_stage_forward_ms": statistics.median(enc), "transform_stage_inverse_ms": statistics.median(dec)}
        return r

    for name, data in inputs.items():
        for tname in ("PACK", "DNA", "ZRLT"):
            out["stage"].setdefault(name, {})[tname + "_device"] = stage(tname, "NONE", data)
        s = out["stage"][name]
        for tname in ("PACK", "DNA"):
            s[tname + "_forward_over_ZRLT_forward"] = s[tname + "_device"]["forward_ms"] / s["ZRLT_device"]["forward_ms"]
            s[tname + "_inverse_over_ZRLT_inverse"] = s[tname + "_device"]["inverse_ms"] / s["ZRLT_device"]["inverse_ms"]
        out["preset"].setdefault(name, {})["DNA+LZ&HUFFMAN_device"] = stage("DNA+LZ", "HUFFMAN", data, whole=True)
        out["preset"][name]["LZ&HUFFMAN_device"] = stage("LZ", "HUFFMAN", data, whole=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
