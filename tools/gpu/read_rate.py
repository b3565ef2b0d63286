#!/usr/bin/env python3
"""Wall time of knz_dev_read_many next to what a caller of the range calls has to do for the same bytes, taken in the same run on the synthetic
bench corpus (bench_corpus.py): R = 1, 64, 4 096 and 65 536 reads of 100 B and of 4 KiB at random offsets into one packed destination, and one
read of the whole stream. The baseline is knz_dev_decompress_many_range with one entry per read for the covering blocks into block-sized buffers
plus the slicing copy (one torch copy per read); it runs only where its buffers (R x covering blocks x block size, twice: destinations and the
batch's staging) fit --baseline-bytes, and is reported as not run with the bytes it would need elsewhere. Both sides start their walks from the
index's bits (knz_source.pos / from_bit). Next to the wall times: the probed kernel
times of the read kernels (plan, scan, gather) and, on the same decoded bytes in the same run, the gather kernel's bytes per second next to
knz_many_place_copy_kernel's (the whole stream through a one-entry range call into an aligned destination, and through one read into a
destination off 16 bytes by 3). Wall clock around the C calls with the tables built beforehand and the data resident on the device, untimed
warm-up calls, then timed calls: median and range, in ms. Every configuration runs in a child process of its own under a time limit; a child that
fails, is killed by a signal or runs out of time ends the run. Writes profiles/read_rate.json (or --out).
  python tools/gpu/read_rate.py [--reps 5] [--warmup 2] [--out profiles/read_rate.json] [--limit 300]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# the two pipelines of tools/gpu/range_rate.py (chain bound) and a bandwidth-shaped one, where the copy is what is left
CONFIGS = {"bwt_ans1_8m": ("BWT+RANK+ZRLT", "ANS1", 8 << 20), "lz_ans0_4m": ("LZ", "ANS0", 4 << 20), "none_huffman_1m": ("NONE", "HUFFMAN", 1 << 20)}
COUNTS = (1, 64, 4096, 65536)
SIZES = (100, 4096)


def ms(xs):
    return {"median_ms": round(1e3 * statistics.median(xs), 3), "min_ms": round(1e3 * min(xs), 3), "max_ms": round(1e3 * max(xs), 3)}


def child(name, reps, warmup, baseline_bytes):
    import numpy as np
    import torch
    import bench_corpus
    import knz
    K = knz.package()
    K.build_library()
    dev = torch.device("cuda", 0)
    transform, entropy, bs = CONFIGS[name]
    corpus = bench_corpus.s_silesia()
    n = len(corpus)
    src = torch.from_numpy(corpus).to(dev)
    comp = torch.zeros(n + n // 2 + (1 << 20), dtype=torch.uint8, device=dev)
    c = K.Codec(transform, entropy, bs)
    nb = c.dev_compress(src.data_ptr(), n, comp.data_ptr(), comp.numel())
    info, pos = c.dev_stream_index(comp.data_ptr(), nb)
    blocks = info["n_blocks"]
    L = c.L

    def timed(fn):
        xs = []
        for it in range(warmup + reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); t1 = time.perf_counter()
            if it >= warmup:
                xs.append(t1 - t0)
        return ms(xs)

    def kernels(prefix):
        acc = {}
        for nm, t in c.last_kernel_times():
            if nm.startswith(prefix):
                acc[nm] = round(acc.get(nm, 0.0) + 1e3 * t, 1)
        return acc                                                          # microseconds per kernel, launches of one name summed

    rows = (K.api._BlockPos * blocks)()
    for i, (bit, bits) in enumerate(pos):
        rows[i].bit, rows[i].bits = bit, bits
    source = (K.api._Source * 1)()
    source[0].d_src, source[0].n, source[0].pos, source[0].n_pos = comp.data_ptr(), nb, rows, blocks
    out = {"bytes": n, "compressed_bytes": int(nb), "blocks": blocks, "block_size": bs, "reads": {}}
    rng = np.random.default_rng(1)
    for size in SIZES:
        for R in COUNTS:
            offs = [int(o) for o in rng.integers(0, n - size, R)]
            packed = torch.zeros(R * size + 64, dtype=torch.uint8, device=dev)
            rd = (K.api._Read * R)()
            for i, o in enumerate(offs):
                rd[i].source, rd[i].offset, rd[i].length, rd[i].d_dst = 0, o, size, packed.data_ptr() + 1 + i * size    # packed, from an odd address
            call = lambda: L.knz_dev_read_many(c.h, source, 1, rd, R, None)
            assert call() == 0
            torch.cuda.synchronize()
            idx = (torch.tensor(offs, device=dev).unsqueeze(1) + torch.arange(size, device=dev)).reshape(-1)
            assert bool(torch.equal(packed[1: 1 + R * size], src[idx])), (R, size)                     # the figures are of the right bytes
            touched = c.last_counter(7)
            row = {"blocks_decoded": int(touched), "read_many": timed(call)}
            call()
            torch.cuda.synchronize()
            row["read_kernels_us"] = kernels("knz_read_")
            # the parent commit's way: one entry per read for its covering blocks into block-sized buffers, then the slices
            cover = [(o // bs + 1, (o + size - 1) // bs + 2) for o in offs]
            need = 2 * sum(t - f for f, t in cover) * (bs + 64)
            if need > baseline_bytes:
                row["baseline"] = {"not_run": "buffers of %d bytes" % need}
            else:
                dsts = [torch.zeros((t - f) * bs + 64, dtype=torch.uint8, device=dev) for f, t in cover]
                st = (K.api._Stream * R)()
                rg = (K.api._BlockRange * R)()
                for i, ((f, t), d) in enumerate(zip(cover, dsts)):
                    st[i].d_src, st[i].n, st[i].d_dst, st[i].dst_cap = comp.data_ptr(), nb, d.data_ptr(), (t - f) * bs
                    rg[i].from_block, rg[i].to_block, rg[i].from_bit = f, t, pos[f - 1][0]

                def base():
                    assert L.knz_dev_decompress_many_range(c.h, st, rg, R, None) == 0
                    for i, (o, d) in enumerate(zip(offs, dsts)):
                        w = o - (cover[i][0] - 1) * bs
                        packed[1 + i * size: 1 + (i + 1) * size] = d[w: w + size]
                packed.zero_()
                base()
                torch.cuda.synchronize()
                assert bool(torch.equal(packed[1: 1 + R * size], src[idx])), (R, size, "baseline")
                row["baseline"] = dict(timed(base), blocks_decoded=int(c.last_counter(7)))
                del dsts
            out["reads"][f"{R}x{size}"] = row
            del packed
    # one read of the whole stream ; the copy kernels on the same decoded bytes
    whole = torch.zeros(n + 128, dtype=torch.uint8, device=dev)
    one = (K.api._Read * 1)()
    gather = {}
    for label, shift in (("aligned", 0), ("off_by_3", 3)):
        one[0].source, one[0].offset, one[0].length, one[0].d_dst = 0, 0, n, whole.data_ptr() + shift
        call = lambda: L.knz_dev_read_many(c.h, source, 1, one, 1, None)
        assert call() == 0 and one[0].out_bytes == n
        torch.cuda.synchronize()
        assert bool(torch.equal(whole[shift: shift + n], src))
        t = timed(call)
        call()
        torch.cuda.synchronize()
        k = kernels("knz_read_")
        us = k["knz_read_gather_kernel"]
        gather[label] = {"read_many": t, "read_kernels_us": k, "gather_GBps": round(n / us / 1e3, 1)}
    out["whole_stream_read"] = gather
    st = (K.api._Stream * 1)()
    rg = (K.api._BlockRange * 1)()
    st[0].d_src, st[0].n, st[0].d_dst, st[0].dst_cap = comp.data_ptr(), nb, whole.data_ptr(), n + 64
    rg[0].from_block, rg[0].to_block, rg[0].from_bit = 1, 0xFFFFFFFF, 0
    call = lambda: L.knz_dev_decompress_many_range(c.h, st, rg, 1, None)
    assert call() == 0 and st[0].out_bytes == n
    torch.cuda.synchronize()
    assert bool(torch.equal(whole[:n], src))
    t = timed(call)
    call()
    torch.cuda.synchronize()
    us = kernels("knz_many_place_copy_kernel")["knz_many_place_copy_kernel"]
    out["whole_stream_many_range"] = {"many_range": t, "place_copy_us": us, "place_copy_GBps": round(n / us / 1e3, 1)}
    c.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds one configuration may take")
    ap.add_argument("--baseline-bytes", type=int, default=24 << 30, help="device memory the baseline's buffers may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_rate.json"))
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.warmup, a.baseline_bytes)
    out = {"reps": a.reps, "warmup": a.warmup, "unit": "ms of wall clock around the C call, tables built beforehand, data resident on the device",
           "corpus": "bench_corpus.s_silesia()", "baseline": "knz_dev_decompress_many_range, one entry per read for its covering blocks into "
           "block-sized buffers, plus one slicing copy per read",
           "kernel_times_us": "HIP event pairs around each launch (knz_last_kernel_times), launches of one name summed; the GB/s figures are the stream's decoded bytes over that time", "results": {}}
    for name in a.configs.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--warmup", str(a.warmup),
               "--baseline-bytes", str(a.baseline_bytes), "--child", name]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:                                  # nothing more is started on the device after a step that did not end well
            out["results"][name] = {"failed": p.returncode}
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
            print(f"{name}: exit status {p.returncode}, stopping", flush=True)
            return 1
        out["results"][name] = json.loads(line[0][7:])
        print(name, line[0][7:], flush=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
