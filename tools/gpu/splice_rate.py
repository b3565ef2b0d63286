#!/usr/bin/env python3
"""Wall time of knz_dev_concat / knz_dev_slice / knz_dev_splice_many next to what a caller without them has to do for the same streams, on the
synthetic bench corpus (bench_corpus.py):
  concat of K = 16 / 64 / 256 streams of 1 MiB input each (consecutive MiB of the corpus, starting over at its end) ; slice of 16 blocks out of the whole corpus stream ; split of the corpus stream into one
  stream per block ; and the whole corpus stream under another header (a pure copy: the splice copy kernel next to knz_write_splice_copy_kernel, which
  knz_dev_append of nothing runs over the same bytes).
The baseline is knz_dev_decompress_many (knz_dev_decompress_range for the slice, knz_dev_decompress for the split) straight into one plain buffer and
knz_dev_compress / knz_dev_compress_many of it. --baseline-lib names the library the baseline runs on (the parent commit's build) ; without it both
sides run on this tree's. Both sides' outputs are compared before anything is timed: byte for byte where the identity with the Writer applies (the
parts are whole blocks), else (1 MiB streams under 4 and 8 MiB blocks: the splice keeps K short blocks, the baseline packs them) as decoded bytes.
The ceiling is one device-to-device copy of the output's byte count. Wall clock around the calls with the tables built beforehand and the data
resident on the device, untimed warm-up calls, then timed calls: median and range, in ms ; kernel times are the HIP event pairs of
knz_last_kernel_times, in us. Every configuration runs in a child process of its own under a time limit; a child that fails, is killed by a signal or
runs out of time ends the run. Writes profiles/splice_rate.json (or --out).
  python tools/gpu/splice_rate.py [--reps 5] [--warmup 2] [--baseline-lib PATH] [--out profiles/splice_rate.json] [--limit 400]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = {"none_huffman_1m": ("NONE", "HUFFMAN", 1 << 20), "lz_ans0_4m": ("LZ", "ANS0", 4 << 20), "bwt_ans1_8m": ("BWT+RANK+ZRLT", "ANS1", 8 << 20)}
MIB = 1 << 20


def ms(xs):
    return {"median_ms": round(1e3 * statistics.median(xs), 3), "min_ms": round(1e3 * min(xs), 3), "max_ms": round(1e3 * max(xs), 3)}


def baseline_codec(K, path, transform, entropy, bs):
    """a Codec on another build of the library (the parent commit's: it has none of the splice symbols, so the package's loader does not take it):
    the calls the baseline makes, bound by hand"""
    import ctypes as C
    A = K.api
    L = C.CDLL(path)
    vp, u64p = C.c_void_p, C.POINTER(C.c_uint64)
    L.knz_open.argtypes = [C.POINTER(A._Cfg), C.POINTER(vp)]
    L.knz_close.argtypes = [vp]
    L.knz_last_error.argtypes = [vp]
    L.knz_last_error.restype = C.c_char_p
    L.knz_dev_compress.argtypes = [vp, vp, C.c_uint64, C.c_int64, vp, C.c_uint64, u64p, vp]
    L.knz_dev_decompress.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, u64p, vp]
    L.knz_dev_compress_many.argtypes = [vp, C.POINTER(A._Stream), C.c_int, vp]
    L.knz_dev_decompress_many.argtypes = [vp, C.POINTER(A._Stream), C.c_int, vp]
    L.knz_dev_decompress_range.argtypes = [vp, vp, C.c_uint64, C.POINTER(A._BlockRange), vp, C.c_uint64, u64p, vp]
    L.knz_last_kernel_times.argtypes = [vp, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int]
    b = A.Codec.__new__(A.Codec)
    b.L = L
    b.cfg = A._Cfg(A.transform_type(transform), A.entropy_type(entropy), bs, 0, 6, -1, 0)
    b.h = vp()
    rc = L.knz_open(C.byref(b.cfg), C.byref(b.h))
    if rc:
        raise A.KnzError(rc, "knz_open on the baseline library failed: " + L.knz_last_error(None).decode())
    return b


def child(name, reps, warmup, baseline_lib):
    import torch
    import bench_corpus
    import knz
    K = knz.package()
    own = K.build_library()
    dev = torch.device("cuda", 0)
    transform, entropy, bs = CONFIGS[name]
    corpus = bench_corpus.s_silesia()
    n = len(corpus)
    src = torch.from_numpy(corpus).to(dev)
    cap = n + n // 2 + (8 << 20)
    buf = lambda size: torch.zeros(size, dtype=torch.uint8, device=dev)
    KMAX = 256
    room = max(n + (16 << 20), KMAX * MIB + (16 << 20))                     # the plain bytes of the corpus, or of the longest concat
    comp, out_a, out_b, plain, back_b = buf(cap), buf(cap), buf(cap), buf(room), buf(room)
    back_a = buf(max(room, KMAX * bs + 64))                                 # (the device decodes block b at b * block_size: K short blocks need K whole ones)
    c = K.Codec(transform, entropy, bs, lib=own)
    b = baseline_codec(K, baseline_lib, transform, entropy, bs) if baseline_lib else K.Codec(transform, entropy, bs, lib=own)    # the baseline's handle
    nb = c.dev_compress(src.data_ptr(), n, comp.data_ptr(), cap)
    nblocks = (n + bs - 1) // bs

    def timed(fn):
        xs = []
        for it in range(warmup + reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); t1 = time.perf_counter()
            if it >= warmup:
                xs.append(t1 - t0)
        return ms(xs)

    def kernels(codec, prefixes):
        acc = {}
        for nm, t in codec.last_kernel_times():
            if nm.startswith(prefixes):
                acc[nm] = round(acc.get(nm, 0.0) + 1e3 * t, 1)
        return acc

    def rate(nbytes, us):
        return round(nbytes / us / 1e3, 1) if us else None                  # GB/s of output bytes

    def same(x, nx, y, ny, decoded_len=None):
        if decoded_len is None:
            return nx == ny and bool(torch.equal(x[:nx], y[:ny]))
        dx = c.dev_decompress(x.data_ptr(), nx, back_a.data_ptr(), back_a.numel())
        dy = c.dev_decompress(y.data_ptr(), ny, back_b.data_ptr(), back_b.numel())
        return dx == dy == decoded_len and bool(torch.equal(back_a[:dx], back_b[:dy]))

    def ceiling(nbytes):
        return timed(lambda: out_b[:nbytes].copy_(out_a[:nbytes]))

    res = {"bytes": n, "compressed_bytes": int(nb), "blocks": nblocks, "block_size": bs, "baseline_library": "parent build" if baseline_lib else "this tree's", "shapes": {}}
    # ---- concat of K streams of 1 MiB input each
    for k in (16, 64, KMAX):
        offs, at = [], 0
        items = []
        for i in range(k):
            items.append((src.data_ptr() + (i * MIB) % (n - MIB) // 16 * 16, MIB, 0, 2 * MIB + (1 << 17), MIB))     # (the corpus has 202 MiB: the last streams start over)
            offs.append(at)
            at += 2 * MIB + (1 << 17)
        many = buf(at)
        items = [(s, ln, many.data_ptr() + o, cp, hs) for (s, ln, _d, cp, hs), o in zip(items, offs)]
        r = c.dev_compress_many(items, check=True)
        lens = [x[0] for x in r]
        ptrs = [many.data_ptr() + o for o in offs]
        call = lambda: c.dev_concat(ptrs, lens, out_a.data_ptr(), cap, k * MIB, check=True)
        dec_items = [(p, ln, plain.data_ptr() + i * MIB, MIB) for i, (p, ln) in enumerate(zip(ptrs, lens))]

        def base():
            b.dev_decompress_many(dec_items, check=True)
            return b.dev_compress(plain.data_ptr(), k * MIB, out_b.data_ptr(), cap, header_input_size=k * MIB)

        na, nbase = call(), base()
        torch.cuda.synchronize()
        assert same(out_a, na, out_b, nbase, None if MIB % bs == 0 else k * MIB), (name, k, "the two sides differ")
        row = {"output_bytes": int(na), "compared": "streams byte for byte" if MIB % bs == 0 else "decoded bytes", "splice": timed(call)}
        call(); torch.cuda.synchronize()
        row["splice_kernels_us"] = kernels(c, ("knz_splice_", "knz_read_scan"))
        row["copy_kernel_GBps"] = rate(na, row["splice_kernels_us"].get("knz_splice_copy_kernel"))
        row["baseline"] = timed(base)
        b.dev_decompress_many(dec_items, check=True); torch.cuda.synchronize()
        pk = kernels(b, ("knz_many_place_copy",))
        row["baseline_place_copy_us"] = pk
        row["baseline_place_copy_GBps"] = rate(k * MIB, pk.get("knz_many_place_copy_kernel"))
        row["ceiling_copy"] = ceiling(na)
        res["shapes"][f"concat_{k}x1MiB"] = row
        del many
    # ---- slice of 16 blocks
    f, t = 3, min(19, nblocks)
    cnt = t - f
    call = lambda: c.dev_slice(comp.data_ptr(), nb, f, t, out_a.data_ptr(), cap, cnt * bs, check=True)

    def base_slice():
        got = b.dev_decompress_range(comp.data_ptr(), nb, plain.data_ptr(), plain.numel(), f, t)
        return b.dev_compress(plain.data_ptr(), got, out_b.data_ptr(), cap, header_input_size=got)

    na, nbase = call(), base_slice()
    torch.cuda.synchronize()
    assert same(out_a, na, out_b, nbase), (name, "slice: the two streams differ")
    row = {"blocks": cnt, "output_bytes": int(na), "compared": "streams byte for byte", "splice": timed(call)}
    call(); torch.cuda.synchronize()
    row["splice_kernels_us"] = kernels(c, ("knz_splice_", "knz_read_scan"))
    row["copy_kernel_GBps"] = rate(na, row["splice_kernels_us"].get("knz_splice_copy_kernel"))
    row["baseline"] = timed(base_slice)
    row["ceiling_copy"] = ceiling(na)
    res["shapes"]["slice_16_blocks"] = row
    # ---- split into one stream per block
    ocap = bs + bs // 2 + (1 << 17)
    split = buf(nblocks * ocap)
    split_b = buf(nblocks * ocap)
    parts = [(comp.data_ptr(), nb, i + 1, i + 2, i) for i in range(nblocks)]
    outs = [(split.data_ptr() + i * ocap, ocap, min(bs, n - i * bs)) for i in range(nblocks)]
    call = lambda: c.dev_splice_many(parts, outs, check=True)
    citems = [(plain.data_ptr() + i * bs, min(bs, n - i * bs), split_b.data_ptr() + i * ocap, ocap, min(bs, n - i * bs)) for i in range(nblocks)]

    def base_split():
        b.dev_decompress(comp.data_ptr(), nb, plain.data_ptr(), plain.numel())
        return b.dev_compress_many(citems, check=True)

    ra, rb = call()[0], base_split()
    torch.cuda.synchronize()
    for i in range(nblocks):
        assert ra[i][0] == rb[i][0] and bool(torch.equal(split[i * ocap: i * ocap + ra[i][0]], split_b[i * ocap: i * ocap + rb[i][0]])), (name, i, "split: the two streams differ")
    total = sum(x[0] for x in ra)
    row = {"outputs": nblocks, "output_bytes": int(total), "compared": "streams byte for byte", "splice": timed(call)}
    call(); torch.cuda.synchronize()
    row["splice_kernels_us"] = kernels(c, ("knz_splice_", "knz_read_scan"))
    row["walk_us"] = row["splice_kernels_us"].get("knz_splice_walk_kernel")
    row["copy_kernel_GBps"] = rate(total, row["splice_kernels_us"].get("knz_splice_copy_kernel"))
    row["baseline"] = timed(base_split)
    row["ceiling_copy"] = ceiling(total)
    res["shapes"]["split_per_block"] = row
    # ---- the whole stream under another header: the two copy kernels on the same bytes
    call = lambda: c.dev_slice(comp.data_ptr(), nb, 1, None, out_a.data_ptr(), cap, 0, check=True)
    other = lambda: c.dev_append(comp.data_ptr(), nb, src.data_ptr(), 0, out_b.data_ptr(), cap, 0, check=True)
    na, no = call(), other()
    torch.cuda.synchronize()
    assert same(out_a, na, out_b, no), (name, "whole stream: the two streams differ")
    row = {"output_bytes": int(na), "compared": "streams byte for byte", "splice": timed(call)}
    call(); torch.cuda.synchronize()
    row["splice_kernels_us"] = kernels(c, ("knz_splice_", "knz_read_scan"))
    row["copy_kernel_GBps"] = rate(na, row["splice_kernels_us"].get("knz_splice_copy_kernel"))
    row["append_of_nothing"] = timed(other)
    other(); torch.cuda.synchronize()
    wk = kernels(c, ("knz_write_splice",))
    row["write_splice_kernels_us"] = wk
    row["write_splice_copy_GBps"] = rate(no, wk.get("knz_write_splice_copy_kernel"))
    row["ceiling_copy"] = ceiling(na)
    res["shapes"]["whole_stream_new_header"] = row
    c.close()
    b.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=400, help="seconds one configuration may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splice_rate.json"))
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--baseline-lib", default="")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.warmup, a.baseline_lib)
    out = {"reps": a.reps, "warmup": a.warmup, "unit": "ms of wall clock around the C calls, tables built beforehand, data resident on the device",
           "corpus": "bench_corpus.s_silesia()",
           "baseline": "knz_dev_decompress_many / knz_dev_decompress_range / knz_dev_decompress straight into one plain buffer, then knz_dev_compress / knz_dev_compress_many",
           "kernel_times_us": "HIP event pairs around each launch (knz_last_kernel_times), launches of one name summed ; GB/s = output bytes / kernel time",
           "ceiling_copy": "one device-to-device copy of the output's byte count, wall clock", "results": {}}
    for name in a.configs.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--warmup", str(a.warmup), "--child", name]
        if a.baseline_lib:
            cmd += ["--baseline-lib", a.baseline_lib]
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
