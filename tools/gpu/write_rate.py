#!/usr/bin/env python3
"""Wall time of knz_dev_write_many / knz_dev_append next to what a caller without them has to do for the same new stream, taken in the same run on
the synthetic bench corpus (bench_corpus.py): one write of 100 B, 64 scattered writes of 100 B, and one append of 1 MiB. The baseline is
knz_dev_decompress of the whole stream, the overlay as device copies (one torch slice assignment per write), and knz_dev_compress of the edited
bytes. Both sides write the header with the edited length; their streams are compared byte for byte before anything is timed. Next to the wall
times: the blocks that entered the decode and the encode batch, and the probed times of the write kernels (overlay, splice plan, splice copy).
Wall clock around the C calls with the tables built beforehand and the data resident on the device, untimed warm-up calls, then timed calls:
median and range, in ms. Every configuration runs in a child process of its own under a time limit; a child that fails, is killed by a signal or
runs out of time ends the run. Writes profiles/write_rate.json (or --out).
  python tools/gpu/write_rate.py [--reps 5] [--warmup 2] [--out profiles/write_rate.json] [--limit 300]"""
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

CONFIGS = {"none_huffman_1m": ("NONE", "HUFFMAN", 1 << 20), "lz_ans0_4m": ("LZ", "ANS0", 4 << 20), "bwt_ans1_8m": ("BWT+RANK+ZRLT", "ANS1", 8 << 20)}


def ms(xs):
    return {"median_ms": round(1e3 * statistics.median(xs), 3), "min_ms": round(1e3 * min(xs), 3), "max_ms": round(1e3 * max(xs), 3)}


def child(name, reps, warmup):
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
    cap = n + n // 2 + (8 << 20)
    comp = torch.zeros(cap, dtype=torch.uint8, device=dev)
    new = torch.zeros(cap, dtype=torch.uint8, device=dev)
    base_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    plain = torch.zeros(n + (2 << 20), dtype=torch.uint8, device=dev)
    c = K.Codec(transform, entropy, bs)
    nb = c.dev_compress(src.data_ptr(), n, comp.data_ptr(), cap)
    L = c.L
    END = K.api.OFFSET_END

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

    rng = np.random.default_rng(1)
    data = torch.from_numpy(rng.integers(0, 256, (1 << 20) + 64, dtype=np.uint8)).to(dev)
    lists = {"1x100": [(int(rng.integers(0, n - 100)), 100)], "64x100": [(int(o), 100) for o in rng.integers(0, n - 100, 64)], "append_1MiB": [(END, 1 << 20)]}
    out = {"bytes": n, "compressed_bytes": int(nb), "blocks": (n + bs - 1) // bs, "block_size": bs, "writes": {}}
    for label, ws in lists.items():
        W = len(ws)
        arr = (K.api._Write * W)()
        at = 0
        for i, (o, l) in enumerate(ws):
            arr[i].offset, arr[i].length, arr[i].d_data = o, l, data.data_ptr() + 1 + at          # from an odd address
            at += l if W > 1 else 0
        grown = n + sum(l for o, l in ws if o == END)
        got, want = C.c_uint64(), C.c_uint64()
        call = lambda: L.knz_dev_write_many(c.h, comp.data_ptr(), nb, arr, W, grown, new.data_ptr(), cap, C.byref(got), None)

        def base():
            dec = C.c_uint64()
            assert L.knz_dev_decompress(c.h, comp.data_ptr(), nb, plain.data_ptr(), plain.numel(), C.byref(dec), None) == 0 and dec.value == n
            cur, k = n, 0
            for o, l in ws:
                o = cur if o == END else o
                plain[o: o + l] = data[1 + k: 1 + k + l]
                cur, k = max(cur, o + l), k + (l if W > 1 else 0)
            assert L.knz_dev_compress(c.h, plain.data_ptr(), grown, grown, base_out.data_ptr(), cap, C.byref(want), None) == 0

        assert call() == 0, c.L.knz_last_error(c.h)
        touched, encoded = int(c.last_counter(7)), int(c.last_counter(16))
        base()
        torch.cuda.synchronize()
        assert got.value == want.value and bool(torch.equal(new[: got.value], base_out[: want.value])), (label, "the two streams differ")
        row = {"decoded_blocks": touched, "encoded_blocks": encoded, "new_stream_bytes": int(got.value), "write_many": timed(call)}
        call()
        torch.cuda.synchronize()
        row["write_kernels_us"] = kernels("knz_write_")
        row["baseline"] = timed(base)
        out["writes"][label] = row
    c.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds one configuration may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "write_rate.json"))
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.warmup)
    out = {"reps": a.reps, "warmup": a.warmup, "unit": "ms of wall clock around the C call, tables built beforehand, data resident on the device",
           "corpus": "bench_corpus.s_silesia()", "baseline": "knz_dev_decompress of the whole stream, one device copy per write, knz_dev_compress of the edited bytes",
           "kernel_times_us": "HIP event pairs around each launch (knz_last_kernel_times), launches of one name summed", "results": {}}
    for name in a.configs.split(","):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--warmup", str(a.warmup), "--child", name]
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
