#!/usr/bin/env python3
"""Wall time of knz_dev_write_streams next to the loop of knz_dev_write_many over the same targets on the same handle, taken in the same run: T = 1, 8
and 64 targets, every source a stream of 4 blocks cut from the synthetic bench corpus (bench_corpus.py), in two shapes: one write of 100 B into the
second block of every target, and one append of 1 MiB per target. Both sides' streams are compared byte for byte before anything is timed. Next to
the wall times: the blocks that entered the decode and the encode batch, and the probed times of the call's plan and copy kernels.
Wall clock around the C calls with the tables built beforehand and the data resident on the device, untimed warm-up calls, then timed calls: median
and range, in ms. Every configuration runs in a child process of its own under a time limit; a child that fails, is killed by a signal or runs out
of time ends the run. Writes profiles/write_streams_rate.json (or --out).
  python tools/gpu/write_streams_rate.py [--reps 5] [--warmup 2] [--out profiles/write_streams_rate.json] [--limit 900]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from write_rate import CONFIGS, ms                                          # the three configurations of the single call's measurement

TARGETS = (1, 8, 64)


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
    n = 4 * bs
    assert len(corpus) > n
    tmax = max(TARGETS)
    step = (len(corpus) - n) // tmax // 16 * 16
    c = K.Codec(transform, entropy, bs)
    L = c.L
    END = K.api.OFFSET_END
    cap = n + n // 2 + (8 << 20)
    rng = np.random.default_rng(1)
    data = torch.from_numpy(rng.integers(0, 256, (1 << 20) + 64, dtype=np.uint8)).to(dev)
    plain = torch.zeros(n, dtype=torch.uint8, device=dev)
    srcs, lens, outs, singles = [], [], [], []
    for k in range(tmax):                                                   # every source compressed once, resident ; two destinations per target
        plain.copy_(torch.from_numpy(corpus[k * step: k * step + n]).to(dev))
        comp = torch.zeros(cap, dtype=torch.uint8, device=dev)
        nb = c.dev_compress(plain.data_ptr(), n, comp.data_ptr(), cap)
        srcs.append(comp[: (nb + 3) // 4 * 4].clone())
        lens.append(int(nb))
        outs.append(torch.zeros(cap, dtype=torch.uint8, device=dev))
        singles.append(torch.zeros(cap, dtype=torch.uint8, device=dev))
        del comp

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

    shapes = {"1x100_second_block": (bs + 12345, 100), "append_1MiB": (END, 1 << 20)}
    out = {"block_size": bs, "source_bytes": n, "shapes": {}}
    for label, (off, length) in shapes.items():
        rows = {}
        for T in TARGETS:
            grown = n + (length if off == END else 0)
            ta, wa = (K.api._WriteTarget * T)(), (K.api._WriteTo * T)()
            one = [(K.api._Write * 1)() for _ in range(T)]
            for k in range(T):
                ta[k].d_src, ta[k].n_bytes, ta[k].d_dst, ta[k].dst_cap, ta[k].header_input_size = srcs[k].data_ptr(), lens[k], outs[k].data_ptr(), cap, grown
                wa[k].target, wa[k].offset, wa[k].length, wa[k].d_data = k, off, length, data.data_ptr() + 1 + k % 32      # from odd addresses
                one[k][0].offset, one[k][0].length, one[k][0].d_data = off, length, data.data_ptr() + 1 + k % 32
            got = C.c_uint64()
            call = lambda: L.knz_dev_write_streams(c.h, ta, T, wa, T, None)

            def loop():
                for k in range(T):
                    assert L.knz_dev_write_many(c.h, srcs[k].data_ptr(), lens[k], one[k], 1, grown, singles[k].data_ptr(), cap, C.byref(got), None) == 0

            assert call() == 0, L.knz_last_error(c.h)
            dec, enc = int(c.last_counter(7)), int(c.last_counter(16))
            loop()
            torch.cuda.synchronize()
            for k in range(T):
                m = int(ta[k].out_bytes)
                assert ta[k].status == 0 and m and bool(torch.equal(outs[k][:m], singles[k][:m])), (label, T, k, "the two streams differ")
            row = {"decoded_blocks": dec, "encoded_blocks": enc, "write_streams": timed(call)}
            call()
            torch.cuda.synchronize()
            row["kernels_us"] = kernels("knz_ws_")
            row["loop_of_write_many"] = timed(loop)
            row["ratio"] = round(row["write_streams"]["median_ms"] / row["loop_of_write_many"]["median_ms"], 3)
            rows[f"T={T}"] = row
            print(f"{name} {label} T={T}: {row['write_streams']['median_ms']} ms against {row['loop_of_write_many']['median_ms']} ms", file=sys.stderr, flush=True)
        out["shapes"][label] = rows
    c.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=900, help="seconds one configuration may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "write_streams_rate.json"))
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.warmup)
    out = {"reps": a.reps, "warmup": a.warmup, "unit": "ms of wall clock around the C call(s), tables built beforehand, data resident on the device",
           "corpus": "4-block slices of bench_corpus.s_silesia()", "baseline": "the loop of knz_dev_write_many over the same targets, same handle, same run",
           "ratio": "median of knz_dev_write_streams / median of the loop",
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
