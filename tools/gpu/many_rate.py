#!/usr/bin/env python3
"""Rates of knz_dev_compress_many / knz_dev_decompress_many next to their yardstick, taken in the same run: the same inputs through a loop of
single knz_dev_compress / knz_dev_decompress calls on one handle. Workload: the head of the bench corpus cut into K files of 1 MiB (K = 16,
64, 256), and a set of files of mixed sizes between 4 KiB and 8 MiB. Wall clock around the calls with the data resident on the device,
untimed warm-up steps, then timed steps: median and range. Every (pipeline, set) runs in a child process of its own under a time limit; a
child that fails, is killed by a signal or runs out of time ends the run. Writes profiles/many_rate.json (or --out).
  python tools/gpu/many_rate.py [--reps 5] [--warmup 2] [--out profiles/many_rate.json] [--limit 240]"""
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

PIPELINES = {"bwt_ans1": ("BWT+RANK+ZRLT", "ANS1", 8 << 20), "l5": ("TEXT+UTF+BWT+RANK+ZRLT", "ANS0", 4 << 20), "lz_ans0": ("LZ", "ANS0", 4 << 20)}
SETS = ("k16", "k64", "k256", "mixed")


def file_sizes(name):
    if name.startswith("k"):
        return [1 << 20] * int(name[1:])
    import numpy as np
    rng = np.random.default_rng(11)
    sizes = [int(4096 * 2 ** rng.uniform(0, 11)) & ~15 for _ in range(96)]   # 4 KiB .. 8 MiB, log-uniform
    return sizes


def stats(xs, nbytes):
    r = [nbytes / 1e6 / x for x in xs]
    return {"median_MBps": round(statistics.median(r), 1), "min_MBps": round(min(r), 1), "max_MBps": round(max(r), 1)}


def child(pipe, sname, reps, warmup):
    import numpy as np
    import torch
    import bench_corpus
    import knz
    K = knz.package()
    K.build_library()
    dev = torch.device("cuda", 0)
    transform, entropy, bs = PIPELINES[pipe]
    sizes = file_sizes(sname)
    total = sum(sizes)
    corpus = np.resize(bench_corpus.s_silesia(), total)                   # (a set longer than the corpus starts over at its head)
    whole = torch.from_numpy(corpus).to(dev)
    srcs, dsts, backs, at = [], [], [], 0
    for n in sizes:                                                        # every file in a buffer of its own (256-byte aligned by the allocator)
        srcs.append(whole[at: at + n].clone())
        dsts.append(torch.zeros(n + n // 2 + (1 << 18), dtype=torch.uint8, device=dev))
        backs.append(torch.zeros(n + 64, dtype=torch.uint8, device=dev))
        at += n
    c = K.Codec(transform, entropy, bs)
    t = {"loop_enc": [], "loop_dec": [], "many_enc": [], "many_dec": []}
    lens = None
    for it in range(warmup + reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        nbs = [c.dev_compress(s.data_ptr(), n, d.data_ptr(), d.numel()) for s, n, d in zip(srcs, sizes, dsts)]
        torch.cuda.synchronize(); t1 = time.perf_counter()
        for d, nb, b, n in zip(dsts, nbs, backs, sizes):
            assert c.dev_decompress(d.data_ptr(), nb, b.data_ptr(), n + 64) == n
        torch.cuda.synchronize(); t2 = time.perf_counter()
        if it == 0:
            single = [d[:nb].clone() for d, nb in zip(dsts, nbs)]
        res = c.dev_compress_many([(s.data_ptr(), n, d.data_ptr(), d.numel()) for s, n, d in zip(srcs, sizes, dsts)], check=True)
        torch.cuda.synchronize(); t3 = time.perf_counter()
        if it == 0:                                                        # the figures are of the same bytes
            assert [r[0] for r in res] == nbs
            assert all(bool(torch.equal(d[:nb], s)) for d, nb, s in zip(dsts, nbs, single)), "many call != loop of single calls"
            for b in backs:
                b.zero_()
        torch.cuda.synchronize(); t4 = time.perf_counter()
        res = c.dev_decompress_many([(d.data_ptr(), nb, b.data_ptr(), n + 64) for d, nb, b, n in zip(dsts, nbs, backs, sizes)], check=True)
        torch.cuda.synchronize(); t5 = time.perf_counter()
        if it == 0:
            assert [r[0] for r in res] == sizes and all(bool(torch.equal(b[:n], s)) for b, n, s in zip(backs, sizes, srcs)), "round trip"
        if it >= warmup:
            t["loop_enc"].append(t1 - t0); t["loop_dec"].append(t2 - t1); t["many_enc"].append(t3 - t2); t["many_dec"].append(t5 - t4)
        lens = nbs
    c.close()
    out = {k: stats(v, total) for k, v in t.items()}
    out.update({"files": len(sizes), "bytes": total, "compressed_bytes": int(sum(lens)), "blocks": int(sum((n + bs - 1) // bs for n in sizes)),
                "encode_ratio": round(out["many_enc"]["median_MBps"] / out["loop_enc"]["median_MBps"], 2),
                "decode_ratio": round(out["many_dec"]["median_MBps"] / out["loop_dec"]["median_MBps"], 2)})
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds one (pipeline, set) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "many_rate.json"))
    ap.add_argument("--pipelines", default=",".join(PIPELINES))
    ap.add_argument("--sets", default=",".join(SETS))
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.reps, a.warmup)
    out = {"reps": a.reps, "warmup": a.warmup, "unit": "MB/s of uncompressed bytes, wall clock, data resident on the device",
           "yardstick": "loop of single knz_dev_compress / knz_dev_decompress calls, one handle, same process and inputs", "results": {}}
    for pipe in a.pipelines.split(","):
        for sname in a.sets.split(","):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--warmup", str(a.warmup), "--child", pipe, sname]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:                              # nothing more is started on the device after a step that did not end well
                out["results"].setdefault(pipe, {})[sname] = {"failed": p.returncode}
                with open(a.out, "w") as f:
                    json.dump(out, f, indent=1)
                print(f"{pipe} {sname}: exit status {p.returncode}, stopping", flush=True)
                return 1
            out["results"].setdefault(pipe, {})[sname] = json.loads(line[0][7:])
            print(pipe, sname, line[0][7:], flush=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
