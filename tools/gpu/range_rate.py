#!/usr/bin/env python3
"""Wall time of knz_dev_decompress_range next to knz_dev_decompress of the whole stream, taken in the same run on the synthetic bench corpus
(bench_corpus.py): ranges of 1, 4 and 16 blocks at the front, the middle and the end of the stream, each walked from the header and from the
index's bit (from_bit), and knz_dev_decompress_many_range of 16 single-block entries next to 16 single range calls. The question the figures
answer: does a range's time follow its slowest block's chain plus the walk, or the stream? Wall clock around the calls with the data resident
on the device, untimed warm-up calls, then timed calls: median and range, in ms. Every configuration runs in a child process of its own under
a time limit; a child that fails, is killed by a signal or runs out of time ends the run. Writes profiles/range_rate.json (or --out).
  python tools/gpu/range_rate.py [--reps 10] [--warmup 3] [--out profiles/range_rate.json] [--limit 420]"""
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

CONFIGS = {"bwt_ans1_8m": ("BWT+RANK+ZRLT", "ANS1", 8 << 20), "lz_ans0_4m": ("LZ", "ANS0", 4 << 20)}


def ms(xs):
    return {"median_ms": round(1e3 * statistics.median(xs), 3), "min_ms": round(1e3 * min(xs), 3), "max_ms": round(1e3 * max(xs), 3)}


def child(name, reps, warmup):
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
    back = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
    c = K.Codec(transform, entropy, bs)
    nb = c.dev_compress(src.data_ptr(), n, comp.data_ptr(), comp.numel())
    info, pos = c.dev_stream_index(comp.data_ptr(), nb)
    blocks = info["n_blocks"]
    assert blocks == (n + bs - 1) // bs and blocks >= 16

    def timed(fn):
        xs = []
        for it in range(warmup + reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); t1 = time.perf_counter()
            if it >= warmup:
                xs.append(t1 - t0)
        return ms(xs)

    out = {"bytes": n, "compressed_bytes": int(nb), "blocks": blocks, "block_size": bs}
    assert c.dev_decompress(comp.data_ptr(), nb, back.data_ptr(), n + 64) == n and bool(torch.equal(back[:n], src)), "round trip"
    out["whole_stream"] = timed(lambda: c.dev_decompress(comp.data_ptr(), nb, back.data_ptr(), n + 64))
    t0 = time.perf_counter()
    for _ in range(reps):
        c.dev_stream_index(comp.data_ptr(), nb, pos_cap=blocks)
    out["index_ms"] = round(1e3 * (time.perf_counter() - t0) / reps, 3)
    out["ranges"] = {}
    for cnt in (1, 4, 16):
        for place, first in (("front", 1), ("middle", (blocks - cnt) // 2 + 1), ("end", blocks - cnt + 1)):
            lo, hi = (first - 1) * bs, min((first - 1 + cnt) * bs, n)
            for hint in (0, pos[first - 1][0]):
                back.zero_()
                got = c.dev_decompress_range(comp.data_ptr(), nb, back.data_ptr(), hi - lo, first, first + cnt, hint)
                assert got == hi - lo and bool(torch.equal(back[:got], src[lo:hi])) and c.last_counter(7) == cnt, (cnt, place, hint)   # the figures are of the right bytes
                r = timed(lambda: c.dev_decompress_range(comp.data_ptr(), nb, back.data_ptr(), hi - lo, first, first + cnt, hint))
                out["ranges"][f"{cnt}_{place}_{'from_bit' if hint else 'walk'}"] = r
    # 16 single-block entries spread over the stream: one many call next to 16 single calls
    ids = [1 + (i * (blocks - 1)) // 15 for i in range(16)]
    dsts = [torch.zeros(bs + 64, dtype=torch.uint8, device=dev) for _ in ids]
    items = [(comp.data_ptr(), nb, d.data_ptr(), bs, b, b + 1, pos[b - 1][0]) for b, d in zip(ids, dsts)]
    res = c.dev_decompress_many_range(items, check=True)
    for (got, _s), b, d in zip(res, ids, dsts):
        assert bool(torch.equal(d[:got], src[(b - 1) * bs: min(b * bs, n)]))
    assert c.last_counter(7) == 16
    out["many_16_single_blocks"] = timed(lambda: c.dev_decompress_many_range(items, check=True))
    out["loop_16_single_blocks"] = timed(lambda: [c.dev_decompress_range(comp.data_ptr(), nb, d.data_ptr(), bs, b, b + 1, pos[b - 1][0]) for b, d in zip(ids, dsts)])
    c.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=420, help="seconds one configuration may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_rate.json"))
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.warmup)
    out = {"reps": a.reps, "warmup": a.warmup, "unit": "ms of wall clock around the call, data resident on the device",
           "corpus": "bench_corpus.s_silesia()", "results": {}}
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
