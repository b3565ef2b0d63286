#!/usr/bin/env python3
"""Wall time of knz_dev_find_many next to what a caller without it has to do for the same answer, taken in the same run on the synthetic bench corpus
(bench_corpus.py): one query of a 12-byte pattern over the whole stream, 64 queries over windows of 1 MiB at random offsets, and 16 patterns over the
whole stream in one call. The patterns are 12-byte pieces of the corpus, so every query has hits; every d_hits array holds 4 096 offsets.
The baseline is what a caller of the library without the find call does: knz_dev_decompress_many for the whole stream (knz_dev_decompress_many_range,
one entry per window for its covering blocks and hinted by the index, for the windows) into device buffers, a copy of those to the host, bytes.find
restarted at hit + 1. Its three parts are timed together and the decode and the copy also alone. knz_dev_decompress_many alone is the floor of any
answer that decodes the stream. Both sides are checked against each other before they are timed. Next to the wall times: the probed kernel times of
the find tail (the knz_find_* kernels and the scans it launches). Wall clock around the calls with the tables built beforehand and the data resident
on the device, untimed warm-up calls, then timed calls: median and range, in ms. Every configuration runs in a child process of its own under a time
limit; a child that fails, is killed by a signal or runs out of time ends the run. Writes profiles/find_rate.json (or --out).
  python tools/gpu/find_rate.py [--reps 5] [--warmup 2] [--out profiles/find_rate.json] [--limit 400]"""
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
PATTERN, WINDOWS, WINDOW, PATTERNS, HITS_CAP = 12, 64, 1 << 20, 16, 4096


def ms(xs):
    return {"median_ms": round(1e3 * statistics.median(xs), 3), "min_ms": round(1e3 * min(xs), 3), "max_ms": round(1e3 * max(xs), 3)}


def host_find(buf, pat, lo, hi):
    """starts in [lo, hi) of buf, overlapping ones included"""
    out, p = [], buf.find(pat, lo)
    while p != -1 and p < hi:
        out.append(p)
        p = buf.find(pat, p + 1)
    return out


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
    comp = torch.zeros(n + n // 2 + (1 << 20), dtype=torch.uint8, device=dev)
    c = K.Codec(transform, entropy, bs)
    nb = c.dev_compress(src.data_ptr(), n, comp.data_ptr(), comp.numel())
    del src
    info, pos = c.dev_stream_index(comp.data_ptr(), nb)
    blocks = info["n_blocks"]
    L = c.L
    raw = corpus.tobytes()

    def timed(fn):
        xs = []
        for it in range(warmup + reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); t1 = time.perf_counter()
            if it >= warmup:
                xs.append(t1 - t0)
        return ms(xs)

    def kernels():
        acc = {}
        for nm, t in c.last_kernel_times():
            if nm.startswith("knz_find_") or nm == "knz_read_scan_kernel":
                acc[nm] = round(acc.get(nm, 0.0) + 1e3 * t, 1)
        return acc                                                          # microseconds per kernel, launches of one name summed

    rows = (K.api._BlockPos * blocks)()
    for i, (bit, bits) in enumerate(pos):
        rows[i].bit, rows[i].bits = bit, bits
    source = (K.api._Source * 1)()
    source[0].d_src, source[0].n, source[0].pos, source[0].n_pos = comp.data_ptr(), nb, rows, blocks
    rng = np.random.default_rng(1)
    pats = [raw[o: o + PATTERN] for o in (int(x) for x in rng.integers(0, n - PATTERN, PATTERNS))]
    offs = [int(o) for o in rng.integers(0, n - WINDOW, WINDOWS)]
    whole = torch.zeros(n + 128, dtype=torch.uint8, device=dev)
    host = torch.empty(n + 128, dtype=torch.uint8).pin_memory()
    out = {"bytes": n, "compressed_bytes": int(nb), "blocks": blocks, "block_size": bs, "cases": {}}

    def find_case(label, queries, baseline, want):
        """queries: [(pattern, offset, length or None)] ; baseline(): the caller's way -> [[offsets]] ; want: the same, computed once on the corpus"""
        q = len(queries)
        hits = torch.zeros(q * HITS_CAP, dtype=torch.int64, device=dev)
        fd = (K.api._Find * q)()
        keep = []
        for i, (pat, o, ln) in enumerate(queries):
            buf = C.create_string_buffer(pat, len(pat))
            keep.append(buf)
            fd[i].source, fd[i].pattern_len, fd[i].pattern, fd[i].offset, fd[i].length = 0, len(pat), C.addressof(buf), o, K.api.LENGTH_END if ln is None else ln
            fd[i].d_hits, fd[i].hits_cap = hits.data_ptr() + 8 * i * HITS_CAP, HITS_CAP
        call = lambda: L.knz_dev_find_many(c.h, source, 1, fd, q, None)
        assert call() == 0
        torch.cuda.synchronize()
        got = hits.cpu().numpy().reshape(q, HITS_CAP)
        for i, w in enumerate(want):                                        # the figures are of the right answers
            assert fd[i].n_hits == len(w) and [int(x) for x in got[i][: min(len(w), HITS_CAP)]] == w[:HITS_CAP], (label, i, fd[i].n_hits, len(w))
        assert baseline() == want, (label, "baseline")
        row = {"queries": q, "hits": [len(w) for w in want], "blocks_decoded": int(c.last_counter(7)), "find_many": timed(call)}
        call()
        torch.cuda.synchronize()
        row["find_kernels_us"] = kernels()
        row["baseline"] = timed(baseline)
        fm, bl = row["find_many"]["median_ms"], row["baseline"]["median_ms"]
        row["find_many_over_baseline"] = round(fm / bl, 3)
        out["cases"][label] = row

    # the whole stream into one device buffer: the floor, and the first two parts of the baseline
    st = (K.api._Stream * 1)()
    st[0].d_src, st[0].n, st[0].d_dst, st[0].dst_cap = comp.data_ptr(), nb, whole.data_ptr(), n + 64

    def decode_whole():
        assert L.knz_dev_decompress_many(c.h, st, 1, None) == 0 and st[0].out_bytes == n

    def fetch_whole():
        decode_whole()
        host[:n].copy_(whole[:n])
        torch.cuda.synchronize()
        return host[:n].numpy().tobytes()

    assert fetch_whole() == raw
    out["decompress_many"] = timed(decode_whole)
    out["decompress_many_and_copy_to_host"] = timed(lambda: (decode_whole(), host[:n].copy_(whole[:n])))

    want1 = [host_find(raw, pats[0], 0, n)]
    find_case("one_pattern_whole_stream", [(pats[0], 0, None)], lambda: [host_find(fetch_whole(), pats[0], 0, n)], want1)
    want16 = [host_find(raw, p, 0, n) for p in pats]

    def base16():
        buf = fetch_whole()
        return [host_find(buf, p, 0, n) for p in pats]
    find_case("16_patterns_whole_stream", [(p, 0, None) for p in pats], base16, want16)

    # 64 windows of 1 MiB: the range call for the covering blocks of each window and of the pattern's reach behind it, then the slices
    cover = [(o // bs + 1, (o + WINDOW + PATTERN - 2) // bs + 2) for o in offs]
    dsts = [torch.zeros((t - f) * bs + 64, dtype=torch.uint8, device=dev) for f, t in cover]
    sts = (K.api._Stream * WINDOWS)()
    rgs = (K.api._BlockRange * WINDOWS)()
    for i, ((f, t), d) in enumerate(zip(cover, dsts)):
        sts[i].d_src, sts[i].n, sts[i].d_dst, sts[i].dst_cap = comp.data_ptr(), nb, d.data_ptr(), (t - f) * bs
        rgs[i].from_block, rgs[i].to_block, rgs[i].from_bit = f, t, pos[f - 1][0]
    wpats = [pats[i % PATTERNS] for i in range(WINDOWS)]

    def base_windows():
        assert L.knz_dev_decompress_many_range(c.h, sts, rgs, WINDOWS, None) == 0
        res = []
        for i, (o, d) in enumerate(zip(offs, dsts)):
            lo = (cover[i][0] - 1) * bs
            buf = d[: int(sts[i].out_bytes)].cpu().numpy().tobytes()
            res.append([lo + p for p in host_find(buf, wpats[i], o - lo, o - lo + WINDOW)])
        return res
    wantw = [host_find(raw, wpats[i], o, o + WINDOW) for i, o in enumerate(offs)]
    find_case("64_windows_of_1MiB", [(wpats[i], o, WINDOW) for i, o in enumerate(offs)], base_windows, wantw)
    out["cases"]["64_windows_of_1MiB"]["baseline_blocks_decoded"] = int(sum(t - f for f, t in cover))
    c.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=400, help="seconds one configuration may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "find_rate.json"))
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.warmup)
    out = {"reps": a.reps, "warmup": a.warmup, "unit": "ms of wall clock around the calls, tables built beforehand, data resident on the device",
           "corpus": "bench_corpus.s_silesia()", "patterns": "%d-byte pieces of the corpus at random offsets" % PATTERN,
           "baseline": "knz_dev_decompress_many (windows: knz_dev_decompress_many_range, one hinted entry per window) into device buffers, a copy to "
           "the host, bytes.find restarted at hit + 1",
           "kernel_times_us": "HIP event pairs around each launch (knz_last_kernel_times), launches of one name summed: the find tail alone", "results": {}}
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
