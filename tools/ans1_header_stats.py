#!/usr/bin/env python3
"""What the block walker has to read of an order-1 rANS chunk header, counted on the CPU for blocks of the bench corpus (bench_corpus.py, S-silesia,
8 MiB blocks, BWT+RANK+ZRLT in front of ANS1: the bench's default configuration). The oracle compresses one block; the parser of
tests/ans1_walk_cases.py (plain Python) walks the chunk headers of its stream and this script prints, per chunk: the contexts that have symbols,
their mean number of symbols, the frequency groups (one dependent read each for the walk) and the bits of the header.

usage: tools/ans1_header_stats.py [BLOCK ...]     (default: blocks 0 and 2: a text-like block and one of the executable-like blocks that form the long chains)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench_corpus  # noqa: E402
import oracle_lib as O  # noqa: E402
import ans1_walk_cases as W  # noqa: E402

BS = 8 << 20
CHUNK = 4 << 20


def read_varint(bits, pos):
    res = 0
    for i in range(4):
        v = bits.get(pos, 8)
        pos += 8
        res |= (v & 0x7F) << (7 * i)
        if v < 128:
            return res, pos
    return res | ((bits.get(pos, 8) & 0x0F) << 28), pos + 8


def main():
    O.build()
    corpus = bench_corpus.s_silesia()
    for b in [int(x) for x in sys.argv[1:]] or [0, 2]:
        block = corpus[b * BS:(b + 1) * BS].tobytes()
        bits = W.Bits(O.compress(block, "BWT+RANK+ZRLT", "ANS1", BS))
        (_f, payload, _n), = W.block_payloads(bits)
        pos, pre = W.chunk_start(bits, payload)
        block_groups = 0
        for k in range((pre + CHUNK - 1) // CHUNK):
            start = pos
            _lr, ctxs, pos = W.parse_chunk_header(bits, pos)
            used = [c for _at, c, _l, _w in ctxs if c]
            groups = sum(len(w) for _at, _c, _l, w in ctxs)
            block_groups += groups
            print(f"block {b} chunk {k}: {len(used)} contexts with symbols, mean {sum(used) / max(1, len(used)):.1f} symbols, {groups} frequency groups "
                  f"({groups / max(1, len(used)):.1f} a context), header {pos - start} bits")
            size, pos = read_varint(bits, pos)
            pos += 128 + 8 * size
        print(f"block {b}: {block_groups} groups + {256 * ((pre + CHUNK - 1) // CHUNK)} alphabets = the walk's dependent reads of the block ({pre} bytes behind the transforms)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
