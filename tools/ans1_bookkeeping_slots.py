#!/usr/bin/env python3
"""Issue slots of the order-1 rANS bookkeeping loops, counted from the library's gfx950 assembly (hipcc -S --cuda-device-only), next to
tools/ans1_step_slots.py and in its manner: text only, one slot per instruction line (an s_nop N or an s_waitcnt is one line, so one slot: a lone
wave pays per instruction it issues, profiles/r02_lone_wave_latencies.md).

  encoder   knz_ans1_encode_asm_kernel (two waves) and knz_ans1_encode_asm1_kernel (one wave, KNZ_ANS1_ENC_ONE_WAVE): the coding wave's turn of
            48 steps = the shortest way round the loop that holds the 48 global_load_dwordx4 (the polling loop behind a full ring is not on
            it; in the one-wave kernel a group without words skips its stores: counted without any and with all three); the placer's turn = the way round the loop that holds the stores of the words (global_store_short), through every block that stores (all three groups of a
            turn have words) and past its polling loop.
  walk      knz_dec_walk_blocks_kernel, knz_ans1_walk_header inlined: a frequency group = the way round the loop whose block holds s_min_u32 and
            s_max_u32 (the window shift is not on it); a context = the way round the loop of the 256 contexts with ONE group on it, less that
            group, once past the block that counts an alphabet's masks (v_bcnt_u32_b32: 255 symbols or fewer) and once not (the flag: all 256).

A way round a loop is found on the control-flow graph of the kernel's basic blocks (labels and branches as text): the shortest cycle through the
blocks named above that enters no block with an s_sleep. Nothing is interpreted or executed.

usage: tools/ans1_bookkeeping_slots.py [--asm FILE]     (without --asm: compiles kanzi-go_amd/csrc/knz_gpu.hip to assembly with $HIPCC)"""
import argparse
import heapq
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT_NS = 2.41                                         # profiles/r02_lone_wave_latencies.md


def device_asm():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "knz_gpu.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-Wno-unused-variable", "-Wno-unused-value",
                               "-o", out, os.path.join(ROOT, "kanzi-go_amd", "csrc", "knz_gpu.hip")])
        return open(out).read()


def blocks_of(text, kernel):
    """basic blocks of a kernel: [(label or None, [instruction lines])], and label -> block index"""
    lines = text.splitlines()
    start = next((i for i, ln in enumerate(lines) if re.match(r"^_Z\d+" + re.escape(kernel) + r"\w*:", ln)), None)
    if start is None:
        return None, None
    blocks, index = [[None, []]], {}
    for ln in lines[start + 1:]:
        if ln.startswith(".Lfunc_end"):
            break
        ln = ln.split(";")[0].strip()
        m = re.match(r"^(\.LBB\d+_\d+):$", ln)
        if m:
            blocks.append([m.group(1), []])
            index[m.group(1)] = len(blocks) - 1
            continue
        if not ln or ln.endswith(":") or ln.startswith("."):
            continue
        blocks[-1][1].append(ln)
        if ln.startswith("s_cbranch") or ln.startswith("s_branch") or ln.startswith("s_endpgm"):
            blocks.append([None, []])                  # what follows a branch is a block of its own
    return blocks, index


def successors(blocks, index, i):
    body = blocks[i][1]
    last = body[-1] if body else ""
    out = []
    if last.startswith("s_branch") or last.startswith("s_cbranch"):
        t = last.split()[-1]
        if t in index:
            out.append(index[t])
    if not last.startswith("s_branch") and not last.startswith("s_endpgm") and i + 1 < len(blocks):
        out.append(i + 1)
    return out


def shortest(blocks, index, src, dst, banned):
    """fewest instruction lines from the start of block src to the start of block dst (src's lines counted, dst's not)"""
    dist, heap = {src: 0}, [(0, src)]
    while heap:
        d, i = heapq.heappop(heap)
        if d > dist.get(i, 1 << 60):
            continue
        for j in successors(blocks, index, i):
            nd = d + len(blocks[i][1])
            if j == dst:
                dist.setdefault(("end", j), nd)
                dist[("end", j)] = min(dist[("end", j)], nd)
                continue
            if j in banned:
                continue
            if nd < dist.get(j, 1 << 60):
                dist[j] = nd
                heapq.heappush(heap, (nd, j))
    return dist.get(("end", dst))


def cycle(blocks, index, through, banned=()):
    """instruction lines of the shortest cycle that visits the blocks of `through` in that order"""
    banned = set(banned) | {i for i, b in enumerate(blocks) if any(x.startswith("s_sleep") for x in b[1])}
    total = 0
    for a, b in zip(through, through[1:] + through[:1]):
        d = shortest(blocks, index, a, b, banned - {a, b})
        if d is None:
            raise SystemExit(f"no way from block {blocks[a][0]} to block {blocks[b][0]}")
        total += d
    return total


def holding(blocks, *starts, count=1):
    return [i for i, b in enumerate(blocks) if all(sum(1 for x in b[1] if x.startswith(s)) >= count for s in starts)]


def encoder(text, kernel, two_waves):
    blocks, index = blocks_of(text, kernel)
    if blocks is None:
        return None
    loads = [i for i, b in enumerate(blocks) if any(x.startswith("global_load_dwordx4") for x in b[1])]
    n_loads = sum(1 for i in loads for x in blocks[i][1] if x.startswith("global_load_dwordx4"))
    coder = cycle(blocks, index, loads)
    stores = [i for i, b in enumerate(blocks) if any(x.startswith("global_store_short") for x in b[1])]
    if two_waves:                                      # the placer's loop stands in front of the coding wave's (the epilogue's tail bytes are stored behind both)
        stores = [i for i in stores if i < loads[0]][:3]
        return n_loads, coder, cycle(blocks, index, stores) if len(stores) == 3 else None
    stores = [i for i in stores if i > loads[-1]][:3]  # one wave: the flush is on the coding wave's turn, a group's stores skipped when it has no word
    return n_loads, coder, cycle(blocks, index, loads + stores) if len(stores) == 3 else None


def walk(text):
    blocks, index = blocks_of(text, "knz_dec_walk_blocks_kernel")
    group = holding(blocks, "s_min_u32", "s_max_u32") if blocks else []
    if len(group) != 1:                                # (the parent's tree walks through the generic reader: no such block)
        return None
    g = group[0]
    per_group = cycle(blocks, index, [g])
    masks = [i for i in holding(blocks, "v_bcnt_u32_b32") if any("row_bcast:31" in x for x in blocks[i][1]) and abs(i - g) < 40]
    tail = [i for i in holding(blocks, "v_cndmask_b32") if g < i < g + 40][:1]                  # the block that keeps the context's position in its lane
    if len(masks) != 1 or not tail:
        raise SystemExit("the walk's context blocks were not found")
    with_masks = cycle(blocks, index, [masks[0], g, tail[0]]) - len(blocks[g][1])
    with_flag = cycle(blocks, index, [g, tail[0]], banned=masks) - len(blocks[g][1])
    return per_group, with_flag, with_masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", default="", help="the library's device assembly (hipcc -S --cuda-device-only); compiled when not given")
    args = ap.parse_args()
    text = open(args.asm).read() if args.asm else device_asm()
    print("| loop | slots | per | model |")
    print("|---|---|---|---|")
    has_two = blocks_of(text, "knz_ans1_encode_asm1_kernel")[0] is not None      # the parent's tree has the one-wave kernel alone, under the name the bench keys
    forms = (("two waves", "knz_ans1_encode_asm_kernel", True), ("one wave (KNZ_ANS1_ENC_ONE_WAVE)", "knz_ans1_encode_asm1_kernel", False)) if has_two else \
            (("one wave", "knz_ans1_encode_asm_kernel", False),)
    for title, kernel, two in forms:
        n_loads, coder, placer = encoder(text, kernel, two)
        print(f"| encoder, {title}: coding wave's turn ({n_loads} steps) | {coder} | {coder / n_loads:.2f} a step | {coder * SLOT_NS / n_loads:.1f} ns a step, {coder * SLOT_NS / n_loads * 1048576 / 1e6:.1f} ms a 4 MiB chunk |")
        if placer is not None and not two:
            print(f"| encoder, {title}: coding wave's turn, all three groups with words | {placer} | {placer / n_loads:.2f} a step | {placer * SLOT_NS / n_loads:.1f} ns a step, {placer * SLOT_NS / n_loads * 1048576 / 1e6:.1f} ms a 4 MiB chunk |")
        elif placer is not None:
            print(f"| encoder, {title}: placer's turn, all three groups with words | {placer} | {placer / n_loads:.2f} a step | {placer * SLOT_NS:.0f} ns a turn against the coding wave's {coder * SLOT_NS:.0f} |")
    w = walk(text)
    if w is not None and w[0] is not None:
        print(f"| walk: a frequency group | {w[0]} | group | {w[0] * SLOT_NS:.1f} ns |")
        print(f"| walk: a context outside its groups, full-alphabet flag | {w[1]} | context | {w[1] * SLOT_NS:.0f} ns |")
        print(f"| walk: a context outside its groups, alphabet masks counted | {w[2]} | context | {w[2] * SLOT_NS:.0f} ns |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
