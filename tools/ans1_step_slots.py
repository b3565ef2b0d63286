#!/usr/bin/env python3
"""Issue slots of the order-1 rANS decoder's hand-written loops (kanzi-go_amd/csrc/ans1.hip, knz_ans1_decode_lds2_kernel).

The loops are inline asm: hipcc preprocesses them (macros expanded, operands named) when it writes the kernel's gfx950 assembly
(-S --cuda-device-only), where each one stands between ';;#ASMSTART' and ';;#ASMEND'. This script finds the loops there by their labels
(.Lknz_a1t_loop_: the default form, sixteen steps a turn; .Lknz_a1d_loop_: round 5's, KNZ_ANS1_R5_LOOP, four steps a turn) and counts TEXT
only, nothing is interpreted: one slot per instruction line between the label and the back edge (an s_nop N or an s_waitcnt is one line,
so one slot: a lone wave pays per instruction it issues, profiles/r02_lone_wave_latencies.md); one step per ds_read_b64 (the window read);
and for each LDS read the lines between it and the s_waitcnt lgkmcnt(N) that first covers it, which is its shadow. LDS operations return
in order and lgkmcnt(N) lets the N newest stay in flight, so a wait covers an operation when at least N were issued behind it. The turn is
read twice in a row, so a read that only a wait of the next turn covers is counted across the back edge, and said to be carried.
'outside the pair's shadow' = the slots of a step that are not between the read of cum[k + 1] and the wait of the pair.

usage: tools/ans1_step_slots.py [--asm FILE]     (without --asm: compiles kanzi-go_amd/csrc/knz_gpu.hip to assembly with $HIPCC)"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = (("default (16 steps a turn)", ".Lknz_a1t_loop_"), ("KNZ_ANS1_R5_LOOP (4 steps a turn)", ".Lknz_a1d_loop_"))
SLOT_NS, BRANCH_NS, LDS_NS = 2.41, 10.0, 27.0         # profiles/r02_lone_wave_latencies.md


def device_asm():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "knz_gpu.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-Wno-unused-variable", "-Wno-unused-value",
                               "-o", out, os.path.join(ROOT, "kanzi-go_amd", "csrc", "knz_gpu.hip")])
        return open(out).read()


def loop_lines(text, label):
    """the instruction lines of the first inline-asm loop with that label, from the label to its back edge (included)"""
    m = re.search(r"^(" + re.escape(label) + r"\d+):\s*$", text, re.M)
    if m is None:
        return None
    name = m.group(1)
    lines = []
    for ln in text[m.end():].splitlines():
        ln = ln.split(";")[0].strip()
        if not ln or ln.endswith(":") or ln.startswith("."):
            continue
        lines.append(ln)
        if ln.startswith("s_cbranch") and ln.split()[-1] == name:
            return lines
    raise SystemExit(f"{label}: no back edge found")


def count(lines):
    steps = sum(1 for ln in lines if ln.startswith("ds_read_b64"))
    n = len(lines)
    two = lines + lines                                       # this turn and the next
    lds = [i for i, ln in enumerate(two) if ln.startswith("ds_")]
    shadows = []                                              # (the read, lines to the wait that covers it, second of a pair, carried to the next turn)
    for k, i in enumerate(lds):
        if i >= n or not two[i].startswith("ds_read"):
            continue
        for j in range(i + 1, len(two)):
            w = re.match(r"s_waitcnt\s+lgkmcnt\((\d+)\)", two[j])
            if w and sum(1 for x in lds[k + 1:] if x < j) >= int(w.group(1)):
                shadows.append((two[i].split()[0] + (" offset:2" if "offset:2" in two[i] else ""), j - i - 1, "offset:2" in two[i], j >= n))
                break
        else:
            raise SystemExit(f"no wait covers line {i}: {two[i]}")
    pair = [s for _mn, s, second, _c in shadows if second]    # the pair's shadow: from the read of cum[k + 1] (offset:2) to the pair's wait
    return steps, shadows, pair


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", default="", help="the library's device assembly (hipcc -S --cuda-device-only); compiled when not given")
    args = ap.parse_args()
    text = open(args.asm).read() if args.asm else device_asm()
    rows = []
    for title, label in FORMS:
        lines = loop_lines(text, label)
        if lines is None:
            raise SystemExit(f"no loop {label}* in the assembly")
        steps, shadows, pair = count(lines)
        turn = len(lines)
        in_pair = sum(pair)
        outside = (turn - in_pair) / steps
        by_kind = {}
        for mn, sh, _second, carried in shadows:
            by_kind.setdefault(mn, []).append((sh, carried))
        # model as in the issue: slots outside the pair's shadow at SLOT_NS, one LDS round trip per step, one taken branch per turn
        model = outside * SLOT_NS + LDS_NS + BRANCH_NS / steps
        rows.append((title, steps, turn, turn / steps, in_pair / steps, outside, model))
        print(f"{title}: {steps} steps a turn, {turn} slots a turn = {turn / steps:.2f} a step; "
              f"{in_pair / steps:.2f} a step in the pair's shadow, {outside:.2f} outside it")
        for mn, ss in by_kind.items():
            carried = [x for x, c in ss if c]
            print(f"    {mn}: {len(ss)} reads a turn, slots between the read and the wait that covers it: {sorted(set(x for x, _c in ss))}"
                  + (f"; {len(carried)} of them carried to the next turn's first wait ({sorted(set(carried))} slots, the back edge's among them)" if carried else ""))
        print(f"    model: {outside:.2f} x {SLOT_NS} + {LDS_NS} + {BRANCH_NS} / {steps} = {model:.1f} ns a step (without the tile work)")
    print()
    print("| form | steps a turn | slots a turn | slots a step | in the pair's shadow | outside it | model ns a step |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]:.2f} | {r[4]:.2f} | {r[5]:.2f} | {r[6]:.1f} |")
    if rows[0][5] >= rows[1][5]:
        print("the default form has NO fewer slots outside the pair's shadow than KNZ_ANS1_R5_LOOP", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
