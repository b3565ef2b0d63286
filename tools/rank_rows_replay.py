#!/usr/bin/env python3
"""Replay of the hand-written packed inverse RANK loop (kanzi-go_amd/csrc/rank_inv_asm.h: knz_rank_rows_packed) on the CPU.

The header is put through the C preprocessor, the instruction text of the loop's asm statement is taken as it stands (operands keep their
names, %[e0] is a register called e0) and interpreted one wave wide. What comes out is what a lone wave pays for on the device: instructions
issued (slots) and taken branches, next to the decoded bytes, which
are compared with the oracle's inverse. So a layout's cost can be predicted before it is measured, and two layouts are compared by giving two
headers (e.g. one written out of an earlier commit with `git show`).

    python tools/rank_rows_replay.py                         # block 2 of the bench corpus, its first 256 KiB of ranks, the header in the tree
    python tools/rank_rows_replay.py --block 2 --ranks 0     # the whole block (slow: the interpreter does ~0.3 M instructions a second)
    python tools/rank_rows_replay.py --header /tmp/parent.h --header kanzi-go_amd/csrc/rank_inv_asm.h
    python tools/rank_rows_replay.py --file ranks.bin        # any file of ranks

The instruction subset is the one the header uses; an instruction the interpreter does not know is an error, never skipped.
"""
import argparse
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "kanzi-go_amd", "csrc", "rank_inv_asm.h")
M32 = 0xFFFFFFFF
T_BWT, T_RANK = 1, 8                                         # the oracle's transform ids


def asm_text(header, defines=(), func="knz_rank_rows_packed"):
    """the instruction text of the asm statement of `func`, preprocessed, and the operands that are bound to a named register"""
    src = '#define __device__\n#define __forceinline__\n#include "%s"\n' % os.path.abspath(header)
    cmd = [os.environ.get("CXX", "c++"), "-E", "-P", "-x", "c++", "-"] + ["-D" + d for d in defines]
    out = subprocess.run(cmd, input=src, capture_output=True, text=True, check=True).stdout
    at = out.index("asm volatile(", out.index("void %s(" % func))
    pos = at + len("asm volatile(")
    parts = []
    while True:
        m = re.compile(r'\s*(?:"((?:[^"\\]|\\.)*)"|(:))').match(out, pos)
        if m is None or m.group(2):
            break
        parts.append(m.group(1).encode().decode("unicode_escape"))
        pos = m.end()
    fixed = dict(re.findall(r'\[(\w+)\]\s*"[=+&]*\{(s\d+)\}"', out[pos:out.index(";", pos)]))
    return "".join(parts), fixed


class Wave:
    """one wave of 64 lanes running the loop's instruction text"""

    def __init__(self, text, fixed):
        self.prog, self.labels, self.fixed = [], {}, fixed
        for line in text.split("\n"):
            line = re.sub(r"/\*.*?\*/", "", line).strip()
            if not line:
                continue
            if line.endswith(":"):
                self.labels[line[:-1]] = len(self.prog)
                continue
            op, _, rest = line.partition(" ")
            mods = {}
            m = re.search(r"\s(quad_perm:\[[\d,]+\]|wave_shr:1|wave_ror:1)", rest)
            if m:
                mods["dpp"] = m.group(1)
                mods["bound"] = "bound_ctrl:1" in rest
                rest = rest[:m.start()]
            self.prog.append((op, [a.strip() for a in rest.split(",")] if rest.strip() else [], mods))
        self.s, self.v = {}, {}
        self.scc = 0
        self.exec = np.ones(64, dtype=bool)
        self.taken = 0

    # ---- operands
    def _name(self, a):
        a = a[2:-1] if a.startswith("%[") else a
        return self.fixed.get(a, a)

    def sget(self, a):
        a = self._name(a)
        if re.fullmatch(r"-?(0x[0-9a-fA-F]+|\d+)", a):
            return int(a, 0) & M32
        return self.s[a]

    def vget(self, a):
        a = self._name(a)
        if a in self.v:
            return self.v[a]
        return np.full(64, self.sget(a), dtype=np.uint32)

    def vset(self, a, val, mask=None):
        a = self._name(a)
        m = self.exec if mask is None else (self.exec & mask)
        old = self.v.get(a)
        if old is None:
            old = np.zeros(64, dtype=np.uint32)
        self.v[a] = np.where(m, val.astype(np.uint32), old)

    def pair(self, a):
        m = re.fullmatch(r"s\[(\d+):(\d+)\]", a)
        return ("s%d" % int(m.group(1)), "s%d" % int(m.group(2)))

    def dpp(self, src, mods):
        """(value per lane, lanes that have a source)"""
        d = mods["dpp"]
        lanes = np.arange(64)
        if d == "wave_shr:1":
            return src[(lanes - 1) % 64], (lanes > 0) | mods["bound"]
        if d == "wave_ror:1":
            return src[(lanes - 1) % 64], np.ones(64, dtype=bool)
        p = [int(x) for x in d[len("quad_perm:["):-1].split(",")]
        return src[(lanes & ~3) + np.array(p)[lanes & 3]], np.ones(64, dtype=bool)

    # ---- run
    def run(self, mem, out, limit=1 << 62):
        """mem: the ranks; out: bytearray of the decoded rows. Returns the instructions issued; self.taken counts the taken branches"""
        pc, n = 0, 0
        prog, s = self.prog, self.s
        while pc < len(prog):
            op, a, mods = prog[pc]
            n += 1
            if n > limit:
                raise RuntimeError("instruction limit reached: the loop does not end")
            nxt = pc + 1
            if op in ("s_branch", "s_cbranch_scc0", "s_cbranch_scc1"):
                if op == "s_branch" or self.scc == (op[-1] == "1"):
                    nxt = self.labels[a[0]]
                    self.taken += 1
            elif op == "s_load_dwordx8":
                lo, _ = self.pair(a[0])
                off = self.sget(a[2])
                assert off % 4 == 0 and off + 32 <= len(mem), ("scalar load out of bounds", off, len(mem))
                for i in range(8):
                    s["s%d" % (int(lo[1:]) + i)] = int.from_bytes(mem[off + 4 * i: off + 4 * i + 4], "little")
            elif op == "s_load_dwordx4":
                lo, _ = self.pair(a[0])
                off = self.sget(a[2])
                assert off % 4 == 0 and off + 16 <= len(mem), ("scalar load out of bounds", off, len(mem))
                for i in range(4):
                    s["s%d" % (int(lo[1:]) + i)] = int.from_bytes(mem[off + 4 * i: off + 4 * i + 4], "little")
            elif op in ("s_waitcnt", "s_nop"):
                pass
            elif op == "s_mov_b32":
                s[self._name(a[0])] = self.sget(a[1])
            elif op == "s_mov_b64":
                if a[0] == "exec":
                    v = int(a[1], 0) & 0xFFFFFFFFFFFFFFFF
                    self.exec = np.array([(v >> i) & 1 for i in range(64)], dtype=bool)
                else:
                    (d0, d1), (s0, s1) = self.pair(a[0]), self.pair(a[1])
                    s[d0], s[d1] = s[s0], s[s1]
            elif op == "s_or_b64":
                (d0, d1), (x0, x1), (y0, y1) = self.pair(a[0]), self.pair(a[1]), self.pair(a[2])
                s[d0], s[d1] = s[x0] | s[y0], s[x1] | s[y1]
                self.scc = int((s[d0] | s[d1]) != 0)
            elif op in ("s_or_b32", "s_and_b32"):
                x, y = self.sget(a[1]), self.sget(a[2])
                r = (x | y) if op == "s_or_b32" else (x & y)
                s[self._name(a[0])] = r
                self.scc = int(r != 0)
            elif op == "s_min_u32":
                x, y = self.sget(a[1]), self.sget(a[2])
                s[self._name(a[0])] = min(x, y)
                self.scc = int(x < y)
            elif op in ("s_add_u32", "s_add_i32"):
                r = self.sget(a[1]) + self.sget(a[2])
                s[self._name(a[0])] = r & M32
                self.scc = int(r > M32)                     # (nobody here reads the carry / overflow)
            elif op == "s_addk_i32":
                s[self._name(a[0])] = (self.sget(a[0]) + int(a[1], 0)) & M32
            elif op == "s_lshr_b32":
                r = self.sget(a[1]) >> (self.sget(a[2]) & 31)
                s[self._name(a[0])] = r
                self.scc = int(r != 0)
            elif op == "s_bfe_u32":
                c = self.sget(a[2])
                r = (self.sget(a[1]) >> (c & 31)) & ((1 << ((c >> 16) & 0x7F)) - 1)
                s[self._name(a[0])] = r
                self.scc = int(r != 0)
            elif op == "s_bitcmp0_b32":
                self.scc = int(((self.sget(a[0]) >> (self.sget(a[1]) & 31)) & 1) == 0)
            elif op in ("s_cmp_le_u32", "s_cmp_eq_u32", "s_cmp_gt_u32", "s_cmp_lt_u32", "s_cmp_lg_u32"):
                x, y = self.sget(a[0]), self.sget(a[1])
                self.scc = int({"le": x <= y, "eq": x == y, "gt": x > y, "lt": x < y, "lg": x != y}[op[6:8]])
            elif op == "v_mov_b32_e32":
                self.vset(a[0], self.vget(a[1]))
            elif op == "v_mov_b32_dpp":
                val, ok = self.dpp(self.vget(a[1]), mods)
                self.vset(a[0], val, ok)
            elif op in ("v_max_i32_dpp", "v_min_i32_dpp"):
                val, ok = self.dpp(self.vget(a[1]), mods)
                x, y = val.astype(np.int32), self.vget(a[2]).astype(np.int32)
                self.vset(a[0], np.maximum(x, y) if op[2:5] == "max" else np.minimum(x, y), ok)
            elif op == "v_cndmask_b32_dpp":
                val, ok = self.dpp(self.vget(a[1]), mods)
                self.vset(a[0], np.where(self.v["vcc"], self.vget(a[2]), val), ok)
            elif op == "v_cndmask_b32_e32":
                self.vset(a[0], np.where(self.v["vcc"], self.vget(a[2]), self.vget(a[1])))
            elif op == "v_cndmask_b32_e64":
                self.vset(a[0], np.where(self.v[self._name(a[3])], self.vget(a[2]), self.vget(a[1])))
            elif op in ("v_cmp_ge_u32_e32", "v_cmp_gt_i32_e32", "v_cmp_gt_i32_e64"):
                x, y = self.vget(a[1]), self.vget(a[2])
                r = (x >= y) if "ge_u32" in op else (x.astype(np.int32) > y.astype(np.int32))
                self.v[self._name(a[0])] = r & self.exec
            elif op == "v_min_i32_e32":
                self.vset(a[0], np.minimum(self.vget(a[1]).astype(np.int32), self.vget(a[2]).astype(np.int32)))
            elif op == "v_add_u32_e32":
                self.vset(a[0], self.vget(a[1]) + self.vget(a[2]))
            elif op == "v_lshrrev_b32_e32":
                self.vset(a[0], self.vget(a[2]) >> (self.vget(a[1]) & 31))
            elif op == "v_and_b32_e32":
                self.vset(a[0], self.vget(a[1]) & self.vget(a[2]))
            elif op == "v_and_or_b32":
                self.vset(a[0], (self.vget(a[1]) & self.vget(a[2])) | self.vget(a[3]))
            elif op == "v_lshl_or_b32":
                self.vset(a[0], (self.vget(a[1]) << (self.vget(a[2]) & 31)) | self.vget(a[3]))
            elif op == "v_alignbyte_b32":
                wide = (self.vget(a[1]).astype(np.uint64) << np.uint64(32)) | self.vget(a[2]).astype(np.uint64)
                self.vset(a[0], (wide >> (np.uint64(8) * (self.vget(a[3]).astype(np.uint64) & np.uint64(3)))) & np.uint64(M32))
            elif op == "v_perm_b32":
                wide = (self.vget(a[1]).astype(np.uint64) << np.uint64(32)) | self.vget(a[2]).astype(np.uint64)
                sel = self.vget(a[3])
                r = np.zeros(64, dtype=np.uint64)
                for b in range(4):
                    sb = (sel >> (8 * b)) & 0xFF
                    assert (sb < 8).all(), "v_perm_b32 selector above 7"
                    r |= ((wide >> (np.uint64(8) * sb.astype(np.uint64))) & np.uint64(0xFF)) << np.uint64(8 * b)
                self.vset(a[0], r)
            elif op == "v_readlane_b32":
                s[self._name(a[0])] = int(self.vget(a[1])[self.sget(a[2]) & 63])
            elif op == "v_writelane_b32":
                v = self.vget(a[0]).copy()
                v[self.sget(a[2]) & 63] = self.sget(a[1])
                self.v[self._name(a[0])] = v
            elif op == "global_store_dword":
                offs, vals = self.vget(a[0]), self.vget(a[1])
                for ln in np.nonzero(self.exec)[0]:
                    o = int(offs[ln])
                    assert o + 4 <= len(out), ("store out of bounds", o, len(out))
                    out[o:o + 4] = int(vals[ln]).to_bytes(4, "little")
            else:
                raise NotImplementedError(op)
            pc = nxt
        return n


def replay(header, ranks, defines=()):
    """-> (decoded bytes, instructions issued, taken branches) of the whole rows of `ranks`"""
    w = Wave(*asm_text(header, defines))
    n = len(ranks) & ~63
    lane = np.arange(64, dtype=np.uint32)
    for k in range(4):
        w.v["e%d" % k] = (64 * k + lane).astype(np.uint32)
        w.v["q%d" % k] = np.zeros(64, dtype=np.uint32)
    w.v["vff"] = np.full(64, 0xFF, dtype=np.uint32)
    w.v["vmax"] = np.full(64, 0x7FFFFFFF, dtype=np.uint32)
    w.v["lane"] = lane
    w.v["sel1"] = np.where(lane & 1, 0x03070105, 0x06020400).astype(np.uint32)
    w.v["sel2"] = np.where(lane & 2, 0x03020706, 0x05040100).astype(np.uint32)
    w.v["doff"] = (4 * (4 * (lane & 3) + ((lane >> 2) & 3))).astype(np.uint32)
    w.v["vcc"] = np.zeros(64, dtype=bool)
    for nm in ("ob", "racc", "tt", "vnew", "es", "qx", "vqc", "qs", "t8", "vbase"):     # (the loop's own registers start as whatever was there)
        w.v[nm] = np.full(64, 0xDEADBEEF, dtype=np.uint32)
    w.s.update({"src": 0, "dbase": 0, "nbytes": n, "i8": 0})
    w.s["lastoff"] = n - (32 if any(op == "s_load_dwordx8" for op, _a, _m in w.prog) else 16)
    out = bytearray(n)
    total = w.run(bytes(ranks[:n]), out, limit=200 * n + 10000)
    return bytes(out), total, w.taken


def block_ranks(block, block_size=8 << 20):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import bench_corpus
    import oracle_lib as O
    base = bench_corpus.s_silesia(bench_corpus.SILESIA_SIZE)
    data = base[block * block_size:(block + 1) * block_size].tobytes()
    O.set_ctx(block_size, O.entropy_type("ANS1"))
    return O.transform_forward(T_RANK, O.transform_forward(T_BWT, data))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--header", action="append", default=[], help="rank_inv_asm.h to replay (repeat to compare layouts; default: the tree's)")
    ap.add_argument("--define", action="append", default=[], help="preprocessor definition for the headers, NAME=VALUE")
    ap.add_argument("--block", type=int, default=2, help="block of the bench corpus (8 MiB blocks) whose ranks are replayed")
    ap.add_argument("--file", default="", help="a file of ranks instead")
    ap.add_argument("--ranks", type=int, default=256 << 10, help="ranks replayed from the start of the block, 0 = all")
    ap.add_argument("--windows", type=int, default=1, help="take the ranks as this many windows spread evenly over the block instead of its start. Which way the "
                                                           "loop goes depends on the ranks alone, never on the list, so the counts are those of the windows; the "
                                                           "decoded bytes are not (the list is not what it would be there) and are not checked")
    ap.add_argument("--no-check", action="store_true", help="do not compare the decoded bytes with the oracle's inverse")
    args = ap.parse_args()
    ranks = open(args.file, "rb").read() if args.file else block_ranks(args.block)
    whole = len(ranks)
    if args.ranks and args.windows > 1:
        size = (args.ranks // args.windows) & ~63
        step = ((whole - size) // (args.windows - 1)) & ~63
        ranks = b"".join(ranks[k * step: k * step + size] for k in range(args.windows))
        args.no_check = True
    elif args.ranks:
        ranks = ranks[:args.ranks]
    ranks = ranks[:len(ranks) & ~63]
    a = np.frombuffer(ranks, dtype=np.uint8)
    groups = len(a) // 16
    g = a.reshape(groups, 16)
    high = int((g >= 64).any(axis=1).sum())
    zero = int((g == 0).all(axis=1).sum())
    print(f"{len(a)} of {whole} ranks, {groups} groups: {high} with a rank >= 64, {groups - high - zero} low, {zero} all zero; {int((a >= 64).sum())} high ranks")
    want = None
    if not args.no_check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib as O
        want = O.transform_inverse(T_RANK, bytes(ranks), len(ranks) + 64)
    for h in args.header or [HEADER]:
        out, total, tk = replay(h, ranks, args.define)
        ok = "" if want is None else ("   decoded bytes == oracle" if out == want else "   DECODED BYTES DIFFER FROM THE ORACLE")
        print(f"{h}{ok}")
        print(f"  instructions {total} ({total / groups:.2f} per group), taken branches {tk} ({tk / groups:.3f} per group)")
        print(f"  at 2.4 ns a slot and 10 ns a taken branch, scaled to the block: {(total * 2.4 + tk * 10) * whole / len(a) / 1e6:.1f} ms")
        if want is not None and out != want:
            sys.exit(1)


if __name__ == "__main__":
    main()
