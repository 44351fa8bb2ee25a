#!/usr/bin/env python3
"""Count what sits on a lone wave's dependent chain in a device assembly file (hipcc -S --cuda-device-only): per kernel
and per loop the instructions, the hazard no-ops with their wait states, the lane reads and writes that reload and spill
scalars, and the waits: the instructions of a lone wave's chain that compute nothing (what they cost was measured in
profiles/phase_chain.md: less than the four cycles of a vector instruction each).

usage: chain_table.py A.s [--kernel SUBSTRING] [--min N] [--follow]

A loop is the text from a backward branch's target to the branch (inner loops are counted in their outer ones too);
loops shorter than --min instructions (default 40) are left out.  The column dpp-dpp counts the no-ops that sit between
two DPP instructions (the steps of a reduction tree); --follow lists which opcode follows the no-ops of each region.
Kernels are named by their demangled names; --kernel keeps those that contain the substring.  CPU only."""
import collections
import os
import re
import subprocess
import sys

CXXFILT = next((p for p in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "/opt/rocm/lib/llvm/bin/llvm-cxxfilt") if os.path.exists(p)), "c++filt")


def kernels(path):
    """{mangled name: [("label", name) | ("ins", text)]} -- as tools/asm_compare.py reads a file"""
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        s = line.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            out[name] = body
            name = None
        elif re.match(r"^\.LBB\w+:", s):
            body.append(("label", s[:-1]))
        elif s and not s.startswith("."):
            body.append(("ins", s))
    return out


def demangled(names):
    if not names:
        return {}
    r = subprocess.run([CXXFILT] + list(names), capture_output=True, text=True, check=True)
    return {n: d.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0] for n, d in zip(names, r.stdout.splitlines())}


def loops(body):
    """-> (instructions, [(first, last)] of every loop, positions in the instruction list)"""
    ins, pos = [], {}
    for kind, s in body:
        if kind == "label":
            pos[s] = len(ins)
        else:
            ins.append(s)
    out = []
    for k, s in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\w+)", s)
        if m and pos.get(m.group(1), k + 1) <= k:
            out.append((pos[m.group(1)], k))
    return ins, sorted(set(out))


def is_dpp(s):
    op = s.split()[0]
    return op.endswith("_dpp") or " quad_perm:" in s or " row_" in s or " wave_" in s


def count(ins, a, b):
    """figures of ins[a .. b]; the instruction after the region's last no-op is looked up past its end"""
    c = collections.Counter()
    follow = collections.Counter()
    for k in range(a, b + 1):
        op = ins[k].split()[0]
        c["ins"] += 1
        if op == "s_nop":
            c["s_nop"] += 1
            c["wait_states"] += int(ins[k].split()[1], 0) + 1
            nxt = next((ins[j] for j in range(k + 1, len(ins)) if not ins[j].startswith("s_nop")), "")
            prv = next((ins[j] for j in range(k - 1, -1, -1) if not ins[j].startswith("s_nop")), "")
            follow[nxt.split()[0] if nxt else "(end)"] += 1
            if nxt and prv and is_dpp(nxt) and is_dpp(prv):
                c["dpp_dpp"] += 1
        elif op in ("v_readlane_b32", "v_writelane_b32", "s_waitcnt", "s_barrier"):
            c[op] += 1
    return c, follow


COLS = ("ins", "s_nop", "wait_states", "dpp_dpp", "v_readlane_b32", "v_writelane_b32", "s_waitcnt", "s_barrier")


def main():
    argv = sys.argv[1:]
    opt = lambda f, d: argv[argv.index(f) + 1] if f in argv else d
    sub, least = opt("--kernel", ""), int(opt("--min", "40"))
    path = next(a for k, a in enumerate(argv) if not a.startswith("--") and (k == 0 or argv[k - 1] not in ("--kernel", "--min")))
    K = kernels(path)
    names = demangled(list(K))
    print("%-44s %-16s %6s %6s %6s %8s %9s %10s %8s %8s" % ("kernel", "region", "ins", "s_nop", "states", "dpp-dpp", "readlane", "writelane", "waitcnt", "barrier"))
    for n in sorted(K, key=lambda x: names[x]):
        if sub not in names[n]:
            continue
        ins, lp = loops(K[n])
        regions = [("whole", 0, len(ins) - 1)] + [("loop %d-%d" % (a, b), a, b) for a, b in lp if b - a + 1 >= least]
        for tag, a, b in regions:
            c, follow = count(ins, a, b)
            print("%-44s %-16s %6d %6d %6d %8d %9d %10d %8d %8d" % ((names[n][:44], tag) + tuple(c[k] for k in COLS)))
            if "--follow" in argv and follow:
                print("    after s_nop: " + ", ".join("%s %d" % kv for kv in follow.most_common()))


if __name__ == "__main__":
    main()
