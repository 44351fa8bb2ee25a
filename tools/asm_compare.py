#!/usr/bin/env python3
"""Compare the kernels of two device assembly files (hipcc -S --cuda-device-only) instruction by instruction.

usage: asm_compare.py A.s B.s [--variant]

Comments, labels, directives, symbol names and the unit's hash symbol are ignored: what is compared is the sequence of
instructions of each kernel, every local label reference replaced by the position of its target in the kernel.
Kernels are matched by their demangled name and template arguments.  --variant: B's kernels carry one more boolean
template argument at the END of their list (a kernel that had no list has `<true>` / `<false>`); B's `..., true>` is
compared with A's kernel without it, B's `..., false>` kernels are listed as extra.  Prints one line per kernel and
exits 1 if a matched kernel differs or a kernel of A has no partner."""
import os
import re
import subprocess
import sys

CXXFILT = next((p for p in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "/opt/rocm/lib/llvm/bin/llvm-cxxfilt") if os.path.exists(p)), "c++filt")


def kernels(path):
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


def normal(body):
    pos, n = {}, 0
    for kind, s in body:
        if kind == "label":
            pos[s] = n
        else:
            n += 1
    res = []
    for kind, s in body:
        if kind == "ins":
            s = re.sub(r"\.LBB\w+", lambda m: "L%d" % pos.get(m.group(0), -1), s)
            res.append(re.sub(r"\b_Z\w+|__hip_cuid_\w+", "SYM", s))
    return res


def demangled(names):
    if not names:
        return {}
    r = subprocess.run([CXXFILT] + list(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def key(dem, variant):
    """-> (kernel name, tuple of template arguments without the variant, is this the general variant?)"""
    m = re.match(r"^(?:void )?(?:\(anonymous namespace\)::)?(\w+)(?:<([^>]*)>)?\(", dem)
    name, args = m.group(1), [a.strip() for a in (m.group(2) or "").split(",") if a.strip()]
    general = True
    if variant and args and args[-1] in ("true", "false"):
        general = args[-1] == "true"
        args = args[:-1]
    return (name, tuple(args)), general


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    variant = "--variant" in sys.argv
    A, B = kernels(args[0]), kernels(args[1])
    dA, dB = demangled(list(A)), demangled(list(B))
    Bk, extra = {}, []
    for n in B:
        k, general = key(dB[n], variant)
        if general:
            Bk[k] = n
        else:
            extra.append(n)
    bad = 0
    for n in sorted(A, key=lambda x: dA[x]):
        k, _ = key(dA[n], False)
        short = dA[n].split("(")[0] if not dA[n].startswith("void (") and not dA[n].startswith("(") else "%s<%s>" % (k[0], ", ".join(k[1]))
        if k not in Bk:
            print("MISSING in B: %s" % short)
            bad += 1
            continue
        na, nb = normal(A[n]), normal(B[Bk[k]])
        same = na == nb
        print("%s %6d %6d  %s" % ("same  " if same else "DIFFER", len(na), len(nb), short))
        bad += 0 if same else 1
    for n in sorted(extra, key=lambda x: dB[x]):
        k, _ = key(dB[n], True)
        print("extra  %6s %6d  %s<%s>" % ("", len(normal(B[n])), k[0], ", ".join(k[1] + ("false",))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
