"""What the compiler reports of a unit's kernels -- registers, scratch, LDS, occupancy -- for the *_resources tests and
tools/resource_usage.py: the unit is cross-compiled (no GPU) with -Rpass-analysis=kernel-resource-usage and the remarks
are read; nothing is run.  Plain helpers: nothing here is collected."""
import os
import re
import subprocess

from videomorphing_amd import build

REMARKS = "-Rpass-analysis=kernel-resource-usage"


def parse_remarks(stderr):
    """{mangled kernel name: {"VGPRs": n, "ScratchSize [bytes/lane]": n, ...}} of the compiler's resource remarks"""
    out, name = {}, None
    for line in stderr.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s+([A-Za-z][^:]*): (\d+))", line)
        if not m:
            continue
        if m.group(1):
            name = m.group(1)
            out[name] = {}
        elif name:
            out[name][m.group(2).strip()] = int(m.group(3))
    return out


def unit_usage(unit_name, tmp_dir):
    """parse_remarks of every kernel of videomorphing_amd/csrc/<unit_name>, compiled with the build's own flags"""
    extra = [e for s, _, e in build.UNITS if s == unit_name][0]
    assert "-ffp-contract=off" in extra
    obj = os.path.join(str(tmp_dir), os.path.splitext(unit_name)[0] + ".o")
    r = subprocess.run([build._hipcc()] + build.COMMON + extra + [REMARKS, "-c", os.path.join(build.CSRC, unit_name), "-o", obj],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return parse_remarks(r.stderr)
