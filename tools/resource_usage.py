"""dev: registers, scratch, LDS and occupancy of every kernel of one .hip unit (the compiler's kernel-resource-usage remarks),
one line per kernel -- diff two commits' tables to see whether a change moved a kernel it was not meant to move.
usage: python tools/resource_usage.py videomorphing_amd/csrc/vm_mgb.hip [-ffp-contract=fast ...] > table.txt
(tools/spill_table.py is the sweep kernels' deeper table)"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from kernel_resources import REMARKS, parse_remarks  # noqa: E402  (the parser of the *_resources tests)
from videomorphing_amd.build import _hipcc  # noqa: E402  (the compiler the library is built with)
src, flags = sys.argv[1], sys.argv[2:]
rem = subprocess.run([_hipcc(), "-O3", "-std=c++17", "--offload-arch=gfx950", "--offload-device-only", "-I" + os.path.join(ROOT, "include")] + flags +
                     [REMARKS, "-c", src, "-o", os.devnull], capture_output=True, text=True).stderr
KEYS = ("VGPRs", "AGPRs", "TotalSGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
usage = {}
for mangled, u in parse_remarks(rem).items():
    name = subprocess.check_output(["c++filt", mangled], text=True).strip().replace("(anonymous namespace)::", "").split("(")[0]
    usage[re.sub(r"^void ", "", name)] = u
print("%-44s %5s %5s %5s %7s %7s %8s %8s %5s" % ("kernel", "VGPR", "AGPR", "SGPR", "v.spill", "s.spill", "scratch", "LDS", "occ."))
for name in sorted(usage):
    print("%-44s %5s %5s %5s %7s %7s %8s %8s %5s" % ((name[:44],) + tuple(usage[name].get(k, "?") for k in KEYS)))
