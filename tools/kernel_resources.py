#!/usr/bin/env python3
"""Registers / LDS / scratch of every kernel, from the metadata notes of the built gfx950 code objects
(dot_ring_amd/csrc/build/*.gfx950, extracted by tools/count_kernel_insts.py).  `python3 tools/kernel_resources.py [substring]`."""
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "dot_ring_amd", "csrc", "build")
FIELDS = {"vgpr": "vgpr_count", "agpr": "agpr_count", "sgpr": "sgpr_count", "lds": "group_segment_fixed_size",
          "scratch": "private_segment_fixed_size", "spill_v": "vgpr_spill_count"}


def resources(build=BUILD):
    """{mangled kernel symbol: {vgpr, agpr, sgpr, lds, scratch, spill_v}} of the code objects under `build`"""
    out = {}
    for co in sorted(glob.glob(os.path.join(build, "*gfx950"))):
        txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
        for blk in txt.split("  - .agpr_count:")[1:]:
            blk = ".agpr_count: " + blk
            g = lambda k: (re.search(r"\." + k + r":\s*(\S+)", blk) or [None, "?"])[1]
            out[g("name")] = {short: g(key) for short, key in FIELDS.items()}
    return out


if __name__ == "__main__":
    want = sys.argv[1] if len(sys.argv) > 1 else ""
    for sym, r in resources().items():
        name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip().split("(")[0]
        if want in name:
            print(f"{name[:64]:64s} vgpr={r['vgpr']:>4s} agpr={r['agpr']:>3s} sgpr={r['sgpr']:>4s} "
                  f"lds={r['lds']:>7s} scratch={r['scratch']:>5s} spill_v={r['spill_v']:>3s}")
