#!/usr/bin/env python3
"""Compare the kernels of two builds, instruction by instruction.

`python3 tools/kernel_diff.py PARENT_BUILD_DIR THIS_BUILD_DIR` (two dot_ring_amd/csrc/build directories holding the .o files of
`make`) disassembles the gfx950 code objects of both (extracted as tools/count_kernel_insts.py does) and, for every kernel symbol
present in both, compares opcode and operands of the whole instruction stream.  The one thing blanked is the literal of each
s_add_u32 / s_addc_u32 that follows an s_getpc_b64: the PC-relative address of a constant, which moves with the layout of the code
object; and the run of s_nop at the very end of a listing is dropped (the alignment padding behind the LAST kernel of a code object,
which belongs to another kernel once a unit gains one).  Per symbol it prints `identical` or `different`; for a different one both instruction counts, both v_mad_i64_i32 counts
(the field products executed) and VGPR / AGPR / SGPR / LDS / scratch of both sides (tools/kernel_resources.py).  Symbols on one
side only are listed.  Exit status 1 if a symbol differs or is missing.  Needs no GPU.
"""
import re
import subprocess
import sys

from count_kernel_insts import OBJDUMP, device_objects
from kernel_resources import resources

_HEAD = re.compile(r"^[0-9a-f]+ <(\S+)>:")
_INSN = re.compile(r"^\s+(\S+)\s*(.*?)\s*//")
_PCREL = re.compile(r"(0x[0-9a-f]+|-?\d+)$")


def streams(build):
    """{kernel symbol: [instruction text]} of every code object under `build`, PC-relative literals blanked"""
    objects = device_objects(build)            # (extracts the code objects that resources() reads)
    kernels = resources(build)
    out = {}
    for co in objects:
        name, after_getpc = None, 0
        for line in subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout.splitlines():
            head = _HEAD.match(line)
            if head:
                name = head.group(1) if head.group(1) in kernels else None
                if name:
                    out[name] = []
                continue
            insn = _INSN.match(line)
            if not name or not insn:
                continue
            op, args = insn.groups()
            args = re.sub(r"<\S+>", "", args).strip()             # branch targets: keep the offset, drop the symbol + offset echo
            if op == "s_getpc_b64":
                after_getpc = 2
            elif after_getpc and op in ("s_add_u32", "s_addc_u32"):
                args, after_getpc = _PCREL.sub("LIT", args), after_getpc - 1
            out[name].append(op + " " + args)
    for ins in out.values():                   # the s_nop padding behind a code object's last kernel is listed under it: not executed
        while ins and ins[-1].startswith("s_nop") and any(i.startswith("s_endpgm") for i in ins):
            ins.pop()
    return kernels, out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    (res_a, a), (res_b, b) = streams(sys.argv[1]), streams(sys.argv[2])
    different = 0
    for sym in sorted(set(a) & set(b)):
        same = a[sym] == b[sym]
        different += not same
        short = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip().split("(")[0]
        print(f"{'identical' if same else 'different':9s} {short}")
        if not same:
            for side, ins, res in (("parent", a[sym], res_a[sym]), ("this", b[sym], res_b[sym])):
                mads = sum(i.startswith("v_mad_i64_i32") for i in ins)
                print(f"    {side:6s} instructions={len(ins)} v_mad_i64_i32={mads} " + " ".join(f"{k}={v}" for k, v in res.items()))
    for side, only in (("parent", set(a) - set(b)), ("this", set(b) - set(a))):
        for sym in sorted(only):
            print(f"only in {side}: {sym}")
    both = len(set(a) & set(b))
    print(f"{both} symbols in both, {both - different} identical, {different} different, {len(set(a) ^ set(b))} on one side only")
    return 1 if different or set(a) ^ set(b) else 0


if __name__ == "__main__":
    sys.exit(main())
