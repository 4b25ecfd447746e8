#!/usr/bin/env python3
"""Compare the kernels of two -save-temps assemblies (qr_device-hip-amdgcn-amd-amdhsa-gfx950.s) body for body.

Every kernel of the OLD file is looked up in the NEW one by its symbol name; its instructions and its .amdhsa_kernel
descriptor block (registers, scratch, LDS), from the symbol's label to its .Lfunc_end label, are compared after local labels --
.LBB<f>_<n>, .Ltmp<n>, .Lfunc_end<n> and the numbered labels of inline assembly (qr_cull_*_<n>) -- are renumbered in order
of first appearance, since they follow the position of the kernel in the file.  Kernels only the NEW file has are listed.
A change to the device code that must leave the existing kernels as they were (a new instance, a new kernel) shows an
empty diff.  A kernel that DIFFERS also says whether its .amdhsa_ descriptor lines are identical and how many instruction lines
it has in OLD and in NEW: what a refactor that moves code between functions is judged by.

usage: kernel_asm_diff.py OLD.s NEW.s [--show N]      exit status 1 when some kernel of OLD differs or is missing
"""
import difflib
import re
import sys

LABEL = re.compile(r"\.LBB\d+_\d+|\.Ltmp\d+|\.Lfunc_end\d+|\bqr_cull_[a-z]+_\d+")


def _norm(lines):
    names = {}
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()          # comments: "; %bb.12", "; @name"
        if not ln:
            continue
        out.append(LABEL.sub(lambda m: names.setdefault(m.group(0), f"L{len(names)}"), ln))
    return out


def kernels(path):
    """{symbol: normalised text} of every kernel in the file: its instructions and its .amdhsa_kernel block, which the
    assembler places between the kernel's label and its .Lfunc_end label"""
    text = open(path, errors="replace").read().split("\n")
    out = {}
    i = 0
    while i < len(text):
        m = re.match(r"^(_Z\w+):", text[i])
        if not m:
            i += 1
            continue
        j = i + 1
        while j < len(text) and not re.match(r"^\.Lfunc_end\d+:", text[j]):
            j += 1
        if any(".amdhsa_kernel" in ln for ln in text[i:j]):
            out[m.group(1)] = _norm(text[i + 1:j])
        i = j
    return out


def _descriptor(body):
    """the .amdhsa_ lines of a kernel: registers, spills' private segment, LDS, what the launch sets up"""
    return [ln.strip() for ln in body if ln.strip().startswith(".amdhsa_")]


def _instructions(body):
    """number of instruction lines: neither labels nor assembler directives"""
    return sum(1 for ln in body if not ln.strip().startswith(".") and not ln.rstrip().endswith(":"))


def main():
    if len(sys.argv) < 3:
        print(__doc__, file=sys.stderr)
        return 2
    show = int(sys.argv[sys.argv.index("--show") + 1]) if "--show" in sys.argv else 20
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(old):
        if name not in new:
            print(f"MISSING  {name}")
            bad += 1
            continue
        if old[name] == new[name]:
            print(f"same     {name}  ({len(old[name])} lines)")
            continue
        bad += 1
        desc = "identical" if _descriptor(old[name]) == _descriptor(new[name]) else "DIFFERENT"
        print(f"DIFFERS  {name}  (descriptor {desc}; instructions {_instructions(old[name])} -> {_instructions(new[name])})")
        d = list(difflib.unified_diff(old[name], new[name], "old", "new", lineterm="", n=1))
        print("\n".join(d[:show]))
    for name in sorted(set(new) - set(old)):
        print(f"new      {name}  ({len(new[name])} lines)")
    print(f"{len(old) - bad} of {len(old)} kernels unchanged")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
