#!/usr/bin/env python
"""Compares the gfx950 code of two builds of one unit, kernel by kernel:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -S --cuda-device-only old/unit.hip -o old.s
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -S --cuda-device-only new/unit.hip -o new.s
    python tools/asm_compare.py old.s new.s [--diff KERNEL]

Per kernel: VGPRs, SGPRs, LDS bytes, private segment (scratch), spill counts and instruction count
of both, and whether the instruction streams are equal once register names (and the labels' numbers)
are masked.  --diff prints the masked unified diff of one kernel (a substring of its name).  The
table of DESIGN section 20 is this tool's output.  No device is needed."""
import argparse
import difflib
import json
import re
import sys

META = {"vgprs": r"; NumVgprs: (\d+)", "sgprs": r"; TotalNumSgprs: (\d+)", "lds": r"; LDSByteSize: (\d+)",
        "scratch": r"; ScratchSize: (\d+)", "sgpr_spill": r"\.sgpr_spill_count:\s+(\d+)",
        "vgpr_spill": r"\.vgpr_spill_count:\s+(\d+)"}
REG = re.compile(r"\b[vsa]\d+\b|\b[vsa]\[\d+:\d+\]|\.LBB\d+_\d+")


def kernels(path):
    text = open(path).read()
    out = {}
    # spill counts live in the metadata at the end of the file, keyed by the kernel's name
    spills = {m.group(1): m.group(0) for m in
              re.finditer(r"- \.agpr_count:.*?\.name:\s+(\S+).*?\.wavefront_size", text, re.S)}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:\n(.*?)(?=; -- Begin function|^\t\.amdgpu_metadata|\Z)",
                         text, re.S | re.M):
        name, body, tail = m.group(1), m.group(2), m.group(3)
        if ".amdhsa_kernel " + name not in text:
            continue
        ins = []
        for line in body.splitlines():
            line = line.split(";")[0].strip()
            if not line or line.startswith((".", "//")) and not line.startswith(".LBB"):
                continue
            ins.append(REG.sub("R", line))
        rec = {"instructions": sum(1 for i in ins if not i.startswith("R:") and not i.endswith(":"))}
        for k, pat in META.items():
            src = spills.get(name, "") if k.endswith("_spill") else tail
            mm = re.search(pat, src)
            rec[k] = int(mm.group(1)) if mm else None
        out[name] = (rec, ins)
    return out


def short(name):
    m = re.match(r"_ZN\d+_GLOBAL__N_1(\d+)", name)
    if m:
        k = len(m.group(0))
        return name[k:k + int(m.group(1))]
    m = re.match(r"_Z(\d+)", name)
    return name[len(m.group(0)):len(m.group(0)) + int(m.group(1))] if m else name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--diff", default=None)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    rows = []
    for name in old:
        if name not in new:
            rows.append({"kernel": short(name), "missing_in_new": True})
            continue
        (ro, io), (rn, inn) = old[name], new[name]
        rows.append({"kernel": short(name), "old": ro, "new": rn, "same_stream": io == inn})
        if a.diff and a.diff in name:
            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(io, inn, "old", "new", lineterm="", n=2))
    rows += [{"kernel": short(n), "missing_in_old": True} for n in new if n not in old]
    if a.json:
        print(json.dumps(rows, indent=1))
    elif not a.diff:
        keys = ("vgprs", "sgprs", "lds", "scratch", "sgpr_spill", "vgpr_spill", "instructions")
        print("kernel | " + " | ".join(keys) + " | same stream")
        for r in rows:
            if "old" not in r:
                print(r)
                continue
            print(r["kernel"] + " | " + " | ".join(
                str(r["old"][k]) if r["old"][k] == r["new"][k] else f"{r['old'][k]} -> {r['new'][k]}" for k in keys)
                + " | " + ("yes" if r["same_stream"] else "NO"))
    return 0 if all(r.get("same_stream") for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
