#!/usr/bin/env python3
"""Compare two builds' gfx950 listings (make's ISA_LISTINGS) function by function.

Per kernel and out-of-line device function: whether the instruction text is the same in both
listings -- labels and instructions, with comments, directives and the metadata block left out --
and, where it is not, both instruction counts and the size of the diff (lines removed / added).
With --resources (two logs of `make resource-usage`), a function that differs also gets both sides'
register, spill, scratch, LDS and occupancy figures.  It diffs text and looks for nothing in it.

Usage: isa_diff.py OLD_DIR NEW_DIR [--resources OLD_REMARKS NEW_REMARKS]
(the directories hold the *.s listings; files are paired by name)"""
import argparse
import difflib
import glob
import os
import re
import subprocess

FIELDS = ["VGPRs", "AGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "LDS Size", "Occupancy"]


def functions(path):
    """name -> the function's lines (labels and instructions)"""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s*(?:;.*)?$", line)
        if m:  # (__hip_cuid_*: the unit's hash, a data symbol)
            cur = None if m.group(1).startswith("__hip_cuid_") else out.setdefault(m.group(1), [])
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
            continue
        if cur is None:
            continue
        text = line.split(";", 1)[0].strip()
        if not text or (text.startswith(".") and not text.endswith(":")):  # comment or directive
            continue
        cur.append(text)
    return out


def resources(path):
    rows, cur = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return rows


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(name):
    """template arguments kept, the parameter list dropped"""
    return re.sub(r"\((?:[^()]|\([^()]*\))*\)(?: \[clone [^\]]*\])?$", "", name.replace("void ", "", 1))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--resources", nargs=2, metavar=("OLD_REMARKS", "NEW_REMARKS"))
    a = ap.parse_args()
    res = [resources(p) for p in a.resources] if a.resources else None
    n_same = n_diff = 0
    for old in sorted(glob.glob(os.path.join(a.old, "*.s"))):
        unit = os.path.basename(old)
        new = os.path.join(a.new, unit)
        if not os.path.exists(new):
            print(f"{unit}: only in {a.old}")
            continue
        fo, fn = functions(old), functions(new)
        names = demangle(sorted(set(fo) | set(fn)))
        print(f"== {unit.split('-hip-')[0]}: {len(fo)} functions, {len(fn)} in the change")
        for m in sorted(names, key=lambda k: names[k]):
            label = short(names[m])
            if m not in fo or m not in fn:
                print(f"  only in {'the parent' if m in fo else 'the change'}  {label}")
                n_diff += 1
                continue
            if fo[m] == fn[m]:
                print(f"  identical  {label}")
                n_same += 1
                continue
            n_diff += 1
            d = [x for x in difflib.unified_diff(fo[m], fn[m], lineterm="", n=0) if x[:1] in "+-" and x[:3] not in ("+++", "---")]
            minus, plus = sum(x[0] == "-" for x in d), sum(x[0] == "+" for x in d)
            print(f"  DIFFERS    {label}: {len(fo[m])} -> {len(fn[m])} lines, diff -{minus} +{plus}")
            if res:
                for side, r in zip(("parent", "change"), res):
                    row = r.get(m)
                    if row:
                        print(f"      {side}: " + "  ".join(f"{k} {row.get(k, '?')}" for k in FIELDS))
    print(f"{n_same} functions identical, {n_diff} differ")


if __name__ == "__main__":
    main()
