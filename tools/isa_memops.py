#!/usr/bin/env python3
"""Which memory path does each kernel's traffic take?

Reads gfx950 assembly listings (hipcc --save-temps, `make check-address-spaces`) and prints, per
kernel and per out-of-line device function, the counts of

  flat / global / LDS (ds_*) / scratch loads, stores and atomics, scalar loads,
  the kinds of s_waitcnt (both counters drained, vmcnt(0) only, lgkmcnt(0) only, counted: N > 0),
  v_readlane / v_writelane (SGPR spill traffic),

and the instruction total.  It counts these instruction classes and nothing else.

With --loops it prints instead, per kernel and function, the loops that contain no inner loop
(found from the listing's backward branches: a label and the last branch back to it), each with its
instruction count, FP64 and other VALU instructions, v_readlane / v_writelane, scalar loads, scratch
loads and stores, global and LDS accesses: where a kernel short of VALU issue slots spends them, and
which of them move spilled SGPRs (launch constants by stage).  All counts are static.

A flat access needs a 64-bit VGPR address, counts on both wait counters and may return out of
order; an access whose address space the source states is a ds_*, global_* or s_load instruction
(address spaces).  With --check, the exit status is 1 if a flat memory instruction
remains in a depth <= 1 kernel of rrt_sample.hip or in a function such a kernel calls, unless
ALLOW lists the function with its reason (DESIGN.md §4 repeats the reasons)."""
import argparse
import re
import sys

# function (demangled-name substring) -> why its flat accesses stay
ALLOW = {
}

CLASSES = [
    ("flat_ld", r"flat_load_"), ("flat_st", r"flat_store_"), ("flat_at", r"flat_atomic_"),
    ("glob_ld", r"global_load_"), ("glob_st", r"global_store_"), ("glob_at", r"global_atomic_"),
    ("lds_rd", r"ds_read"), ("lds_wr", r"ds_write"), ("lds_oth", r"ds_"),
    ("scr_ld", r"scratch_load_"), ("scr_st", r"scratch_store_"),
    ("s_ld", r"s_(?:buffer_)?load_"),
    ("rdlane", r"v_readlane_b32"), ("wrlane", r"v_writelane_b32"),
]
WAITS = ["w_both", "w_vm", "w_lgkm", "w_cnt"]
COLS = [c for c, _ in CLASSES] + WAITS + ["insts"]


def wait_kind(ops):
    vm = re.search(r"vmcnt\((\d+)\)", ops)
    lg = re.search(r"lgkmcnt\((\d+)\)", ops)
    if not vm and not lg:  # a raw immediate or expcnt only
        return "w_cnt"
    if (vm and int(vm.group(1)) > 0) or (lg and int(lg.group(1)) > 0):
        return "w_cnt"
    return "w_both" if vm and lg else "w_vm" if vm else "w_lgkm"


def functions(path):
    """name -> (counts, callees, is a kernel)"""
    out, kernels = {}, set()
    name, cnt, calls = None, None, None
    for line in open(path):
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kernels.add(m.group(1))
            continue
        m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s*(?:;.*)?$", line)
        if m and not line.startswith(".L"):
            name, cnt, calls = m.group(1), dict.fromkeys(COLS, 0), set()
            out[name] = (cnt, calls)
            continue
        m = re.match(r"^\.Lfunc_end\d+:", line)
        if m:
            name = None
            continue
        if name is None or not line.startswith("\t"):
            continue
        ins = line.strip()
        if not ins or ins[0] in ";.":
            continue
        op, _, ops = ins.partition(" ")
        cnt["insts"] += 1
        for c, pat in CLASSES:
            if re.match(pat, op):
                cnt[c] += 1
                break
        if op == "s_waitcnt":
            cnt[wait_kind(ops)] += 1
        for m in re.finditer(r"(_Z\w+)@(?:rel32|gotpcrel32)@lo", ops):
            calls.add(m.group(1))
    return {n: (c, cl, n in kernels) for n, (c, cl) in out.items()}


LOOP_COLS = ["insts", "fp64", "valu", "rdlane", "wrlane", "s_ld", "scr_ld", "scr_st", "glob", "lds"]


def loop_class(op):
    """the --loops column of one instruction, or None (it still counts in insts)"""
    if re.match(r"v_readlane_b32", op):
        return "rdlane"
    if re.match(r"v_writelane_b32", op):
        return "wrlane"
    if op.startswith("v_"):
        return "fp64" if re.search(r"_f64(?:_|$)", op) else "valu"
    if re.match(r"s_(?:buffer_)?load_", op):
        return "s_ld"
    if op.startswith("scratch_load_"):
        return "scr_ld"
    if op.startswith("scratch_store_"):
        return "scr_st"
    if re.match(r"global_(?:load|store|atomic)_", op):
        return "glob"
    if op.startswith("ds_"):
        return "lds"
    return None


def innermost_loops(path):
    """name -> [(header label, first line, last line, counts)] of the loops without an inner loop.

    A loop is a label and the last branch back to it from further down the same function (the
    listing's backward branches); it is innermost if no other loop lies within its span."""
    out = {}
    name, ins, labels = None, [], {}

    def close():
        if name is None:
            return
        span = {}  # header index -> last back-branch index
        for i, (_ln, op, ops) in enumerate(ins):
            if not re.match(r"s_c?branch", op):
                continue
            tgt = ops.split(",")[-1].strip()
            if tgt in labels and labels[tgt] <= i:
                h = labels[tgt]
                span[h] = max(span.get(h, i), i)
        res = []
        for h, e in sorted(span.items()):
            if any((h2, e2) != (h, e) and h <= h2 and e2 <= e for h2, e2 in span.items()):
                continue
            cnt = dict.fromkeys(LOOP_COLS, 0)
            for _ln, op, _ops in ins[h : e + 1]:
                cnt["insts"] += 1
                c = loop_class(op)
                if c:
                    cnt[c] += 1
            label = next(l for l, k in labels.items() if k == h)
            res.append((label, ins[h][0], ins[e][0], cnt))
        out[name] = res

    for ln, line in enumerate(open(path), 1):
        m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s*(?:;.*)?$", line)
        if m and not line.startswith(".L"):
            close()
            name, ins, labels = m.group(1), [], {}
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            close()
            name = None
            continue
        if name is None:
            continue
        m = re.match(r"^(\.L\w+):", line)
        if m:
            labels.setdefault(m.group(1), len(ins))  # the next instruction's index
            continue
        if not line.startswith("\t"):
            continue
        s = line.strip()
        if not s or s[0] in ";.":
            continue
        op, _, ops = s.partition(" ")
        ins.append((ln, op, ops.split(";")[0]))
    close()
    return out


def print_loops(paths, only):
    for path in paths:
        kernels = {n for n, (_c, _cl, k) in functions(path).items() if k}
        print(f"# {path.split('/')[-1]}: loops without an inner loop (label, listing lines)")
        for n, loops in innermost_loops(path).items():
            tag = ("K " if n in kernels else "f ") + short(n)
            if not loops or (only and only not in tag):
                continue
            print(tag)
            print(f"  {'loop':12s} {'lines':>15s} " + " ".join(f"{c:>6s}" for c in LOOP_COLS))
            tot = dict.fromkeys(LOOP_COLS, 0)
            for label, a, b, cnt in loops:
                print(f"  {label:12s} {f'{a}-{b}':>15s} " + " ".join(f"{cnt[c]:6d}" for c in LOOP_COLS))
                for c in LOOP_COLS:
                    tot[c] += cnt[c]
            print(f"  {'total':12s} {len(loops):>9d} loops " + " ".join(f"{tot[c]:6d}" for c in LOOP_COLS))


def short(name):
    """the mangled name's readable core: function name + its template arguments' literals"""
    core = name
    m = re.match(r"_Z(?:N3rrt)?(\d+)(\w+)", name)
    if m:
        core = m.group(2)[: int(m.group(1))]
    args = re.findall(r"L([bij])(n?\d+)E", name)
    lit = ", ".join(("-" + v[1:] if v.startswith("n") else v) for _t, v in args)
    return f"{core}<{lit}>" if lit else core


def depth1_kernel(path, name):
    """a depth <= 1 kernel of rrt_sample.hip: all of its kernels but rrt_sample_kernel<.., DEEP = true>"""
    if "rrt_sample" not in path:
        return False
    return not re.search(r"rrt_sample_kernelILb[01]ELi\d+ELi\d+ELb1E", name)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listings", nargs="+")
    ap.add_argument("--check", action="store_true", help="fail on a flat memory instruction in the depth <= 1 kernels")
    ap.add_argument("--loops", action="store_true",
                    help="per kernel and function, the loops without an inner loop: instructions, FP64, other VALU, "
                         "lane moves, scalar / scratch / global / LDS accesses")
    ap.add_argument("--only", default="", help="with --loops: only functions whose printed name contains this")
    a = ap.parse_args()
    if a.loops:
        print_loops(a.listings, a.only)
        return
    bad = []
    for path in a.listings:
        fns = functions(path)
        print(f"# {path.split('/')[-1]}")
        print(f"{'function':44s} " + " ".join(f"{c:>7s}" for c in COLS))
        reach = set()
        todo = [n for n, (_c, _cl, k) in fns.items() if k and depth1_kernel(path, n)]
        while todo:
            n = todo.pop()
            if n in reach or n not in fns:
                continue
            reach.add(n)
            todo += list(fns[n][1])
        for n, (c, _cl, k) in fns.items():
            if c["insts"] == 0:
                continue
            tag = ("K " if k else "f ") + short(n)
            print(f"{tag[:44]:44s} " + " ".join(f"{c[x]:7d}" for x in COLS))
            flat = c["flat_ld"] + c["flat_st"] + c["flat_at"]
            if a.check and n in reach and flat and not any(s in short(n) for s in ALLOW):
                bad.append((path.split("/")[-1], short(n), flat))
    for s, why in ALLOW.items():
        print(f"# allowed: {s}: {why}")
    for p, n, flat in bad:
        print(f"FLAT: {p}: {n}: {flat} flat memory instructions", file=sys.stderr)
    if a.check:
        print("address spaces: " + ("FAILED" if bad else "no flat memory instruction in the depth <= 1 kernels"))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
