#!/usr/bin/env python3
"""Instruction census of the wave-stage loops of a kernel, from a device-only `hipcc -S` listing.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -S pg_kinship.hip -o kin.s
    tools/kin_census.py kin.s 'k_kinship_syrkILb1ELb1ELi3E'        # substring of the mangled kernel name

A "wave-stage loop" is a loop of the kernel (a backward branch to a label) whose body holds matrix instructions and no
other such loop: the 13-tile kinship kernels have one per wave variant of their `switch (wave)`.  A loop
that was unrolled over several stages holds one workgroup barrier per stage, so the counts are divided by the number of
`s_barrier` in the body.  Instructions are classified by opcode prefix ONLY:

    mfma  v_mfma*            valu  every other v_*           ds_read / ds_write  ds_read* (ds_load*) / every other ds_*
    vmem  buffer_* global_* flat_* scratch_*                 salu  every s_* that is no branch, wait or barrier
    branch  s_cbranch* s_branch                               (waits, barriers and s_nop are listed as "sync")

Registers and spills come from the code object's metadata at the end of the listing (amdhsa.kernels).  No GPU is needed.
With --json the per-loop rows are printed as one JSON document instead of the table.  With --f64-blocks the f64 VALU count of
every basic block of a trip is listed per loop: the fused sums' one-trait and two-trait chains are alternatives behind a branch, and
the table's f64 column adds them up.
"""
import argparse
import json
import re
import sys

CLASSES = ("total", "mfma", "valu", "ds_read", "ds_write", "vmem", "salu", "branch", "sync")
DETAIL = ("v_add_u32", "v_cndmask", "v_mov_b32", "dpp", "f64")


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "ds_read"
    if op.startswith("ds_"):
        return "ds_write"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith(("s_waitcnt", "s_barrier", "s_nop", "s_sleep")):
        return "sync"
    if op.startswith("s_"):
        return "salu"
    return None


def kernel_bodies(lines):
    """(name, first line, last line) of every function of the listing"""
    starts = [(i, m.group(1)) for i, l in enumerate(lines) if (m := re.match(r"\s*\.type\s+(\S+),@function", l))]
    out = []
    for k, (i, name) in enumerate(starts):
        end = next((j for j in range(i, len(lines)) if re.match(r"\s*\.size\s+" + re.escape(name) + r"\b", lines[j])), len(lines))
        out.append((name, i, end))
    return out


def instructions(lines, lo, hi):
    """(line number, opcode, text) of the instructions and (label -> line number) of lines lo..hi"""
    ins, labels = [], {}
    for i in range(lo, hi):
        l = lines[i].split(";")[0].strip()
        if not l:
            continue
        m = re.match(r"([.\w$]+):$", l)
        if m:
            labels[m.group(1)] = i
            continue
        if l[0] == ".":
            continue
        ins.append((i, l.split()[0], l))
    return ins, labels


def stage_loops(ins, labels):
    """line ranges (head, back branch) of the innermost loops that hold matrix instructions"""
    ranges = []
    for i, op, text in ins:
        if op.startswith(("s_cbranch", "s_branch")):
            tgt = labels.get(text.split()[-1])
            if tgt is not None and tgt < i:
                ranges.append((tgt, i))
    mf = [i for i, op, _ in ins if op.startswith("v_mfma")]
    ranges = [r for r in ranges if any(r[0] < i < r[1] for i in mf)]
    # innermost: a backward jump to a shared exit block that the compiler placed earlier spans whole loops and is none itself
    return sorted(r for r in set(ranges) if not any(o != r and r[0] <= o[0] and o[1] <= r[1] for o in ranges))


def census(ins, lo, hi):
    c = {k: 0 for k in CLASSES + DETAIL}
    barriers = 0
    for i, op, text in ins:
        if not lo < i <= hi:
            continue
        k = classify(op)
        if k is None:
            continue
        c["total"] += 1
        c[k] += 1
        barriers += op == "s_barrier"
        if k == "valu":
            for d in ("v_add_u32", "v_cndmask", "v_mov_b32"):
                c[d] += op.startswith(d)
            c["dpp"] += "_dpp" in op or " row_" in text or "quad_perm" in text
            c["f64"] += op.endswith("_f64") or "_f64_" in op
    stages = max(barriers, 1)
    return {k: v / stages for k, v in c.items()}, stages


def f64_blocks(ins, labels, lo, hi):
    """f64 VALU count of every basic block of lines lo..hi that has any, in listing order (a block ends at a label or behind a
    branch).  Whole trip, not per stage: the fused sums' one-trait and two-trait code are different blocks of one loop."""
    starts = {i for i in labels.values() if lo < i <= hi}
    out, n, prev = [], 0, lo
    for i, op, text in ins:
        if not lo < i <= hi:
            continue
        if any(prev < s <= i for s in starts):
            out.append(n); n = 0
        prev = i
        n += classify(op) == "valu" and (op.endswith("_f64") or "_f64_" in op)
        if op.startswith(("s_cbranch", "s_branch")):
            out.append(n); n = 0
    out.append(n)
    return [b for b in out if b]


def metadata(lines, name):
    """register and spill counts of kernel `name` from the amdhsa.kernels document"""
    out, inside = {}, False
    keys = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
            ".group_segment_fixed_size")
    block = {}
    for l in lines:
        s = l.strip()
        if s.startswith("- .") or s == "...":      # a new kernel record (or the end of the document)
            if block.get(".name") == name:
                out = block
            block = {}
        m = re.match(r"-?\s*(\.[\w]+):\s*(\S+)$", s)
        if m and (m.group(1) in keys or m.group(1) == ".name"):
            block[m.group(1)] = m.group(2)
    if block.get(".name") == name:
        out = block
    return {k[1:]: int(v) for k, v in out.items() if k != ".name"}


def fmt(v):
    return f"{v:g}" if abs(v - round(v)) > 1e-9 else str(int(round(v)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("kernel", help="substring of the (mangled) kernel name; every match is reported")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--f64-blocks", action="store_true", help="also list, per loop, the f64 VALU count of each basic block that has any (per trip)")
    a = ap.parse_args()
    lines = open(a.listing).read().split("\n")
    doc = []
    for name, lo, hi in kernel_bodies(lines):
        if a.kernel not in name:
            continue
        ins, labels = instructions(lines, lo, hi)
        rows = []
        for head, back in stage_loops(ins, labels):
            c, stages = census(ins, head, back)
            c["stages_per_iteration"] = stages
            if a.f64_blocks:
                c["f64_blocks"] = f64_blocks(ins, labels, head, back)
            rows.append(c)
        doc.append({"kernel": name, "metadata": metadata(lines, name), "loops": rows})
    if not doc:
        sys.exit(f"no kernel matching {a.kernel!r} in {a.listing}")
    if a.json:
        print(json.dumps(doc, indent=1))
        return
    for k in doc:
        md = k["metadata"]
        print(f"{k['kernel']}")
        print("  " + "  ".join(f"{key}={md[key]}" for key in sorted(md)))
        cols = CLASSES + DETAIL
        print("  loop  st/it " + " ".join(f"{c:>9}" for c in cols))
        for n, r in enumerate(k["loops"]):
            print(f"  {n:4d}  {r['stages_per_iteration']:5d} " + " ".join(f"{fmt(r[c]):>9}" for c in cols))
        if k["loops"]:
            print("  range       " + " ".join(f"{fmt(min(r[c] for r in k['loops'])) + '-' + fmt(max(r[c] for r in k['loops'])):>9}" for c in cols))
        if a.f64_blocks:
            for n, r in enumerate(k["loops"]):
                print(f"  loop {n:2d}: f64 VALU per basic block of a trip: " + " ".join(str(b) for b in r["f64_blocks"]))
        print("  (per wave and stage; valu excludes mfma; the last five columns are subsets of valu)")


if __name__ == "__main__":
    main()
