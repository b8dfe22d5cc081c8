#!/usr/bin/env python3
"""Instruction budget of a kernel by SECTION, from a hipcc -S device listing (development tool):
   tools/loop_budget.py listing.s <mangled kernel name substring> [<substring of the kernels whose resources to list>]
Sections: the prologue (entry to the first block of a loop), every loop (its own instructions, child loops excluded; depth and the
label of the listing; blocks are assigned by the loop their label's comment names), the blocks between the loops that belong to none,
and the epilogue (after the last block of a loop).  Per section: VALU instructions
that are not transcendental, transcendentals (v_exp / v_log / v_rcp / v_rsq / v_sqrt / v_sin / v_cos), v_permlane, LDS (ds_*), vector
memory (buffer_ / global_ / scratch_ / flat_), scalar (s_* other than waits and branches), waits (s_waitcnt, s_nop) and branches.
With a third argument: VGPRs, SGPRs, LDS and scratch bytes of every kernel whose name contains it (tools/isa_stats.py's figures)."""
import re
import sys

s = open(sys.argv[1]).read()
pat = sys.argv[2]
TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")
CLASSES = ("valu", "trans", "permlane", "lds", "vmem", "scalar", "wait", "branch")


def classify(op):
    if op.startswith("v_permlane"):
        return "permlane"
    if op.startswith(TRANS):
        return "trans"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "scratch_", "flat_")):
        return "vmem"
    if op in ("s_waitcnt", "s_nop"):
        return "wait"
    if op.startswith(("s_cbranch", "s_branch", "s_endpgm")):
        return "branch"
    return "scalar" if op.startswith("s_") else None


for chunk in s.split(".end_amdhsa_kernel"):
    heads = [l.split(":")[0] for l in chunk.split("\n") if l.startswith("_ZN") and ":" in l and pat in l.split(":")[0]]
    if not heads:
        continue
    name = heads[-1]
    body = chunk[chunk.index("\n" + name + ":"):].split("\n")
    end = next((n for n, l in enumerate(body) if l.strip().startswith("s_endpgm")), len(body) - 1)
    # every basic block names the loop it belongs to in its label's comment ("in Loop: Header=BB5_12 Depth=1", or "Loop Header: Depth=N"
    # for a header itself, possibly on the comment line after "Parent Loop ..."); blocks that name none lie outside every loop
    owner, depth, order, cur = {}, {}, [], None
    for n, l in enumerate(body[:end + 1]):
        m = re.match(r"(?:\.L|; %bb\.)(BB\d+_\d+|\d+):", l)
        if m:
            text = l + " " + (body[n + 1] if body[n + 1].lstrip().startswith(";") and "%bb." not in body[n + 1] else "")
            h = re.search(r"Loop Header: Depth=(\d+)", text)
            i = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", text)
            cur = m.group(1) if h else (i.group(1) if i else None)
            if h:
                depth[cur] = int(h.group(1))
                order.append(cur)
        owner[n] = cur
    in_loop = [n for n in range(end + 1) if owner[n]]
    first, last = (in_loop[0], in_loop[-1]) if in_loop else (end + 1, end + 1)

    def count(lines):
        c = dict.fromkeys(CLASSES, 0)
        for n in lines:
            t = body[n].strip().split()
            if t and not t[0].startswith((".", ";")):
                k = classify(t[0])
                if k:
                    c[k] += 1
        return c

    def show(tag, c):
        print(f"  {tag:34s}" + "".join(f" {k} {c[k]:4d}" for k in CLASSES))

    print(name)
    show("prologue (to the first loop)", count(range(0, first)))
    for lab in order:
        show(f"loop .L{lab} depth {depth[lab]} (own)", count(n for n in range(end + 1) if owner[n] == lab))
    show("between the loops", count(n for n in range(first, last + 1) if not owner[n]))
    show("epilogue (after the last loop)", count(range(last + 1, end + 1)))

if len(sys.argv) > 3:
    for m in re.finditer(r"^(_ZN3sgr\w+):.*?\.end_amdhsa_kernel", s, re.S | re.M):
        if sys.argv[3] in m.group(1):
            f = lambda k: re.search(k + r"\s+(\d+)", m.group(0)).group(1)
            print(m.group(1), "vgpr", f(r"\.amdhsa_next_free_vgpr"), "sgpr", f(r"\.amdhsa_next_free_sgpr"), "lds",
                  f(r"\.amdhsa_group_segment_fixed_size"), "scratch", f(r"\.amdhsa_private_segment_fixed_size"))
