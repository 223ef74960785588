#!/usr/bin/env python
"""Median kernel duration per shape and run from a rocprofv3 --kernel-trace of tools/attn_probe.py:

    python tools/attn_trace_medians.py TRACE_DIR REPS NAME...     (NAME...: the runs in the order of the probe's --libs, e.g. parent head parent head)

The trace holds, shape by shape, one group of REPS launches per run; the first four launches of a group are dropped.  With at least two runs
named "parent" each later column is held to the rule of profiles/attn_blocks_refactor.txt section 4: inside the span of the first two parent medians widened by that span on
each side."""
import csv, glob, re, sys
d, reps, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
PAT = re.compile(r"(attn3_kernel|attn_gqa_kernel|attn_rot_kernel)<(\d+)>")
rows = sorted((r for r in csv.DictReader(open(f)) if PAT.search(r["Kernel_Name"])), key=lambda r: int(r["Start_Timestamp"]))
assert len(rows) % (reps * len(names)) == 0, (len(rows), reps, names)
print("  %-26s " % "shape: kernel, grid" + " ".join("%8s" % f"{i + 1}:{n}" for i, n in enumerate(names)) + "   bound [us]        verdict of every run but the two parent runs")
for s in range(len(rows) // (reps * len(names))):
    med = []
    for r in range(len(names)):
        grp = rows[(s * len(names) + r) * reps:(s * len(names) + r + 1) * reps]
        assert len({PAT.search(x["Kernel_Name"]).group(0) for x in grp}) == 1
        t = sorted((int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3 for x in grp[4:])
        med.append(t[len(t) // 2])
    tag = f"{s}: {PAT.search(grp[0]['Kernel_Name']).group(0).replace('_kernel', '').replace('attn_', '')} {int(grp[0]['Grid_Size_X']) // int(grp[0]['Workgroup_Size_X'])} x {grp[0]['Workgroup_Size_X']}"
    line = "  %-26s " % tag + " ".join("%8.2f" % m for m in med)
    pi = [i for i, n in enumerate(names) if n == "parent"][:2]
    if len(pi) == 2:
        span = abs(med[pi[0]] - med[pi[1]]); lo, hi = min(med[pi[0]], med[pi[1]]) - span, max(med[pi[0]], med[pi[1]]) + span
        line += f"   [{lo:.2f}, {hi:.2f}]   " + ", ".join(f"{names[i]} {'inside' if lo - 1e-9 <= m <= hi + 1e-9 else 'OUTSIDE'}" for i, m in enumerate(med) if i not in pi)
    print(line)
