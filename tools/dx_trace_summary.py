#!/usr/bin/env python3
"""Per-launch durations of the BPTT loop's two split-K d x GEMMs out of a `rocprofv3 --kernel-trace --output-format csv` run of
bench.py: the launches of uic_gemm_glds_kernel with a 4-slice grid (12 column tiles = d x2, 8 = d x1), in start order.  A training
step launches d x2 for decode steps 16 ... 0 and d x1 for 16 ... 1, so the i-th launch of a kind belongs to decode step
16 - i % 17 (16 - i % 16): per decode step the row tiles of the grid, the kernel variant and the median / min duration in
microseconds; then the sums over decode steps 16 ... 9 and 8 ... 0.
    python tools/dx_trace_summary.py DIR [T]"""
import csv
import glob
import os
import re
import statistics
import sys

root = sys.argv[1]
T = int(sys.argv[2]) if len(sys.argv) > 2 else 17
files = glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)
assert files, "no kernel trace under %s" % root
rows = {12: [], 8: []}
names = set()
for f in files:
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"]
        if "uic_gemm_glds_kernel" not in name:
            continue
        wg = (int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_Y"]), int(r["Workgroup_Size_Z"]))
        grid = (int(r["Grid_Size_X"]) // wg[0], int(r["Grid_Size_Y"]) // wg[1], int(r["Grid_Size_Z"]) // wg[2])
        if grid[2] != 4 or grid[1] not in rows:
            continue
        names.add(name)
        rows[grid[1]].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, grid[0],
                              re.sub(r".*uic_gemm_glds_kernel", "", name)[:40]))
for n in sorted(names):
    print("kernel:", n)
for cols, what, per in ((12, "d x2", T), (8, "d x1", T - 1)):
    v = sorted(rows[cols])
    if len(v) % per:
        print("%s: %d launches, not a multiple of %d -- no per-step table" % (what, len(v), per))
        continue
    late = early = 0.0
    for i in range(per):
        t = T - 1 - i
        d = [x[1] for x in v[i::per]]
        med = statistics.median(d)
        late, early = (late + med, early) if t >= 9 else (late, early + med)
        print("%s decode step %2d: %d row tiles, %-28s launches %3d  median %6.2f us  min %6.2f us" %
              (what, t, v[i][2], v[i][3], len(d), med, min(d)))
    print("%s: sum of the medians, decode steps 16 ... 9: %.1f us; 8 ... %d: %.1f us" % (what, late, T - per, early))
