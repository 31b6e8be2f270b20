"""Phase of co-resident scans in a rocprofv3 kernel trace: start-to-start offsets of consecutive launches
of the dominant kernel against its duration."""
import csv, sys
from collections import defaultdict
import numpy as np
rows = []
with open(sys.argv[1], newline="") as f:
    for r in csv.DictReader(f):
        rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
tot = defaultdict(int)
for n, s, e in rows:
    tot[n] += e - s
dom = max(tot, key=tot.get)
sel = sorted((s, e) for n, s, e in rows if n == dom)[-1000:]
s = np.array([x[0] for x in sel], float) / 1e3
e = np.array([x[1] for x in sel], float) / 1e3
dur = e - s
d1 = np.diff(s)
res_at_start = np.array([int(((s[:i] <= s[i]) & (e[:i] > s[i])).sum()) for i in range(len(s))])
pc = lambda v: "p10 %.1f p50 %.1f p90 %.1f" % tuple(np.percentile(v, [10, 50, 90]))
print("kernel:", dom[:100])
print("duration us:", pc(dur))
print("start-to-start us:", pc(d1), " mean %.2f" % d1.mean())
print("start-to-start / duration (0 or 1 = in phase, 0.5 = opposite):", pc(d1 / dur[1:]))
print("gap from previous launch's end to this start us (negative = overlap):", pc(s[1:] - e[:-1]))
print("other launches of it resident at a launch's start:", {int(a): int(b) for a, b in zip(*np.unique(res_at_start[10:], return_counts=True))})
print("first 12 start-to-start us:", np.round(d1[500:512], 1).tolist())
