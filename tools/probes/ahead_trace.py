#!/usr/bin/env python3
"""Where the partition front of step i+1 runs relative to the RANSAC kernel of step i, out of a rocprofv3
--kernel-trace CSV of bench.py.  Steps are counted by their k_build_begin; the j-th launch of
k_ransac<64, 16, 6, ...> (the one-wave instance: the main kernel of a headline step) is the RANSAC of step j and is
paired with the front of step j+1: the first k_part_hist and k_part_scatter behind the (j+1)-th k_build_begin.  All
times in microseconds, relative to the begin / the end of that k_ransac launch.
usage: tools/probes/ahead_trace.py <dir with *_kernel_trace.csv> [steps to skip at the front, default 4]"""
import csv, glob, os, statistics, sys

f = sorted(glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)[-1]
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 4
ev = []
for r in csv.DictReader(open(f)):
    name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
    ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name, r.get("Stream_Id", "?")))
ev.sort()
begin = [e for e in ev if e[2].startswith("k_build_begin")]
main = [e for e in ev if e[2].startswith("k_ransac<64, 16, 6")]
hist = [e for e in ev if e[2].startswith("k_part_hist<")]
scat = [e for e in ev if e[2].startswith("k_part_scatter<")]
build = [e for e in ev if e[2].startswith("k_bucket_build")]


def first_behind(events, t):
    return next((e for e in events if e[0] >= t), None)


rows = []
for j in range(min(len(main), len(begin) - 1)):
    r, b = main[j], begin[j + 1]
    h, s, k = first_behind(hist, b[0]), first_behind(scat, b[0]), first_behind(build, b[0])
    if h is None or s is None or k is None or abs(b[0] - r[0]) > 5e6:   # (5 ms apart: not neighbours - another phase of the run)
        continue
    rows.append({
        "ransac_us": (r[1] - r[0]) / 1e3,
        "front_begin_vs_ransac_begin": (b[0] - r[0]) / 1e3,
        "hist_begin_vs_ransac_begin": (h[0] - r[0]) / 1e3, "hist_end_vs_ransac_end": (h[1] - r[1]) / 1e3,
        "hist_us": (h[1] - h[0]) / 1e3,
        "scatter_begin_vs_ransac_begin": (s[0] - r[0]) / 1e3, "scatter_begin_vs_ransac_end": (s[0] - r[1]) / 1e3,
        "scatter_end_vs_ransac_end": (s[1] - r[1]) / 1e3, "scatter_us": (s[1] - s[0]) / 1e3,
        "bucket_build_begin_vs_ransac_end": (k[0] - r[1]) / 1e3,
        "streams": "ransac %s hist %s scatter %s" % (r[3], h[3], s[3]),
    })
rows = rows[skip:]
print("%s: %d steps (the first %d skipped)" % (os.path.basename(f), len(rows), skip))
if not rows:
    sys.exit(0)
for k in rows[0]:
    if k == "streams":
        print("%-34s %s" % (k, sorted(set(r[k] for r in rows))))
        continue
    v = [r[k] for r in rows]
    print("%-34s mean %9.1f  median %9.1f  min %9.1f  max %9.1f" % (k, statistics.mean(v), statistics.median(v), min(v), max(v)))
n = sum(1 for r in rows if r["hist_begin_vs_ransac_begin"] < r["ransac_us"])
print("steps whose k_part_hist begins before the end of the previous step's k_ransac: %d of %d" % (n, len(rows)))
n = sum(1 for r in rows if r["scatter_begin_vs_ransac_end"] < 0)
print("steps whose k_part_scatter begins before the end of the previous step's k_ransac: %d of %d" % (n, len(rows)))
n = sum(1 for r in rows if r["scatter_end_vs_ransac_end"] < 0)
print("steps whose k_part_scatter ends before the end of the previous step's k_ransac: %d of %d" % (n, len(rows)))
