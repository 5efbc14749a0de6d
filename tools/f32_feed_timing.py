"""A/B of the float32 input path against f64 on BASELINE config 3 (10 M planar points, Grid of 1 m voxels,
subdivide(len > 64), map_leaf_points_cuda_ransac with H = 1024, k = 6, thr = 0.01, incl. apply_mask).

The cloud is rounded to f32 once and the f64 arm gets exactly those values widened, so both arms build identical
trees and do identical RANSAC work; the only difference is the dtype handed to the library (24 or 12 bytes per
point over PCIe, host upcast or device widening).  The arms run alternately in one process, after a warm-up, for:

  api_inclusive   a fresh Grid, insert_points(host array), subdivide, RANSAC, n_points (bench.py's api_inclusive)
  api_pipelined   the same with scan i+1 handed over early: upload_async(pinned_empty buffer), 16 scans
  scan_pipeline   ScanPipeline(2) over a ring of 5 pinned buffers, 16 scans

Every scan's n_points after RANSAC must be the same in both arms.  Prints one JSON object.

    python tools/f32_feed_timing.py [--rounds 5] [--n 10000000]
    python tools/f32_feed_timing.py --profile-ingest      # insertions only, for rocprofv3 --kernel-trace --stats
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(samples_ms, n):
    med = statistics.median(samples_ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(samples_ms), 4), "ms_max": round(max(samples_ms), 4),
            "Mpoints_per_s": round(n / med / 1e3, 1), "samples": len(samples_ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scans", type=int, default=16)
    ap.add_argument("--k-split", type=int, default=64)
    ap.add_argument("--profile-ingest", action="store_true",
                    help="only insertions (f32 host, f32 DeviceCloud, f64 host), for a kernel trace")
    args = ap.parse_args()

    import octreelib_amd as oa
    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig

    n = args.n
    p32 = synthetic.planar_cloud(n, (32, 32, 32), seed=1).astype(np.float32)
    p64 = p32.astype(np.float64)
    np.random.seed(0)
    table = np.random.random((1024, 6))
    ctx = nat.get_context()

    if args.profile_ingest:
        clouds = {"f32": p32, "f64": p64}
        for _ in range(10):
            for name in ("f32", "f64"):
                g = Grid(GridConfig(voxel_edge_length=1))
                g.insert_points(0, clouds[name])
                g._forest.close()
            dc = oa.upload_async(p32)
            g = Grid(GridConfig(voxel_edge_length=1))
            g.insert_points(0, dc)
            ctx.sync()
            g._forest.close()
            dc.release()
        print(json.dumps({"profile_ingest": "done", "n": n, "inserts_per_kind": 10}))
        return

    def fit(grid, i=0):
        grid.subdivide([MaxPoints(args.k_split)])
        grid.map_leaf_points_cuda_ransac(hypotheses=table)
        return grid.n_points(0)

    # -- api_inclusive --------------------------------------------------------------------------------------------
    host = {"f64": p64, "f32": p32}

    def inclusive(dt):
        t0 = time.perf_counter()
        g = Grid(GridConfig(voxel_edge_length=1))
        g.insert_points(0, host[dt])
        kept = fit(g)
        g._forest.close()
        return (time.perf_counter() - t0) * 1e3, kept

    # -- api_pipelined --------------------------------------------------------------------------------------------
    stage = {dt: [oa.pinned_empty((n, 3), host[dt].dtype) for _ in range(5)] for dt in host}
    for dt in host:
        for s in stage[dt]:
            s[:] = host[dt]

    def pipelined(dt, count):
        st = stage[dt]
        kept = []
        t0 = time.perf_counter()
        nxt = oa.upload_async(st[0])
        for i in range(count):
            cur = nxt
            g = Grid(GridConfig(voxel_edge_length=1))
            g.insert_points(0, cur)
            nxt = oa.upload_async(st[(i + 1) & 1]) if i + 1 < count else None
            kept.append(fit(g))
            g._forest.close()
            cur.release()
        return (time.perf_counter() - t0) * 1e3 / count, kept

    # -- ScanPipeline(2) ------------------------------------------------------------------------------------------
    pipes = {dt: oa.ScanPipeline(2) for dt in host}

    def scan_pipeline(dt, count):
        t0 = time.perf_counter()
        kept = list(pipes[dt].map((stage[dt][i % 5] for i in range(count)), fit))
        return (time.perf_counter() - t0) * 1e3 / count, kept

    res = {k: {"f64": [], "f32": []} for k in ("api_inclusive", "api_pipelined", "scan_pipeline")}
    kept_all = {"f64": set(), "f32": set()}
    try:
        for dt in host:   # warm-up: pools, hypothesis tables, staging buffers of every arm
            inclusive(dt)
            pipelined(dt, 2)
            scan_pipeline(dt, 4)
        for r in range(args.rounds):
            order = ("f64", "f32") if r % 2 == 0 else ("f32", "f64")
            for dt in order:
                for _ in range(3):
                    ms, k = inclusive(dt)
                    res["api_inclusive"][dt].append(ms)
                    kept_all[dt].add(k)
                ms, k = pipelined(dt, args.scans)
                res["api_pipelined"][dt].append(ms)
                kept_all[dt].update(k)
                ms, k = scan_pipeline(dt, args.scans)
                res["scan_pipeline"][dt].append(ms)
                kept_all[dt].update(k)
    finally:
        for p in pipes.values():
            p.close()

    out = {"tool": "f32_feed_timing", "n": n, "rounds": args.rounds, "scans_per_loop": args.scans,
           "points_after_ransac": sorted(kept_all["f64"]),
           "same_points_after_ransac": kept_all["f32"] == kept_all["f64"] and len(kept_all["f64"]) == 1}
    for loop, arms in res.items():
        out[loop] = {dt: _stats(v, n) for dt, v in arms.items()}
        out[loop]["f32_speedup"] = round(out[loop]["f64"]["ms_median"] / out[loop]["f32"]["ms_median"], 3)
    print(json.dumps(out))
    if not out["same_points_after_ransac"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
