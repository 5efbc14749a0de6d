"""Device time of the neighbourhood statistics on the window of tools/thin_timing.py: 16 poses of 100 k points each,
every pose another draw of the SAME planar scene (8 x 8 x 4 voxels of 1 m), Grid of 1 m voxels, subdivide(len > 64);
the queries are a 17th draw (in HBM).  Every arm before and after thin(map, L/8), at radius L/8, arms alternated in one
process, medians with min - max:

  (a) neighbourhood_statistics   kernel time of k_neighbourhood_stats for the 100 k scan, eigen=False and eigen=True,
                                 from the library's hipEvent timers
  (b) radius_count               k_radius_count (uncapped) of the same queries at the same radius: the same walk without
                                 the moments - the ratio (a) / (b) is what the nine sums and the rows cost
  (c) point_statistics           the self-query of the newest pose against the whole map: kernel time of k_point_stats
                                 and the wall time of the call (download, sort and all)
  (d) host definition            neighbourhood_statistics_np on a subsample of the scan (wall time, scaled to the scan)

No pass/fail threshold.  Prints one JSON object.

    python tools/normals_timing.py [--poses 16] [--points 100000] [--rounds 5] [--subsample 64]
"""

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stat(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--k-split", type=int, default=64)
    ap.add_argument("--subsample", type=int, default=64)
    args = ap.parse_args()

    from octreelib_amd import MaxPoints, neighbourhood_statistics_np, point_statistics, synthetic, thin
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig

    dims, L = (8, 8, 4), 1.0
    r = L / 8
    clouds = [synthetic.planar_cloud(args.points, dims, seed=1, stream=p) for p in range(args.poses)]
    scan = synthetic.planar_cloud(args.points, dims, seed=1, stream=args.poses)
    ctx = nat.get_context()
    lib = ctx.lib
    g = Grid(GridConfig(voxel_edge_length=1))
    for p, P in enumerate(clouds):
        g.insert_points(p, P)
    g.subdivide([MaxPoints(args.k_split)])
    f = g._forest
    f.ensure_built()

    def timed(fn, prefixes):
        ctx.set_profiling(1)
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e6
        t = ctx.timings()
        ctx.set_profiling(0)
        return {k: ms * 1e3 for k, (ms, _) in t.items() if k.startswith(prefixes)}, wall, out

    nq = len(scan)
    bufs = {name: C.c_void_p() for name in ("xin", "count32", "count", "mean", "cov", "w", "v")}
    sizes = {"xin": 24 * nq, "count32": 4 * nq, "count": 8 * nq, "mean": 24 * nq, "cov": 48 * nq, "w": 24 * nq, "v": 72 * nq}
    for name, p in bufs.items():
        ctx.check(lib.octl_dev_alloc(ctx.handle, sizes[name], C.byref(p)))
    ctx.check(lib.octl_dev_upload(ctx.handle, bufs["xin"], nat.ptr(scan), scan.nbytes))
    b = bufs
    arms = {
        "moments": (lambda: f.neighbourhood_stats_device(b["xin"], nq, r, b["count"], b["mean"], b["cov"]),
                    "neighbourhood_stats"),
        "moments_eigen": (lambda: f.neighbourhood_stats_device(b["xin"], nq, r, b["count"], b["mean"], b["cov"],
                                                               b["w"], b["v"]), "neighbourhood_stats"),
        "radius_count": (lambda: f.radius_count_device(b["xin"], nq, r, b["count32"]), "radius_count"),
    }
    out = {"poses": args.poses, "points_per_pose": args.points, "rounds": args.rounds, "voxel_edge": L, "radius": r}
    for stage in ("before_thin", "after_thin"):
        if stage == "after_thin":
            thin(g, L / 8)
        for fn, _ in arms.values():                       # (warm: the index of every pose is in place)
            fn()
        ctx.sync()
        cnt = np.empty(nq, dtype=np.int32)
        ctx.check(lib.octl_dev_download(ctx.handle, nat.ptr(cnt), b["count32"], cnt.nbytes))
        us = {name: [] for name in arms}
        for _ in range(args.rounds):                      # arms alternated
            for name, (fn, timer) in arms.items():
                k, _, _ = timed(fn, (timer,))
                us[name].append(k[timer])
        med = {name: statistics.median(v) for name, v in us.items()}
        newest = args.poses - 1
        point_statistics(g, r, pose_numbers=[newest])     # (warm)
        self_k, self_wall, rows = [], [], 0
        for _ in range(args.rounds):
            k, wall, ps = timed(lambda: point_statistics(g, r, pose_numbers=[newest]), ("point_stats",))
            self_k.append(k["point_stats"])
            self_wall.append(wall)
            rows = len(ps)
        sub = scan[:args.subsample]
        stored = [(p, g.get_points(p)) for p in range(args.poses)]
        t0 = time.perf_counter()
        neighbourhood_statistics_np(sub, stored, r, chunk=8)
        host_us = (time.perf_counter() - t0) * 1e6
        out[stage] = {"map_points": int(f.n_ord), "mean_count": round(float(cnt.mean()), 2),
                      "max_count": int(cnt.max()),
                      **{name + "_kernel_us": _stat(v) for name, v in us.items()},
                      "moments_over_radius_count": round(med["moments"] / med["radius_count"], 3),
                      "moments_eigen_over_radius_count": round(med["moments_eigen"] / med["radius_count"], 3),
                      "point_stats_newest_kernel_us": _stat(self_k), "point_stats_newest_wall_us": _stat(self_wall),
                      "point_stats_rows": rows,
                      "host_definition_wall_us_subsample": round(host_us, 1), "subsample": len(sub),
                      "host_definition_wall_us_scaled_to_scan": round(host_us * nq / max(len(sub), 1), 1)}
        print(f"{stage}: done", file=sys.stderr, flush=True)
    for p in bufs.values():
        lib.octl_dev_free(ctx.handle, p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
