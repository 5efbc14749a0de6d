"""Device time of transform_poses and the wall time of the cycle it closes, on BASELINE config 3 (10 M planar points,
Grid of 1 m voxels, subdivide(len > 64), map_leaf_points_cuda_ransac with H = 1024, k = 6, thr = 0.01, incl.
apply_mask): DESIGN.md 4.13's table.  Arms alternated in one process, medians with min - max over the rounds.

  kernel   hipEvent time of k_transform_poses (the library's timer "transform_poses") on the fitted map, every pose
           selected, and of k_ingest<true> (timer "ingest": a device cloud of the same number of rows copied into a fresh
           forest's store and folded into its box) - the project's own copy-and-fold stream, the yardstick.  Once with
           one pose and once with three.  ns per row, ns per byte moved (49 B per row for the transform: 24 read, 24
           written, the alive flag; 48 + the flag written for the ingest), and the ratio of the two.
  cycle    from Python: transform_poses + subdivide + RANSAC + apply_mask, against the only alternative without it -
           get_points of every pose, transform_np, a fresh Grid, insert_points - followed by the same three steps.

Prints one JSON object.

    python tools/transform_poses_timing.py [--n 10000000] [--calls 20] [--cycles 3] [--no-cycle]
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


def _stat(v, digits=1):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits),
            "max": round(max(v), digits)} if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--cycles", type=int, default=3)
    ap.add_argument("--k-split", type=int, default=64)
    ap.add_argument("--no-cycle", action="store_true", help="kernel times only")
    args = ap.parse_args()

    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd import _native as nat
    from octreelib_amd._engine import Forest
    from octreelib_amd.grid import Grid, GridConfig
    from octreelib_amd.registration import se3_exp, transform_np

    side = 32 if args.n >= 1_000_000 else 8
    P = synthetic.planar_cloud(args.n, (side, side, side), seed=1)
    np.random.seed(0)
    table = np.random.random((1024, 6))
    ctx = nat.get_context()
    lib = ctx.lib
    centre = np.full(3, side / 2.0)
    fwd = se3_exp([0.0, 0.0, 0.01, 0.2, -0.1, 0.05], centre)     # a small step about the scene's centre
    back = np.linalg.inv(fwd)

    def fitted(clouds):
        g = Grid(GridConfig(voxel_edge_length=1))
        for p, X in enumerate(clouds):
            g.insert_points(p, X)
        fit(g)
        return g

    def fit(g):
        g.subdivide([MaxPoints(args.k_split)])
        g.map_leaf_points_cuda_ransac(hypotheses=table)
        return g._forest.n_ord       # (books the compaction's counts: the host has waited)

    def timed(fn, name):
        ctx.set_profiling(1)
        fn()
        ctx.sync()
        t = ctx.timings()
        ctx.set_profiling(0)
        return t[name][0] * 1e3      # us

    out = {"config": "config3", "n": args.n, "calls": args.calls, "kernel": {}}
    scan = C.c_void_p()
    ctx.check(lib.octl_dev_alloc(ctx.handle, P.nbytes, C.byref(scan)))
    ctx.check(lib.octl_dev_upload(ctx.handle, scan, nat.ptr(P), P.nbytes))
    for n_poses in (1, 3):
        cut = [args.n * k // n_poses for k in range(n_poses + 1)]
        g = fitted([P[cut[k]:cut[k + 1]] for k in range(n_poses)])
        f = g._forest
        alive = int(f.n_ord)
        xf, ing = [], []
        g.transform_poses([fwd] * n_poses)          # (the first call sizes the second block)
        g.transform_poses([back] * n_poses)
        for i in range(args.calls):                 # arms alternated
            T = fwd if i % 2 == 0 else back
            xf.append(timed(lambda: g.transform_poses([T] * n_poses), "transform_poses"))
            fresh = Forest(0, np.zeros(3), 1.0)
            ing.append(timed(lambda: fresh.add_pose_device(scan, args.n), "ingest"))
            ctx.sync()
            fresh.close()
        rows = args.n
        mx, mi = statistics.median(xf), statistics.median(ing)
        out["kernel"][f"{n_poses}_pose" + ("s" if n_poses > 1 else "")] = {
            "rows": rows, "alive_rows": alive,
            "transform_us": _stat(xf), "ingest_copy_us": _stat(ing),
            "transform_ns_per_row": round(mx * 1e3 / rows, 4), "ingest_ns_per_row": round(mi * 1e3 / rows, 4),
            "transform_ns_per_byte": round(mx * 1e3 / (rows * 49), 5),
            "ingest_ns_per_byte": round(mi * 1e3 / (rows * 49), 5),
            "transform_TB_per_s": round(rows * 49 / (mx * 1e-6) / 1e12, 2),
            "ingest_TB_per_s": round(rows * 49 / (mi * 1e-6) / 1e12, 2),
            "ratio_per_byte": round(mx / mi, 3)}
        if n_poses == 3 and not args.no_cycle:
            # ---- the cycle: A moves its map in place, B downloads, moves on the host and inserts again ---------------
            fit(g)
            b = fitted([P[cut[k]:cut[k + 1]] for k in range(n_poses)])
            wall_a, wall_b, parts_b = [], [], []
            for i in range(args.cycles):
                T = fwd if i % 2 == 0 else back
                ctx.sync()
                t0 = time.perf_counter()
                g.transform_poses([T] * n_poses)
                t1 = time.perf_counter()
                fit(g)
                wall_a.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
                ctx.sync()
                t0 = time.perf_counter()
                clouds = [b.get_points(p) for p in range(n_poses)]
                t1 = time.perf_counter()
                clouds = [transform_np(T, X) for X in clouds]
                t2 = time.perf_counter()
                b._forest.close()
                b = Grid(GridConfig(voxel_edge_length=1))
                for p, X in enumerate(clouds):
                    b.insert_points(p, X)
                t3 = time.perf_counter()
                fit(b)
                t4 = time.perf_counter()
                wall_b.append((t4 - t0) * 1e3)
                parts_b.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3))
            out["cycle"] = {
                "poses": n_poses, "rounds": args.cycles,
                "write_back_ms": _stat([w[0] for w in wall_a], 2),
                "of_which_transform_poses_ms": _stat([w[1] for w in wall_a], 3),
                "host_round_trip_ms": _stat(wall_b, 1),
                "host_parts_ms": {k: _stat([p[j] for p in parts_b], 1)
                                  for j, k in enumerate(("get_points", "transform_np", "insert_points", "fit"))},
                "speedup": round(statistics.median(wall_b) / statistics.median([w[0] for w in wall_a]), 2)}
            b._forest.close()
        f.close()
    lib.octl_dev_free(ctx.handle, scan)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
