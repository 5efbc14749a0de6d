"""Device time of the store pass of remove_poses and the wall time of a window step, on BASELINE config 3 (planar
points, Grid of 1 m voxels, subdivide(len > 64), RANSAC with H = 1024, k = 6, thr = 0.01, incl. apply_mask): DESIGN.md
4.17's tables.  Arms alternated in one process, medians with min - max.

  kernel   hipEvent time of k_retire_poses alone (the library's timer "remove_poses" on a forest WITHOUT tables: the
           fitted map's scheme is dropped by an identity transform_poses first, which leaves the dead rows and their flags
           where they are, so the call is the store pass and nothing else) against k_ingest<true> (timer "ingest": a
           device cloud of as many rows as the squeezed store holds copied into a fresh forest's store and folded into
           its box).  Per row of the NEW store the retire pass moves 50 B (24 read, 24 written, a flag byte read and
           one written) and its time includes k_alive_count; the ingest moves 49 B (no flag to read).  Scenes: the
           first of three poses removed with an even and with an odd number of rows (the odd one puts every source unit 8
           bytes off its destination), the first of 64.
  window   from Python: remove_poses of the oldest of 16 poses of 100 k points on the fitted map, against the only
           alternative without it - a fresh Grid, the 15 remaining DeviceClouds inserted again, subdivide, RANSAC,
           apply_mask.

Prints one JSON object.

    python tools/remove_poses_timing.py [--n 10000000] [--calls 8] [--steps 8] [--no-window]
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
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--k-split", type=int, default=64)
    ap.add_argument("--no-window", action="store_true", help="kernel times only")
    args = ap.parse_args()

    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd import _native as nat
    from octreelib_amd._engine import Forest
    from octreelib_amd.feed import DeviceCloud
    from octreelib_amd.grid import Grid, GridConfig

    side = 32 if args.n >= 1_000_000 else 8
    P = synthetic.planar_cloud(args.n, (side, side, side), seed=1)
    np.random.seed(0)
    table = np.random.random((1024, 6))
    ctx = nat.get_context()
    lib = ctx.lib

    def fit(g):
        g.subdivide([MaxPoints(args.k_split)])
        f = g._forest
        f.ransac_all(10, table, 0.01)
        f.apply_device_mask()
        return f.n_ord               # (books the compaction's counts: the host has waited)

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
    third = args.n // 3
    scenes = {"first_of_3_even_shift": [third - third % 2, third, args.n - 2 * third + third % 2],
              "first_of_3_odd_shift": [third - third % 2 + 1, third, args.n - 2 * third + third % 2 - 1],
              "first_of_64": [args.n // 64] * 63 + [args.n - 63 * (args.n // 64)]}
    eye = np.eye(4)
    for name, sizes in scenes.items():
        cut = np.concatenate([[0], np.cumsum(sizes)])
        rows = int(args.n - sizes[0])
        rm, ing, alive = [], [], 0
        for i in range(args.calls):
            g = Grid(GridConfig(voxel_edge_length=1))
            for p in range(len(sizes)):
                g.insert_points(p, P[cut[p]:cut[p + 1]])
            alive = int(fit(g))
            g.transform_poses([eye] * len(sizes))          # no tables from here on; dead rows stay dead
            rm.append(timed(lambda: g.remove_poses([0]), "remove_poses"))
            assert g._forest.store_size()[0] == rows
            g._forest.close()
            fresh = Forest(0, np.zeros(3), 1.0)
            ing.append(timed(lambda: fresh.add_pose_device(scan, rows), "ingest"))
            ctx.sync()
            fresh.close()
        if len(rm) > 2:                                     # (the first round sizes the blocks)
            rm, ing = rm[1:], ing[1:]
        mr, mi = statistics.median(rm), statistics.median(ing)
        out["kernel"][name] = {
            "poses": len(sizes), "removed_rows": int(sizes[0]), "rows_after": rows, "alive_rows_before": alive,
            "retire_us": _stat(rm), "ingest_copy_us": _stat(ing),
            "retire_ns_per_byte": round(mr * 1e3 / (rows * 50), 5),
            "ingest_ns_per_byte": round(mi * 1e3 / (rows * 49), 5),
            "retire_TB_per_s": round(rows * 50 / (mr * 1e-6) / 1e12, 2),
            "ingest_TB_per_s": round(rows * 49 / (mi * 1e-6) / 1e12, 2),
            "ratio_per_byte": round((mr / 50) / (mi / 49), 3)}
    lib.octl_dev_free(ctx.handle, scan)

    if not args.no_window:
        W, m = 16, 100_000
        total = W + args.steps
        Q = synthetic.planar_cloud(m * total, (16, 16, 16), seed=2)
        clouds = [DeviceCloud(np.ascontiguousarray(Q[k * m:(k + 1) * m])) for k in range(total)]
        ctx.sync()
        g = Grid(GridConfig(voxel_edge_length=1))
        for k in range(W):
            g.insert_points(k, clouds[k])
        fit(g)
        f = g._forest
        wall_a, wall_b = [], []
        for s in range(args.steps):
            oldest, newest = s, W + s
            ctx.sync()
            t0 = time.perf_counter()
            g.remove_poses([oldest])
            wall_a.append((time.perf_counter() - t0) * 1e3)
            assert f.store_size()[0] == (W - 1) * m
            # today's alternative for the same 15 poses: everything again
            ctx.sync()
            t0 = time.perf_counter()
            b = Grid(GridConfig(voxel_edge_length=1))
            for k in range(oldest + 1, newest):
                b.insert_points(k, clouds[k])
            fit(b)
            wall_b.append((time.perf_counter() - t0) * 1e3)
            b._forest.close()
            # the window moves on (not timed): the next scan comes in late and is fitted
            g.insert_points(newest, clouds[newest])
            f.ransac_all(10, table, 0.01)
            f.apply_device_mask()
            f.n_ord
        out["window"] = {"poses": W, "points_per_pose": m, "steps": args.steps,
                         "remove_poses_ms": _stat(wall_a, 3), "rebuild_ms": _stat(wall_b, 2),
                         "speedup": round(statistics.median(wall_b) / statistics.median(wall_a), 1)}
        f.close()
        for c in clouds:
            c.release()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
