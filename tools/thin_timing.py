"""Device time of the cell count and of voxel-grid thinning on a window with heavy overlap: 16 poses of 100 k points
each, every pose another draw of the SAME planar scene (8 x 8 x 4 voxels of 1 m, so every surface is seen 16 times),
Grid of 1 m voxels, subdivide(len > 64).  Arms on maps built afresh (thinning changes the map), medians with min - max:

  (a) thin           thin(cell) for cell in {L/32, L/8, L/2}: kernel time of k_thin_mask and of the compaction from the
                     library's hipEvent timers, wall time of the call (the index in place), points before and after
  (b) cell_count     kernel time of k_cell_count for one 100 k scan (a 17th draw, in HBM), uncapped and max_count = 1
  (c) remove_sparse  remove_sparse(radius=cell, min_neighbours) on the same map: the yardstick among the device edits
  (d) host path      what users had: the clouds read back and thin_keep_np on the host (the rule alone, wall time)
  (e) nearest        k_nearest<1> for the same scan before and after thin(L/8): what the consumers gain

No pass/fail threshold.  Prints one JSON object.

    python tools/thin_timing.py [--poses 16] [--points 100000] [--rounds 3]
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--k-split", type=int, default=64)
    ap.add_argument("--min-neighbours", type=int, default=4)
    args = ap.parse_args()

    from octreelib_amd import MaxPoints, cell_count, synthetic, thin, thin_keep_np
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig

    dims, L = (8, 8, 4), 1.0
    clouds = [synthetic.planar_cloud(args.points, dims, seed=1, stream=p) for p in range(args.poses)]
    scan = synthetic.planar_cloud(args.points, dims, seed=1, stream=args.poses)
    ctx = nat.get_context()
    lib = ctx.lib
    cells = {"L/32": L / 32, "L/8": L / 8, "L/2": L / 2}

    def build():
        g = Grid(GridConfig(voxel_edge_length=1))
        for p, P in enumerate(clouds):
            g.insert_points(p, P)
        g.subdivide([MaxPoints(args.k_split)])
        g._forest.ensure_built()
        cell_count(g, scan[:1], L / 8)                 # (the index of every pose is in place)
        ctx.sync()
        return g

    def timed(fn, prefixes):
        ctx.set_profiling(1)
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e6
        t = ctx.timings()
        ctx.set_profiling(0)
        return {k: ms * 1e3 for k, (ms, _) in t.items() if k.startswith(prefixes)}, wall, out

    xin, d_count = C.c_void_p(), C.c_void_p()
    d_slot, d_index, d_d2 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    nq = len(scan)
    for p, nbytes in ((xin, 24 * nq), (d_count, 4 * nq), (d_slot, 4 * nq), (d_index, 8 * nq), (d_d2, 8 * nq)):
        ctx.check(lib.octl_dev_alloc(ctx.handle, nbytes, C.byref(p)))
    ctx.check(lib.octl_dev_upload(ctx.handle, xin, nat.ptr(scan), scan.nbytes))

    out = {"poses": args.poses, "points_per_pose": args.points, "rounds": args.rounds, "voxel_edge": L, "thin": {},
           "cell_count": {}, "remove_sparse": {}, "host_rule_wall_us": {}, "nearest_k1_kernel_us": {}}

    def nearest_us(g):
        f = g._forest
        fn = lambda: f.nearest_device(xin, nq, 1, L / 8, d_slot, d_index, d_d2, d_count)
        fn()
        ctx.sync()
        return [timed(fn, ("nearest_k1",))[0]["nearest_k1"] for _ in range(args.rounds)]

    for name, cell in cells.items():
        mask_k, compact_k, wall_us, left, sparse_k, sparse_wall, sparse_left = [], [], [], set(), [], [], set()
        for i in range(args.rounds):
            g = build()
            f = g._forest
            before = int(f.n_ord)
            if i == 0:
                count_us = {"uncapped": [], "cap1": []}
                for arm, cap in (("uncapped", None), ("cap1", 1)):
                    fn = lambda: f.cell_count_device(xin, nq, cell, d_count, cap)
                    fn()
                    ctx.sync()
                    count_us[arm] = [timed(fn, ("cell_count",))[0]["cell_count"] for _ in range(args.rounds)]
                cnt = np.empty(nq, dtype=np.int32)
                f.cell_count_device(xin, nq, cell, d_count)
                ctx.check(lib.octl_dev_download(ctx.handle, nat.ptr(cnt), d_count, cnt.nbytes))
                out["cell_count"][name] = {"uncapped_kernel_us": _stat(count_us["uncapped"]),
                                           "cap1_kernel_us": _stat(count_us["cap1"]),
                                           "mean_count": round(float(cnt.mean()), 2),
                                           "share_new": round(float((cnt == 0).mean()), 4)}
                if name == "L/8":
                    out["nearest_k1_kernel_us"]["before"] = _stat(nearest_us(g))
                t0 = time.perf_counter()
                keep = thin_keep_np([(p, g.get_points(p)) for p in range(args.poses)], None, cell)
                out["host_rule_wall_us"][name] = round((time.perf_counter() - t0) * 1e6, 1)
                host_left = int(sum(int(k.sum()) for k in keep))
            k, wall, removed = timed(lambda: thin(g, cell), ("thin_mask", "apply_mask"))
            mask_k.append(k["thin_mask"])
            compact_k.append(k["apply_mask"])
            wall_us.append(wall)
            left.add(int(f.n_ord))
            if i == 0 and name == "L/8":
                cell_count(g, scan[:1], cell)
                out["nearest_k1_kernel_us"]["after"] = _stat(nearest_us(g))
            g = build()
            f = g._forest
            k, wall, _ = timed(lambda: g.remove_sparse(cell, args.min_neighbours), ("sparse_mask", "apply_mask"))
            sparse_k.append(k["sparse_mask"])
            sparse_wall.append(wall)
            sparse_left.add(int(f.n_ord))
            print(f"cell {name} round {i}: done", file=sys.stderr, flush=True)
        out["thin"][name] = {"cell": cell, "points_before": before, "points_after": sorted(left),
                             "host_rule_agrees": left == {host_left}, "thin_mask_kernel_us": _stat(mask_k),
                             "compaction_kernel_us": _stat(compact_k), "call_wall_us": _stat(wall_us)}
        out["remove_sparse"][name] = {"radius": cell, "min_neighbours": args.min_neighbours,
                                      "sparse_mask_kernel_us": _stat(sparse_k), "call_wall_us": _stat(sparse_wall),
                                      "points_after": sorted(sparse_left)}
    for p in (xin, d_count, d_slot, d_index, d_d2):
        lib.octl_dev_free(ctx.handle, p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
