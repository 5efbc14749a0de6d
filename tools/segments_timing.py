"""Device time of plane_segments on BASELINE config 3 (10 M planar points, Grid of 1 m voxels, subdivide(len > 64),
map_leaf_points_cuda_ransac with H = 1024, k = 6, thr = 0.01, incl. apply_mask): the map of DESIGN.md 4.8's table.
Arms alternated in one process, medians with min - max over the rounds, kernel times from the library's hipEvent timers:

  segments       every timed region of a computation of octl_forest_plane_segments on an existing pooled table (the
                 gates change from round to round, so nothing is answered from the cache), by name and in total
  locate         octl_forest_locate_device on the 6 x rows probe points of the same map, shuffled: the walk alone,
                 the floor of seg_link - and the ratio to it
  pooled         the kernels of one octl_forest_pooled_leaf_stats (asked for another selection than the table in
                 place, so every call computes)
  wall           a plane_segments call from Python (computation and download), and plane_segments_np on the
                 downloaded tables: the host loop this replaces

Prints one JSON object.

    python tools/segments_timing.py [--n 10000000] [--rounds 7] [--no-host]
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
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--k-split", type=int, default=64)
    ap.add_argument("--no-host", action="store_true", help="skip plane_segments_np on the downloaded tables")
    args = ap.parse_args()

    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig
    from octreelib_amd.query import plane_segments_np, segment_probes_np

    side = 32 if args.n >= 1_000_000 else 8
    P = synthetic.planar_cloud(args.n, (side, side, side), seed=1)
    np.random.seed(0)
    table = np.random.random((1024, 6))
    ctx = nat.get_context()
    lib = ctx.lib

    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P)
    g.subdivide([MaxPoints(args.k_split)])
    g.map_leaf_points_cuda_ransac(hypotheses=table)
    f = g._forest
    f.ensure_built()
    f.n_ord   # (books the compaction's counts)
    planes = g.leaf_planes()
    R = len(planes)

    def timed(fn):
        ctx.set_profiling(1)
        fn()
        ctx.sync()
        t = ctx.timings()
        ctx.set_profiling(0)
        return {k: ms * 1e3 for k, (ms, _) in t.items()}

    def segments(angle):
        nr, ns = C.c_int64(0), C.c_int64(0)
        ctx.check(lib.octl_forest_plane_segments(f.handle, None, 0, 8, -1.0, float(np.cos(angle)), 0.05, 0, 0,
                                                 *([None] * 9), C.byref(nr), C.byref(ns)))
        return nr.value, ns.value

    nd = f.nodes
    probes = segment_probes_np(nd["corner"][planes.node], nd["edge"][planes.node]).reshape(-1, 3)
    probes = np.ascontiguousarray(probes[np.random.default_rng(0).permutation(len(probes))])
    xin, d_node = C.c_void_p(), C.c_void_p()
    ctx.check(lib.octl_dev_alloc(ctx.handle, probes.nbytes, C.byref(xin)))
    ctx.check(lib.octl_dev_alloc(ctx.handle, 4 * len(probes), C.byref(d_node)))
    ctx.check(lib.octl_dev_upload(ctx.handle, xin, nat.ptr(probes), probes.nbytes))
    f.locate_device(xin, len(probes), d_node)
    segments(0.1)
    ctx.sync()

    names = ("seg_init", "seg_link", "seg_flatten", "seg_scan", "seg_keys", "seg_sort", "seg_merge")
    seg = {k: [] for k in names}
    total, loc, pooled, wall = [], [], [], []
    n_segs = None
    for i in range(args.rounds):           # arms alternated
        angle = 0.1 + 0.001 * (i + 1)
        t = timed(lambda: segments(angle))
        for k in names:
            seg[k].append(t.get(k, 0.0))
        total.append(sum(t.get(k, 0.0) for k in names))
        loc.append(timed(lambda: f.locate_device(xin, len(probes), d_node))["locate"])
        f._pooled = None
        t = timed(lambda: f.leaf_planes([0]))      # (another selection than the table in place: computed)
        pooled.append(sum(v for k, v in t.items() if k.startswith("pool_")))
        f._pooled = None
        g.leaf_planes()
        t0 = time.perf_counter()
        ps = g.plane_segments(max_angle=0.2 + 0.001 * i)
        wall.append((time.perf_counter() - t0) * 1e3)
        n_segs = len(ps.segments.count)
    for p in (xin, d_node):
        lib.octl_dev_free(ctx.handle, p)

    med = statistics.median
    out = {"config": "config3", "n": args.n, "map_points": int(f.n_ord), "nodes": int(len(nd["edge"])), "rows": R,
           "segments_at_0.2": n_segs, "rounds": args.rounds,
           "segments_kernels_us": {k: _stat(v) for k, v in seg.items()}, "segments_total_us": _stat(total),
           "locate_6R_us": _stat(loc), "pooled_leaf_stats_us": _stat(pooled),
           "seg_link_over_locate": round(med(seg["seg_link"]) / med(loc), 2),
           "total_over_locate": round(med(total) / med(loc), 2),
           "total_over_pooled": round(med(total) / med(pooled), 2),
           "call_wall_ms": _stat(wall)}
    if not args.no_host:
        ps = g.plane_segments()
        t0 = time.perf_counter()
        ref = plane_segments_np(ps.planes, nd, f.voxels, f.mode, f._cube[1])
        out["plane_segments_np_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out["equal_to_np"] = bool(np.array_equal(ref.neighbour, ps.neighbour) and np.array_equal(ref.label, ps.label)
                                  and np.array_equal(ref.segments.root, ps.segments.root)
                                  and np.array_equal(ref.segments.n_leaves, ps.segments.n_leaves))
        out["segments"] = int(len(ps.segments.count))
        out["largest_segment_leaves"] = int(ps.segments.n_leaves.max()) if len(ps.segments.count) else 0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
