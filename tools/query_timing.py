"""Device time of the map queries on BASELINE config 3 (10 M planar points, Grid of 1 m voxels, subdivide(len > 64),
map_leaf_points_cuda_ransac with H = 1024, k = 6, thr = 0.01, incl. apply_mask), for 10 M and 100 k query points (a
second scan of the same scene: shuffled, and in the order a rotating LiDAR delivers it - synthetic.sweep_order).
Side by side, arms alternated in one process, medians with min - max:

  locate / point_to_plane   kernel time of octl_forest_locate_device / octl_forest_point_to_plane_device from the
                            library's hipEvent timers (the points are in HBM already), and the achieved design traffic
                            (24 B read + 4 B, resp. 16 B, written per query) over that time
  pooled_planes             the kernels of one octl_forest_pooled_leaf_stats over the map (grouping, moments, eigen)
  insert_late_pose          the only device way to the same answer before this feature: the same points inserted as a
                            late pose (Grid.insert_points after subdivide: incremental.hip) - kernels (inc_*) and wall
                            time of the build call; the map is rebuilt before every round because the insertion changes it
  locate_np                 the host definition on the downloaded tables

Prints one JSON object.

    python tools/query_timing.py [--n 10000000] [--rounds 7] [--insert-rounds 3] [--host-max 10000000]
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
    ap.add_argument("--queries", type=int, nargs="+", default=[10_000_000, 100_000])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--insert-rounds", type=int, default=3)
    ap.add_argument("--host-max", type=int, default=10_000_000, help="largest query count locate_np is timed on")
    ap.add_argument("--k-split", type=int, default=64)
    args = ap.parse_args()

    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig
    from octreelib_amd.query import locate_np

    P = synthetic.planar_cloud(args.n, (32, 32, 32), seed=1)
    np.random.seed(0)
    table = np.random.random((1024, 6))
    ctx = nat.get_context()
    lib = ctx.lib

    def build_map():
        g = Grid(GridConfig(voxel_edge_length=1))
        g.insert_points(0, P)
        g.subdivide([MaxPoints(args.k_split)])
        g.map_leaf_points_cuda_ransac(hypotheses=table)
        g._forest.ensure_built()
        g._forest.n_ord   # (books the compaction's counts)
        return g

    def timed(fn, prefixes):
        """kernel microseconds by timer name (those starting with one of `prefixes`) and wall microseconds of fn()"""
        ctx.set_profiling(1)
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e6
        t = ctx.timings()
        ctx.set_profiling(0)
        return {k: ms * 1e3 for k, (ms, _) in t.items() if k.startswith(prefixes)}, wall

    g = build_map()
    f = g._forest
    planes = g.leaf_planes()
    out = {"config": "config3", "n": args.n, "map_points": int(f.n_ord), "nodes": int(len(f.nodes["edge"])),
           "leaves_with_planes": len(planes), "rounds": args.rounds, "queries": {}}

    pooled = []
    for i in range(args.rounds):
        # (the map holds one pose: "pose 0" and "all poses" are the same planes but another selection, so that the
        #  library computes the table again instead of handing out the one it has)
        sel = [0] if i % 2 == 0 else None
        k, _ = timed(lambda: f.leaf_planes(sel), ("pool_",))   # (pool_group covers its sort and scan)
        pooled.append(sum(k.values()))
    out["pooled_planes_kernels_us"] = _stat(pooled)
    g.leaf_planes()

    for nq in args.queries:
        scan = synthetic.planar_cloud(nq, (32, 32, 32), seed=1, stream=1)
        clouds = {"shuffled": scan, "sweep": synthetic.sweep_order(scan, seed=2)}
        res = {}
        bufs = []

        def dev(nbytes):
            p = C.c_void_p()
            ctx.check(lib.octl_dev_alloc(ctx.handle, int(nbytes), C.byref(p)))
            bufs.append(p)
            return p

        xin, d_node, d_row, d_dist = dev(24 * nq), dev(4 * nq), dev(4 * nq), dev(8 * nq)
        for order, Q in clouds.items():
            ctx.check(lib.octl_dev_upload(ctx.handle, xin, nat.ptr(Q), Q.nbytes))
            f.locate_device(xin, nq, d_node)            # (warm)
            f.point_to_plane_device(xin, nq, d_node, d_row, d_dist)
            ctx.sync()
            loc, p2p = [], []
            for _ in range(args.rounds):                 # arms alternated
                k, _ = timed(lambda: f.locate_device(xin, nq, d_node), ("locate",))
                loc.append(k["locate"])
                k, _ = timed(lambda: f.point_to_plane_device(xin, nq, d_node, d_row, d_dist), ("point_to_plane",))
                p2p.append(k["point_to_plane"])
            r = {"locate_kernel_us": _stat(loc), "point_to_plane_kernel_us": _stat(p2p),
                 "locate_design_GBps": round(28.0 * nq / statistics.median(loc) / 1e3, 1),
                 "point_to_plane_design_GBps": round(40.0 * nq / statistics.median(p2p) / 1e3, 1)}
            node = np.empty(nq, dtype=np.int32)
            ctx.check(lib.octl_dev_download(ctx.handle, nat.ptr(node), d_node, node.nbytes))
            r["located_share"] = round(float((node >= 0).mean()), 4)
            if nq <= args.host_max:
                nodes, voxels = f.nodes, f.voxels
                t0 = time.perf_counter()
                ref = locate_np(nodes, voxels, 0, 1.0, Q)
                r["locate_np_s"] = round(time.perf_counter() - t0, 3)
                r["locate_np_equal"] = bool(np.array_equal(ref, node))
            res[order] = r
        for p in bufs:
            lib.octl_dev_free(ctx.handle, p)
        # the same points as a late pose (shuffled order), on a map rebuilt for every round
        ins_k, ins_wall = [], []
        for i in range(args.insert_rounds):
            g2 = build_map()
            f2 = g2._forest
            g2.insert_points(1, clouds["shuffled"])
            k, wall = timed(lambda: f2.ensure_built(), ("inc_",))   # (inc_sort covers the radix sort's passes)
            ins_k.append(sum(k.values()))
            ins_wall.append(wall)
            parts = {name: round(v, 1) for name, v in k.items()}
            f2.close()
        res["insert_late_pose"] = {"kernels_us": _stat(ins_k), "build_call_wall_us": _stat(ins_wall),
                                   "kernels_last_round_us": parts, "rounds": args.insert_rounds}
        out["queries"][str(nq)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
