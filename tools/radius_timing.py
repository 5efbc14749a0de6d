"""Device time of the radius count and of radius outlier removal on BASELINE config 3 (10 M planar points, Grid of 1 m
voxels, subdivide(len > 64), map_leaf_points_cuda_ransac with H = 1024, k = 6, thr = 0.01, incl. apply_mask), for
10 M and 100 k query points (a second scan of the same scene: shuffled, and in the order a rotating LiDAR delivers it
- synthetic.sweep_order).  Arms alternated in one process, medians with min - max:

  (a) radius_count   kernel time of k_radius_count at r = 0.1 from the library's hipEvent timers (the scan is in HBM),
                     uncapped and with max_count = 8
  (b) nearest        k_nearest<1> and k_nearest<8> on the same queries and radius: the walk's floor and the old ceiling
  (c) remove_sparse  remove_sparse(0.1, 4) over the whole map: kernel time of k_sparse_mask and of the compaction, and
                     the wall time of the call (the index in place).  The call changes the map, so every round of (c)
                     and (d) runs on a map built afresh (--sparse-rounds of them)
  (d) host path      what users had: the stored points read back, nearest(k = 8) over them, the rule in NumPy (only
                     defined for min_neighbours <= 7), apply_host_mask - wall time; checked to leave as many points

Only one work mapping of k_sparse_mask is built (one wavefront per block), so there is no arm (e).  Prints one JSON
object.

    python tools/radius_timing.py [--n 10000000] [--queries 10000000 100000] [--rounds 7] [--sparse-rounds 3]
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
    ap.add_argument("--sparse-rounds", type=int, default=3, help="rounds of arms (c) and (d): a fresh map each")
    ap.add_argument("--k-split", type=int, default=64)
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--min-neighbours", type=int, default=4)
    args = ap.parse_args()

    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig

    P = synthetic.planar_cloud(args.n, (32, 32, 32), seed=1)
    np.random.seed(0)
    table = np.random.random((1024, 6))
    ctx = nat.get_context()
    lib = ctx.lib
    r, m = args.radius, args.min_neighbours

    def build():
        g = Grid(GridConfig(voxel_edge_length=1))
        g.insert_points(0, P)
        g.subdivide([MaxPoints(args.k_split)])
        g.map_leaf_points_cuda_ransac(hypotheses=table)
        g._forest.ensure_built()
        return g

    def timed(fn, prefixes):
        ctx.set_profiling(1)
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e6
        t = ctx.timings()
        ctx.set_profiling(0)
        return {k: ms * 1e3 for k, (ms, _) in t.items() if k.startswith(prefixes)}, wall

    g = build()
    f = g._forest
    out = {"config": "config3", "n": args.n, "map_points": int(f.n_ord), "rounds": args.rounds,
           "sparse_rounds": args.sparse_rounds, "radius": r, "min_neighbours": m, "queries": {}}
    for nq in args.queries:
        scan = synthetic.planar_cloud(nq, (32, 32, 32), seed=1, stream=1)
        clouds = {"shuffled": scan, "sweep": synthetic.sweep_order(scan, seed=2)}
        bufs = []

        def dev(nbytes):
            p = C.c_void_p()
            ctx.check(lib.octl_dev_alloc(ctx.handle, int(nbytes), C.byref(p)))
            bufs.append(p)
            return p

        xin, d_count = dev(24 * nq), dev(4 * nq)
        d_slot, d_index, d_d2, d_cnt8 = dev(4 * nq * 8), dev(8 * nq * 8), dev(8 * nq * 8), dev(4 * nq)
        res = {}
        for order, Q in clouds.items():
            ctx.check(lib.octl_dev_upload(ctx.handle, xin, nat.ptr(Q), Q.nbytes))
            arms = {"radius_count_uncapped": (lambda: f.radius_count_device(xin, nq, r, d_count), "radius_count"),
                    "radius_count_cap8": (lambda: f.radius_count_device(xin, nq, r, d_count, 8), "radius_count"),
                    "nearest_k1": (lambda: f.nearest_device(xin, nq, 1, r, d_slot, d_index, d_d2, d_cnt8), "nearest_k1"),
                    "nearest_k8": (lambda: f.nearest_device(xin, nq, 8, r, d_slot, d_index, d_d2, d_cnt8), "nearest_k8")}
            for fn, _ in arms.values():                   # (warm)
                fn()
            ctx.sync()
            cnt = np.empty(nq, dtype=np.int32)
            arms["radius_count_uncapped"][0]()
            ctx.check(lib.octl_dev_download(ctx.handle, nat.ptr(cnt), d_count, cnt.nbytes))
            us = {name: [] for name in arms}
            for _ in range(args.rounds):                  # arms alternated
                for name, (fn, timer) in arms.items():
                    k, _ = timed(fn, (timer,))
                    us[name].append(k[timer])
            med = {name: statistics.median(v) for name, v in us.items()}
            res[order] = {name + "_kernel_us": _stat(v) for name, v in us.items()}
            res[order].update({"cap8_over_nearest_k8": round(med["radius_count_cap8"] / med["nearest_k8"], 3),
                               "uncapped_over_nearest_k1": round(med["radius_count_uncapped"] / med["nearest_k1"], 3),
                               "mean_count": round(float(cnt.mean()), 2), "share_above_8": round(float((cnt > 8).mean()), 4)})
            print(f"queries {nq} {order}: done", file=sys.stderr, flush=True)
        for p in bufs:
            lib.octl_dev_free(ctx.handle, p)
        out["queries"][str(nq)] = res

    # (c) and (d): a fresh map each, alternated
    sparse_k, compact_k, sparse_wall, host_wall, left = [], [], [], [], set()
    for i in range(args.sparse_rounds):
        if i:
            g = build()
        f = g._forest
        g.radius_count(P[:1], r)                          # (the index of every pose is in place)
        ctx.sync()
        k, wall = timed(lambda: g.remove_sparse(r, m), ("sparse_mask", "apply_mask"))
        sparse_k.append(k["sparse_mask"])
        compact_k.append(k["apply_mask"])
        sparse_wall.append(wall)
        left.add(int(f.n_ord))
        print(f"remove_sparse round {i}: done", file=sys.stderr, flush=True)
        if m <= 7:
            g = build()
            f = g._forest
            ctx.sync()
            t0 = time.perf_counter()
            pts = f.xyz                                   # (one pose: storage order)
            nb = g.nearest(pts, 8, max_distance=r)
            f.apply_host_mask((nb.count - 1 >= m).astype(np.uint8))     # (the point itself is one of the 8)
            ctx.sync()
            host_wall.append((time.perf_counter() - t0) * 1e6)
            left.add(int(f.n_ord))
            print(f"host path round {i}: done", file=sys.stderr, flush=True)
    out["remove_sparse"] = {"sparse_mask_kernel_us": _stat(sparse_k), "compaction_kernel_us": _stat(compact_k),
                            "call_wall_us": _stat(sparse_wall), "host_path_wall_us": _stat(host_wall),
                            "points_left": sorted(left), "host_path_agrees": len(left) == 1}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
