"""Device time of the ray query on BASELINE config 3 (10 M planar points, Grid of 1 m voxels, subdivide(len > 64),
map_leaf_points_cuda_ransac with H = 1024, k = 6, thr = 0.01, incl. apply_mask).  The rays go from one sensor origin
(the centre of the scene) to every point of a second scan of the same scene, max_range = the measured range - the
free-space check of a registered scan - shuffled, and in the order a rotating LiDAR delivers them
(synthetic.sweep_order).  Arms alternated in one process, medians with min - max:

  raycast cube / plane   kernel time of octl_forest_raycast_device from the library's hipEvent timers (rays in HBM
                         already, the block index / the pooled planes of the selection exist)
  nearest k = 1          kernel time of octl_forest_nearest_device, r = 0.05, on the rays' end points: the project's
                         other walk that leaves the query's own leaf
  locate                 kernel time of octl_forest_locate_device on the end points: one walk to one leaf
                         - and the ratios of the ray query to both

Prints one JSON object.

    python tools/raycast_timing.py [--n 10000000] [--rays 1000000 100000] [--rounds 7]
"""

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SURFACES = ("cube", "plane")


def _stat(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--rays", type=int, nargs="+", default=[1_000_000, 100_000])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--k-split", type=int, default=64)
    ap.add_argument("--side", type=int, default=32, help="voxels per axis of the scene")
    args = ap.parse_args()

    from octreelib_amd import MaxPoints, normalize_directions, synthetic
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig

    box = (args.side,) * 3
    P = synthetic.planar_cloud(args.n, box, seed=1)
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
    f.leaf_planes(None)

    def timed(fn, prefixes):
        """kernel microseconds by timer name (those starting with one of `prefixes`)"""
        ctx.set_profiling(1)
        fn()
        ctx.sync()
        t = ctx.timings()
        ctx.set_profiling(0)
        return sum(ms * 1e3 for k, (ms, _) in t.items() if k.startswith(prefixes))

    out = {"config": "config3", "n": args.n, "map_points": int(f.n_ord), "nodes": int(len(f.nodes["edge"])),
           "blocks": int(len(f.blocks["node"])), "rounds": args.rounds, "rays": {}}
    sensor = np.full(3, args.side / 2.0) + np.array([0.37, 0.21, 0.13])

    for nr in args.rays:
        scan = synthetic.planar_cloud(nr, box, seed=1, stream=1)
        orders = {"shuffled": scan, "sweep": synthetic.sweep_order(scan, seed=2)}
        bufs = []

        def dev(nbytes):
            p = C.c_void_p()
            ctx.check(lib.octl_dev_alloc(ctx.handle, int(nbytes), C.byref(p)))
            bufs.append(p)
            return p

        d_o, d_d, d_a, d_b, d_end = dev(24 * nr), dev(24 * nr), dev(8 * nr), dev(8 * nr), dev(24 * nr)
        d_node, d_t, d_row = dev(4 * nr), dev(8 * nr), dev(4 * nr)
        d_slot, d_idx, d_d2, d_cnt = dev(4 * nr), dev(8 * nr), dev(8 * nr), dev(4 * nr)
        res = {}
        for order, Q in orders.items():
            v = Q - sensor
            rng_ = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            O = np.ascontiguousarray(np.broadcast_to(sensor, Q.shape))
            D = normalize_directions(v)
            for p, a in ((d_o, O), (d_d, D), (d_a, np.zeros(nr)), (d_b, np.ascontiguousarray(rng_)),
                         (d_end, np.ascontiguousarray(Q))):
                ctx.check(lib.octl_dev_upload(ctx.handle, p, nat.ptr(a), a.nbytes))
            cast = {s: (lambda s=s: f.raycast_device(d_o, d_d, d_a, d_b, nr, d_node, d_t, d_row, None, s))
                    for s in SURFACES}
            near = lambda: f.nearest_device(d_end, nr, 1, 0.05, d_slot, d_idx, d_d2, d_cnt)
            loc = lambda: f.locate_device(d_end, nr, d_node)
            for fn in (*cast.values(), near, loc):          # (warm: voxel codes, the index, the planes)
                fn()
            ctx.sync()
            t_loc, t_near, t_ray = [], [], {s: [] for s in SURFACES}
            for _ in range(args.rounds):                     # arms alternated
                t_loc.append(timed(loc, ("locate",)))
                t_near.append(timed(near, ("nearest_",)))
                for s in SURFACES:
                    t_ray[s].append(timed(cast[s], ("raycast_",)))
            rr = {"locate_kernel_us": _stat(t_loc), "nearest_k1_r0.05_kernel_us": _stat(t_near),
                  "median_range_m": round(float(np.median(rng_)), 2)}
            for s in SURFACES:
                cast[s]()
                node, t = np.empty(nr, dtype=np.int32), np.empty(nr)
                ctx.check(lib.octl_dev_download(ctx.handle, nat.ptr(node), d_node, node.nbytes))
                ctx.check(lib.octl_dev_download(ctx.handle, nat.ptr(t), d_t, t.nbytes))
                med = statistics.median(t_ray[s])
                hit = node >= 0
                rr[f"raycast_{s}"] = {"kernel_us": _stat(t_ray[s]), "ns_per_ray": round(med * 1e3 / nr, 2),
                                      "ratio_to_locate": round(med / statistics.median(t_loc), 2),
                                      "ratio_to_nearest_k1": round(med / statistics.median(t_near), 2),
                                      "hit_share": round(float(hit.mean()), 4),
                                      "median_hit_t_over_range": round(float(np.median(t[hit] / rng_[hit])), 4)
                                      if hit.any() else None}
            res[order] = rr
        for p in bufs:
            lib.octl_dev_free(ctx.handle, p)
        out["rays"][str(nr)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
