"""Device time of the ray-evidence walk on BASELINE config 3 (10 M planar points, Grid of 1 m voxels, subdivide(len >
64), map_leaf_points_cuda_ransac with H = 1024, k = 6, thr = 0.01, incl. apply_mask).  The rays go from one sensor
origin (the centre of the scene) to every point of a second scan of the same scene with their measured ranges -
shuffled, and in the order a rotating LiDAR delivers them (synthetic.sweep_order).  Arms alternated in one process,
medians with min - max:

  ray_evidence     kernel time of octl_forest_ray_evidence_device from the library's hipEvent timers (rays and
                   counters in HBM already), once with min_range = 0 and once with a blind range of --blind metres:
                   rays from one origin all cross the same leaves next to it, so the difference is what the
                   same-address atomics there cost
  raycast plane    kernel time of octl_forest_raycast_device (k_raycast<true>) on the same rays, max_range = the
                   measured range: the walk that stops at the first accepted plane
                   - and the ratio of the two

Prints one JSON object.

    python tools/evidence_timing.py [--n 10000000] [--rays 1000000 100000] [--rounds 7] [--blind 3.0]
"""

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stat(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--rays", type=int, nargs="+", default=[1_000_000, 100_000])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--k-split", type=int, default=64)
    ap.add_argument("--side", type=int, default=32, help="voxels per axis of the scene")
    ap.add_argument("--margin", type=float, default=0.05)
    ap.add_argument("--blind", type=float, default=3.0, help="the blind range of the second arm, metres")
    args = ap.parse_args()

    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig
    from octreelib_amd.query import evidence_inputs

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
    N = f.n_scheme_nodes()

    def timed(fn, prefixes):
        """kernel microseconds by timer name (those starting with one of `prefixes`)"""
        ctx.set_profiling(1)
        fn()
        ctx.sync()
        t = ctx.timings()
        ctx.set_profiling(0)
        return sum(ms * 1e3 for k, (ms, _) in t.items() if k.startswith(prefixes))

    out = {"config": "config3", "n": args.n, "map_points": int(f.n_ord), "nodes": N,
           "leaves": int((f.nodes["first_child"] < 0).sum()), "rounds": args.rounds, "margin": args.margin,
           "blind_range_m": args.blind, "rays": {}}
    sensor = np.full(3, args.side / 2.0) + np.array([0.37, 0.21, 0.13])
    zeros = np.zeros(2 * N, dtype=np.uint32)

    for nr in args.rays:
        scan = synthetic.planar_cloud(nr, box, seed=1, stream=1)
        orders = {"shuffled": scan, "sweep": synthetic.sweep_order(scan, seed=2)}
        bufs = []

        def dev(nbytes):
            p = C.c_void_p()
            ctx.check(lib.octl_dev_alloc(ctx.handle, int(nbytes), C.byref(p)))
            bufs.append(p)
            return p

        d_o, d_d, d_free, d_end = dev(24 * nr), dev(24 * nr), dev(8 * nr), dev(8 * nr)
        d_min = {"min_range_0": dev(8 * nr), "blind": dev(8 * nr)}
        d_rng, d_node, d_t, d_row = dev(8 * nr), dev(4 * nr), dev(8 * nr), dev(4 * nr)
        d_cnt = dev(8 * N)
        d_hits = C.c_void_p(d_cnt.value + 4 * N)
        res = {}
        for order, Q in orders.items():
            v = Q - sensor
            rng_ = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            O = np.ascontiguousarray(np.broadcast_to(sensor, Q.shape))
            o, d, tmin, tfree, tend = evidence_inputs(O, v, rng_, args.margin)
            for p, a in ((d_o, o), (d_d, d), (d_free, tfree), (d_end, tend), (d_min["min_range_0"], tmin),
                         (d_min["blind"], np.full(nr, args.blind)), (d_rng, np.ascontiguousarray(rng_))):
                ctx.check(lib.octl_dev_upload(ctx.handle, p, nat.ptr(a), a.nbytes))
            arms = {k: (lambda k=k: f.ray_evidence_device(d_o, d_d, d_min[k], d_free, d_end, nr, d_cnt, d_hits, N))
                    for k in d_min}
            cast = lambda: f.raycast_device(d_o, d_d, d_min["min_range_0"], d_rng, nr, d_node, d_t, d_row, None, "plane")
            for fn in (*arms.values(), cast):          # (warm: voxel codes, the planes)
                fn()
            ctx.sync()
            t_cast, t_ev = [], {k: [] for k in arms}
            for _ in range(args.rounds):               # arms alternated
                t_cast.append(timed(cast, ("raycast_",)))
                for k, fn in arms.items():
                    t_ev[k].append(timed(fn, ("ray_evidence",)))
            rr = {"raycast_plane_kernel_us": _stat(t_cast), "median_range_m": round(float(np.median(rng_)), 2)}
            for k, fn in arms.items():
                ctx.check(lib.octl_dev_upload(ctx.handle, d_cnt, nat.ptr(zeros), zeros.nbytes))
                fn()
                cnt = np.empty(2 * N, dtype=np.uint32)
                ctx.check(lib.octl_dev_download(ctx.handle, nat.ptr(cnt), d_cnt, cnt.nbytes))
                through, hits = cnt[:N].astype(np.int64), cnt[N:].astype(np.int64)
                med = statistics.median(t_ev[k])
                rr[f"ray_evidence_{k}"] = {"kernel_us": _stat(t_ev[k]), "ns_per_ray": round(med * 1e3 / nr, 2),
                                           "ratio_to_raycast_plane": round(med / statistics.median(t_cast), 2),
                                           "atomics_per_ray": round(float(through.sum() + hits.sum()) / nr, 2),
                                           "largest_counter": int(max(through.max(), hits.max())),
                                           "leaves_free_2_0": int(((through >= 2) & (hits == 0)).sum())}
            res[order] = rr
        for p in bufs:
            lib.octl_dev_free(ctx.handle, p)
        out["rays"][str(nr)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
