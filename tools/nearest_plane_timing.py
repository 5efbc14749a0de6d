"""Device time of the nearest-point-to-plane registration normal equations on BASELINE config 3 (10 M planar points,
Grid of 1 m voxels, subdivide(len > 64), map_leaf_points_cuda_ransac with H = 1024, k = 6, thr = 0.01, incl.
apply_mask), for 100 k and 10 M query points (a second scan of the same scene under a small motion, shuffled).  Arms
alternated in one process, hipEvent kernel times from the library's timers, medians with min - max:

  (a) nearest_plane  k_regn_match + k_regn_partial + k_reg_fold   octl_forest_nearest_plane_registration_system_device
  (b) point          k_reg_match + k_regp_partial + k_reg_fold    octl_forest_point_registration_system_device, same radius
  (c) own_leaf       k_reg_partial + k_reg_fold                   octl_forest_registration_system_device

and, for the known small motion on the smallest scan, the iterations and the wall time to convergence of
align_nearest_planes, align_points and align (scan resident, planes and index made before the clock starts).

Prints one JSON object.

    python tools/nearest_plane_timing.py [--n 10000000] [--queries 100000 10000000] [--rounds 7]
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
    ap.add_argument("--queries", type=int, nargs="+", default=[100_000, 10_000_000])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--k-split", type=int, default=64)
    ap.add_argument("--max-distance", type=float, default=0.1)
    args = ap.parse_args()

    from octreelib_amd import MaxPoints, align_nearest_planes, synthetic
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig
    from octreelib_amd.registration import default_origin, se3_exp, transform_np

    P = synthetic.planar_cloud(args.n, (32, 32, 32), seed=1)
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
    planes = g.leaf_planes()
    md = args.max_distance

    def timed(fn, prefixes):
        ctx.set_profiling(1)
        fn()
        ctx.sync()
        t = ctx.timings()
        ctx.set_profiling(0)
        return {k: ms * 1e3 for k, (ms, _) in t.items() if k.startswith(prefixes)}

    out = {"config": "config3", "n": args.n, "map_points": int(f.n_ord), "leaf_planes": int(len(planes)),
           "rounds": args.rounds, "max_distance": md, "queries": {}}
    # the scan was taken 0.5 degrees and a few centimetres away from where the map has it
    T = se3_exp([0.004, -0.005, 0.006, 0.03, -0.02, 0.01], [16.0, 16.0, 16.0])
    for nq in args.queries:
        Q = transform_np(np.linalg.inv(T), synthetic.planar_cloud(nq, (32, 32, 32), seed=1, stream=1))
        c = default_origin(T, Q)
        bufs = []

        def dev(nbytes):
            p = C.c_void_p()
            ctx.check(lib.octl_dev_alloc(ctx.handle, int(nbytes), C.byref(p)))
            bufs.append(p)
            return p

        xin, d_out = dev(24 * nq), dev(256)
        d_counts = C.c_void_p(d_out.value + 28 * 8)
        ctx.check(lib.octl_dev_upload(ctx.handle, xin, nat.ptr(Q), Q.nbytes))
        counts = np.empty(2, dtype=np.int64)
        arms = {
            "nearest_plane": (lambda: f.nearest_plane_registration_system_device(xin, nq, T, c, d_out, d_counts, md),
                              ("regn_match", "regn_partial", "reg_fold")),
            "point": (lambda: f.point_registration_system_device(xin, nq, T, c, d_out, d_counts, md),
                      ("reg_match", "regp_partial", "reg_fold")),
            "own_leaf": (lambda: f.registration_system_device(xin, nq, T, c, d_out, d_counts),
                         ("reg_partial", "reg_fold")),
        }
        res = {}
        times = {name: {k: [] for k in keys} for name, (_, keys) in arms.items()}
        for name, (fn, _) in arms.items():                # (warm, and the shares each system uses)
            fn()
            ctx.check(lib.octl_dev_download(ctx.handle, nat.ptr(counts), d_counts, 16))
            res[name] = {"used_share": round(int(counts[0]) / nq, 4), "located_share": round(int(counts[1]) / nq, 4)}
        for _ in range(args.rounds):                      # arms alternated
            for name, (fn, keys) in arms.items():
                k = timed(fn, ("reg_", "regn_", "regp_"))
                for key in keys:
                    times[name][key].append(k[key])
        for name, (_, keys) in arms.items():
            for key in keys:
                res[name][f"{key}_kernel_us"] = _stat(times[name][key])
            res[name]["system_kernels_us"] = round(sum(statistics.median(times[name][key]) for key in keys), 1)
        for p in bufs:
            lib.octl_dev_free(ctx.handle, p)
        out["queries"][str(nq)] = res

    # alignment to convergence from the identity, smallest scan
    nq = min(args.queries)
    Q = transform_np(np.linalg.inv(T), synthetic.planar_cloud(nq, (32, 32, 32), seed=1, stream=1))
    g.nearest(Q[:16], 1, max_distance=md)
    runs = {"align_nearest_planes": lambda: align_nearest_planes(g, Q, max_distance=md),
            "align_points": lambda: g.align_points(Q, max_distance=md),
            "align": lambda: g.align(Q)}
    al = {}
    for name, fn in runs.items():
        fn()                                              # (warm)
        walls, a = [], None
        for _ in range(args.rounds):
            ctx.sync()
            t0 = time.perf_counter()
            a = fn()
            walls.append((time.perf_counter() - t0) * 1e6)
        al[name] = {"iterations": a.iterations, "converged": bool(a.converged), "reason": a.reason,
                    "n_used": int(a.n_used), "error": float(np.abs(a.transform - T).max()), "wall_us": _stat(walls)}
    out["alignment"] = {"queries": nq, "runs": al}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
