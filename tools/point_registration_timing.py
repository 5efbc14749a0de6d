"""Device time of the point-to-point registration normal equations on BASELINE config 3 (10 M planar points, Grid of
1 m voxels, subdivide(len > 64), map_leaf_points_cuda_ransac with H = 1024, k = 6, thr = 0.01, incl. apply_mask), for
10 M and 100 k query points (a second scan of the same scene under a small motion: shuffled, and in the order a
rotating LiDAR delivers it - synthetic.sweep_order).  Arms alternated in one process, medians with min - max:

  (a) point registration  kernel time of k_reg_match / k_regp_partial / k_reg_fold from the library's hipEvent timers
                          (the scan is in HBM), and the wall time of one align_points iteration on the resident scan
                          (device form, the 240-byte download, the 6x6 solve, the pose update)
  (b) host_formation      what the library offered for the same job before: the scan transformed on the host, uploaded,
                          octl_forest_nearest_device with k = 1, its four downloads, the matched points looked up and H,
                          g formed in NumPy - wall time, and the share of the kernel in it
  (c) floor               the kernel of octl_forest_nearest_device (k_nearest<1>) alone, on the transformed scan

Prints one JSON object.

    python tools/point_registration_timing.py [--n 10000000] [--queries 10000000 100000] [--rounds 7] [--host-rounds 3]
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
    ap.add_argument("--host-rounds", type=int, default=3, help="rounds of arm (b), whose NumPy part is slow at 10 M")
    ap.add_argument("--k-split", type=int, default=64)
    ap.add_argument("--max-distance", type=float, default=0.1)
    args = ap.parse_args()

    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig
    from octreelib_amd.registration import default_origin, se3_exp, system_from_sums, transform_np

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
    md = args.max_distance

    def timed(fn, prefixes):
        ctx.set_profiling(1)
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e6
        t = ctx.timings()
        ctx.set_profiling(0)
        return {k: ms * 1e3 for k, (ms, _) in t.items() if k.startswith(prefixes)}, wall

    out = {"config": "config3", "n": args.n, "map_points": int(f.n_ord), "rounds": args.rounds,
           "host_rounds": args.host_rounds, "max_distance": md, "queries": {}}
    # the scan was taken 0.5 degrees and a few centimetres away from where the map has it
    T = se3_exp([0.004, -0.005, 0.006, 0.03, -0.02, 0.01], [16.0, 16.0, 16.0])
    for nq in args.queries:
        scan = synthetic.planar_cloud(nq, (32, 32, 32), seed=1, stream=1)
        scan = transform_np(np.linalg.inv(T), scan)
        clouds = {"shuffled": scan, "sweep": synthetic.sweep_order(scan, seed=2)}
        res = {}
        bufs = []

        def dev(nbytes):
            p = C.c_void_p()
            ctx.check(lib.octl_dev_alloc(ctx.handle, int(nbytes), C.byref(p)))
            bufs.append(p)
            return p

        xin, xt, d_out = dev(24 * nq), dev(24 * nq), dev(256)
        d_slot, d_index, d_d2, d_count = dev(4 * nq), dev(8 * nq), dev(8 * nq), dev(4 * nq)
        d_counts = C.c_void_p(d_out.value + 28 * 8)
        slot, index = np.empty(nq, np.int32), np.empty(nq, np.int64)
        d2, count = np.empty(nq, np.float64), np.empty(nq, np.int32)
        buf = np.empty(30, dtype=np.float64)
        for order, Q in clouds.items():
            c = default_origin(T, Q)
            ctx.check(lib.octl_dev_upload(ctx.handle, xin, nat.ptr(Q), Q.nbytes))

            def reg():
                f.point_registration_system_device(xin, nq, T, c, d_out, d_counts, md)

            def iteration():
                reg()
                ctx.check(lib.octl_dev_download(ctx.handle, nat.ptr(buf), d_out, buf.nbytes))
                s = system_from_sums(buf[:28].copy(), buf[28:].view(np.int64), c)
                return s, se3_exp(s.solve(), c) @ T

            def floor_kernel():
                f.nearest_device(xt, nq, 1, md, d_slot, d_index, d_d2, d_count)

            def host_formation():
                p = transform_np(T, Q)
                ctx.check(lib.octl_dev_upload(ctx.handle, xt, nat.ptr(p), p.nbytes))
                floor_kernel()
                for a, d in ((slot, d_slot), (index, d_index), (d2, d_d2), (count, d_count)):
                    ctx.check(lib.octl_dev_download(ctx.handle, nat.ptr(a), d, a.nbytes))
                used = count > 0
                e = p[used] - P[index[used]]
                d = p[used] - c
                sd = d.sum(axis=0)
                H = np.zeros((6, 6))
                H[:3, :3] = (d * d).sum() * np.eye(3) - d.T @ d
                H[:3, 3:] = [[0.0, -sd[2], sd[1]], [sd[2], 0.0, -sd[0]], [-sd[1], sd[0], 0.0]]
                H[3:, :3] = H[:3, 3:].T
                H[3:, 3:] = len(d) * np.eye(3)
                return H, np.concatenate([np.cross(d, e).sum(axis=0), e.sum(axis=0)]), int(used.sum())

            s, _ = iteration()                            # (warm)
            Hh, gh, nu = host_formation()                 # (warm; leaves the transformed scan in xt for the floor arm)
            agrees = bool(nu == s.n_used and np.allclose(Hh, s.H, rtol=1e-9, atol=1e-9 * np.abs(s.H).max())
                          and np.allclose(gh, s.g, rtol=1e-9, atol=1e-9 * np.abs(s.g).max()))
            match, part, fold, it_wall, floor, hf_wall, hf_kernel = [], [], [], [], [], [], []
            for i in range(args.rounds):                  # arms alternated
                k, _ = timed(reg, ("reg_", "regp_"))
                match.append(k["reg_match"])
                part.append(k["regp_partial"])
                fold.append(k["reg_fold"])
                k, _ = timed(floor_kernel, ("nearest_k1",))
                floor.append(k["nearest_k1"])
                ctx.sync()
                t0 = time.perf_counter()
                iteration()
                it_wall.append((time.perf_counter() - t0) * 1e6)
                if i < args.host_rounds:
                    k, wall = timed(host_formation, ("nearest_k1",))
                    hf_wall.append(wall)
                    hf_kernel.append(k["nearest_k1"])
            kernels = statistics.median(match) + statistics.median(part) + statistics.median(fold)
            res[order] = {
                "reg_match_kernel_us": _stat(match), "regp_partial_kernel_us": _stat(part),
                "reg_fold_kernel_us": _stat(fold), "align_points_iteration_wall_us": _stat(it_wall),
                "floor_nearest_k1_kernel_us": _stat(floor),
                "kernels_over_floor": round(kernels / statistics.median(floor), 3),
                "match_over_floor": round(statistics.median(match) / statistics.median(floor), 3),
                "host_formation_wall_us": _stat(hf_wall), "host_formation_kernel_us": _stat(hf_kernel),
                "host_formation_agrees": agrees, "used_share": round(s.n_used / nq, 4),
                "located_share": round(s.n_located / nq, 4),
            }
        for p in bufs:
            lib.octl_dev_free(ctx.handle, p)
        out["queries"][str(nq)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
