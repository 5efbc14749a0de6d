"""Time of the multi-pose plane-adjustment system on BASELINE config 3's scene as a sliding window sees it: 8 poses of
1.25 M planar points in one Grid of 1 m voxels, subdivide(len > 64), map_leaf_points_cuda_ransac with H = 1024, k = 6,
thr = 0.01, incl. apply_mask.  Arms alternated in one process, medians with min - max:

  (a) preparation    the one-off reduction of the map to block moments and the two block orders (wall; forced by
                     alternating between two spellings of the same selection) and its kernels
  (b) system         one octl_forest_adjustment_system call on the prepared forest: k_adj_leaf / k_adj_partial /
                     k_adj_fold from the library's hipEvent timers, and wall
  (c) iteration      one adjust iteration: the call, the S 6x6 solves, the pose updates (wall)
  (d) registrations  what the library offered for the same job before: S x registration_system(get_points(p)) against
                     the planes of all poses (wall)
  (e) numpy          adjustment_system_np on the downloaded block moments (wall)

Prints one JSON object.

    python tools/adjustment_timing.py [--poses 8] [--n 1250000] [--rounds 7] [--slow-rounds 2]
"""

import argparse
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
    ap.add_argument("--poses", type=int, default=8)
    ap.add_argument("--n", type=int, default=1_250_000, help="points per pose")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--slow-rounds", type=int, default=2, help="rounds of arms (d) and (e)")
    ap.add_argument("--k-split", type=int, default=64)
    ap.add_argument("--max-variance", type=float, default=1e-3)
    args = ap.parse_args()

    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd import _native as nat
    from octreelib_amd.adjustment import adjustment_system_np
    from octreelib_amd.grid import Grid, GridConfig
    from octreelib_amd.registration import se3_exp

    S = args.poses
    np.random.seed(0)
    table = np.random.random((1024, 6))
    ctx = nat.get_context()
    g = Grid(GridConfig(voxel_edge_length=1))
    for p in range(S):
        g.insert_points(p, synthetic.planar_cloud(args.n, (32, 32, 32), seed=1, stream=p))
    g.subdivide([MaxPoints(args.k_split)])
    g.map_leaf_points_cuda_ransac(hypotheses=table)
    f = g._forest
    f.ensure_built()
    c = f.adjustment_origin()
    rng = np.random.default_rng(3)
    T = np.stack([se3_exp(np.concatenate([rng.normal(size=3) * 1e-3, rng.normal(size=3) * 5e-3]), c) for _ in range(S)])
    T[0] = np.eye(4)
    gates = dict(max_variance=args.max_variance)
    everyone = list(range(S))

    def timed(fn, prefixes):
        ctx.set_profiling(1)
        t0 = time.perf_counter()
        r = fn()
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e6
        t = ctx.timings()
        ctx.set_profiling(0)
        return {k: ms * 1e3 for k, (ms, _) in t.items() if k.startswith(prefixes)}, wall, r

    def registrations():
        g.leaf_planes()
        return [g.registration_system(g.get_points(p), T[p], origin=c, **gates) for p in range(S)]

    s = g.adjustment_system(T, origin=c, leaves=True, **gates)          # (warm; the tables for arm (e))
    blocks = s.blocks
    out = {"config": "config3 as a window", "poses": S, "points_per_pose": args.n, "map_points": int(f.n_ord),
           "blocks": len(blocks), "leaves_pooled": s.n_leaves[0], "leaves_used": s.n_leaves[1],
           "points_used": int(s.n_points.sum()), "rounds": args.rounds, "slow_rounds": args.slow_rounds}
    prep_wall, prep_k, sys_wall, k_leaf, k_part, k_fold, it_wall, reg_wall, np_wall = ([] for _ in range(9))
    launches = None
    for i in range(args.rounds):                                         # arms alternated
        # (a) the same poses under another spelling of the selection: the tables are made again
        k, wall, _ = timed(lambda: g.adjustment_system(T, pose_numbers=everyone if i % 2 == 0 else None, origin=c,
                                                       **gates), ("adj_",))
        prep_wall.append(wall)
        prep_k.append(sum(v for name, v in k.items() if name not in ("adj_leaf", "adj_partial", "adj_fold")))
        g.adjustment_system(T, pose_numbers=everyone if i % 2 == 0 else None, origin=c, **gates)
        k, _, _ = timed(lambda: g.adjustment_system(T, pose_numbers=everyone if i % 2 == 0 else None, origin=c,
                                                    **gates), ("adj_",))
        k_leaf.append(k["adj_leaf"])
        k_part.append(k["adj_partial"])
        k_fold.append(k["adj_fold"])
        sel = everyone if i % 2 == 0 else None
        a = nat_counter(nat, "octl_debug_launches")
        ctx.sync()
        t0 = time.perf_counter()
        g.adjustment_system(T, pose_numbers=sel, origin=c, **gates)
        sys_wall.append((time.perf_counter() - t0) * 1e6)
        launches = nat_counter(nat, "octl_debug_launches") - a
        t0 = time.perf_counter()
        s2 = g.adjustment_system(T, pose_numbers=sel, origin=c, **gates)
        xi = s2.solve()
        np.stack([se3_exp(xi[k2], c) @ T[k2] for k2 in range(S)])
        it_wall.append((time.perf_counter() - t0) * 1e6)
        if i < args.slow_rounds:
            ctx.sync()
            t0 = time.perf_counter()
            registrations()
            reg_wall.append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter()
            ref = adjustment_system_np(blocks, T, c, **gates)
            np_wall.append((time.perf_counter() - t0) * 1e6)
            out["numpy_agrees"] = bool(np.array_equal(ref.n_points, s.n_points)
                                       and np.allclose(ref.H, s.H, rtol=1e-9, atol=1e-9 * np.abs(s.H).max()))
    out.update({
        "preparation_wall_us": _stat(prep_wall), "preparation_kernels_us": _stat(prep_k),
        "system_wall_us": _stat(sys_wall), "adj_leaf_kernel_us": _stat(k_leaf), "adj_partial_kernel_us": _stat(k_part),
        "adj_fold_kernel_us": _stat(k_fold), "launches_per_call": int(launches),
        "adjust_iteration_wall_us": _stat(it_wall), "registrations_wall_us": _stat(reg_wall),
        "adjustment_system_np_wall_us": _stat(np_wall),
    })
    print(json.dumps(out))


def nat_counter(nat, name):
    import ctypes as C

    v = C.c_uint64(0)
    getattr(nat.load(), name)(C.byref(v))
    return v.value


if __name__ == "__main__":
    main()
