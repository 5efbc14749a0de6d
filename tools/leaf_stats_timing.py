"""Device time of per-leaf statistics (octl_forest_leaf_stats) on BASELINE config 3 (10 M planar points, Grid of 1 m
voxels, subdivide(len > 64), map_leaf_points_cuda_ransac with H = 1024, k = 6, thr = 0.01, incl. apply_mask), against
the host loop it replaces (get_leaf_points, then mean / np.cov / eigh leaf by leaf) on a sample of the leaves.

  kernels_us    the kernels of one leaf_stats call over every block of the pose, from the library's hipEvent timers
                (leaf_moments, leaf_chunks when a block can exceed the chunk size, leaf_eigen), median over --rounds
  call_us       wall time of Forest.leaf_stats (upload of the ids, kernels, download of 176 B per block)
  host_loop     the Python / NumPy loop per leaf on --sample leaves, extrapolated to all of them

Prints one JSON object.

    python tools/leaf_stats_timing.py [--rounds 20] [--n 10000000] [--sample 2000]
    python tools/leaf_stats_timing.py --profile     # leaf_stats calls only, for rocprofv3 --kernel-trace --stats
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--k-split", type=int, default=64)
    ap.add_argument("--profile", action="store_true", help="only the leaf_stats calls (no timers, no host loop)")
    args = ap.parse_args()

    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig

    P = synthetic.planar_cloud(args.n, (32, 32, 32), seed=1)
    np.random.seed(0)
    table = np.random.random((1024, 6))
    ctx = nat.get_context()
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P)
    g.subdivide([MaxPoints(args.k_split)])
    g.map_leaf_points_cuda_ransac(hypotheses=table)
    f = g._forest
    f.ensure_built()
    ids = f.slot_blocks(0)
    n_points = int(f.blocks["size"][ids].sum())
    st = f.leaf_stats(ids)   # (warm: scratch allocated)

    if args.profile:
        for _ in range(args.rounds):
            f.leaf_stats(ids)
        print(json.dumps({"profile": "done", "blocks": len(ids), "calls": args.rounds + 1}))
        return

    kernels, calls = {}, []
    for _ in range(args.rounds):
        ctx.set_profiling(1)   # (clears the timers)
        before = ctx.timings()
        t0 = time.perf_counter()
        f.leaf_stats(ids)
        calls.append((time.perf_counter() - t0) * 1e6)
        after = ctx.timings()
        ctx.set_profiling(0)
        for name, (ms, _) in after.items():
            if name.startswith("leaf_"):
                kernels.setdefault(name, []).append((ms - before.get(name, (0.0, 0))[0]) * 1e3)
    per_kernel = {k: round(statistics.median(v), 1) for k, v in kernels.items()}
    total_kernel = [sum(v[i] for v in kernels.values()) for i in range(args.rounds)]

    leaves = g.get_leaf_points(0)
    sample = leaves[: args.sample]
    t0 = time.perf_counter()
    for v in sample:
        Q = v.get_points()
        Q.mean(axis=0)
        c = np.cov(Q.T, bias=True) if len(Q) > 1 else np.zeros((3, 3))
        np.linalg.eigh(c)
    host_s = time.perf_counter() - t0
    per_leaf_us = host_s / max(1, len(sample)) * 1e6

    print(json.dumps({
        "config": "config3", "n": args.n, "points_after_ransac": n_points, "blocks": len(ids),
        "max_block": int(st.count.max()) if len(st) else 0,
        "kernels_us": per_kernel, "kernels_total_us_median": round(statistics.median(total_kernel), 1),
        "call_us_median": round(statistics.median(calls), 1), "call_us_min": round(min(calls), 1),
        "host_loop": {"leaves_timed": len(sample), "us_per_leaf": round(per_leaf_us, 2),
                      "extrapolated_s": round(per_leaf_us * len(leaves) / 1e6, 3)},
        "rounds": args.rounds,
    }))


if __name__ == "__main__":
    main()
