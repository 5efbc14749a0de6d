"""Times of prune() on an MI355X: DESIGN.md 4.18's tables.  hipEvent times of the call's two timed regions (the library's
timers "prune_mark": fill, mark, flags, scan; "prune_nodes": node pass, block pass) and wall times from Python, arms
alternated in one process, median (min - max) of --calls after a warm-up.

  half     BASELINE config 3's scene (planar points, Grid of 1 m voxels, subdivide(len > 64), RANSAC with H = 1024,
           k = 6, thr = 0.01, incl. apply_mask) as two poses that hold alternate voxels; the second pose removed, so half
           of the voxels are empty: prune alone, and a plain device copy of the bytes the node pass reads and writes
           (torch, when it is there).
  window   a window of 16 poses of 100 k points driven --steps steps along a line, one voxel per step (remove_poses of
           the oldest, a late pose, RANSAC + apply_mask): one map pruned every step, its twin never.  At the end, on the
           pruned map against the unpruned one: ray_evidence of 100 k rays and map_leaf_points_cuda_ransac; and prune
           against the only alternative without it - a fresh Grid, the window inserted again, subdivide, RANSAC,
           apply_mask.

Prints one JSON object.

    python tools/prune_timing.py [--n 10000000] [--calls 7] [--steps 64] [--no-window]
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stat(v, digits=1):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits),
            "max": round(max(v), digits)} if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--k-split", type=int, default=64)
    ap.add_argument("--no-window", action="store_true", help="the half-emptied scene only")
    args = ap.parse_args()

    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd import _native as nat
    from octreelib_amd.feed import DeviceCloud
    from octreelib_amd.grid import Grid, GridConfig

    np.random.seed(0)
    table = np.random.random((1024, 6))
    ctx = nat.get_context()

    def fit(g, subdivide=True):
        if subdivide:
            g.subdivide([MaxPoints(args.k_split)])
        f = g._forest
        f.ransac_all(10, table, 0.01)
        f.apply_device_mask()
        return f.n_ord               # (books the compaction's counts: the host has waited)

    def timed_prune(g):
        """(hipEvent us of the two regions, wall ms, PruneResult)"""
        g._forest.ensure_built()
        ctx.sync()
        ctx.set_profiling(1)
        t0 = time.perf_counter()
        res = g.prune()
        wall = (time.perf_counter() - t0) * 1e3
        ctx.sync()
        t = ctx.timings()
        ctx.set_profiling(0)
        return t["prune_mark"][0] * 1e3, t.get("prune_nodes", (0.0,))[0] * 1e3, wall, res

    def wall_ms(fn):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3

    out = {"n": args.n, "calls": args.calls}

    # ---- half of config 3's voxels emptied ----------------------------------------------------------------------
    side = 32 if args.n >= 1_000_000 else 8
    V = side ** 3
    lin = np.arange(V)
    parity = (lin // (side * side) + (lin // side) % side + lin % side) % 2       # a checkerboard
    A = synthetic.planar_cloud(args.n // 2, (side, side, side), seed=1, voxels=lin[parity == 0])
    B = synthetic.planar_cloud(args.n // 2, (side, side, side), seed=1, stream=1, voxels=lin[parity == 1])
    mark, nodes, wall, res = [], [], [], None
    for i in range(args.calls + 1):
        g = Grid(GridConfig(voxel_edge_length=1))
        g.insert_points(0, A)
        g.insert_points(1, B)
        fit(g)
        g.remove_poses([1])
        a, b, w, res = timed_prune(g)
        if i:                                                   # (the first round sizes the buffers)
            mark.append(a), nodes.append(b), wall.append(w)
        g._forest.close()
    row = 3 * 4 + 6 * 4 + 32                                    # a node's columns
    moved = res.nodes_dropped + res.n_nodes, res.n_nodes
    half = {"nodes_before": moved[0], "nodes_after": res.n_nodes, "voxels_dropped": res.voxels_dropped,
            "collapsed": res.collapsed, "mark_flags_scan_us": _stat(mark), "node_and_block_pass_us": _stat(nodes),
            "prune_wall_ms": _stat(wall, 3)}
    try:
        import torch

        nbytes = moved[0] * (row + 12) + moved[1] * row         # read: the row, occ, keep, new id; written: the kept rows
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        copy = []
        for i in range(args.calls + 1):
            ev[0].record()
            dst.copy_(src)
            ev[1].record()
            torch.cuda.synchronize()
            if i:
                copy.append(ev[0].elapsed_time(ev[1]) * 1e3)
        half["plain_copy_same_bytes_us"] = _stat(copy)
        half["copy_bytes"] = nbytes
    except Exception as e:   # noqa: BLE001 (no torch, or no device through it: the figure is left out)
        half["plain_copy_same_bytes_us"] = f"not measured: {type(e).__name__}"
    out["half"] = half

    # ---- the window along a line --------------------------------------------------------------------------------
    if not args.no_window:
        W, m = 16, 100_000
        total = W + args.steps
        dims = (total + 8, 8, 4)
        clouds = [DeviceCloud(np.ascontiguousarray(synthetic.planar_cloud(
            m, dims, seed=2, stream=k, box=((k, 0, 0), (k + 8, 8, 4))))) for k in range(total)]
        ctx.sync()
        P, U = (Grid(GridConfig(voxel_edge_length=1)) for _ in range(2))
        for g in (P, U):
            for k in range(W):
                g.insert_points(k, clouds[k])
            fit(g)
        prune_us, prune_wall = [], []
        for s in range(args.steps):
            for g in (P, U):
                g.remove_poses([s])
                g.insert_points(W + s, clouds[W + s])
                fit(g, subdivide=False)
            a, b, w, res = timed_prune(P)
            prune_us.append(a + b), prune_wall.append(w)
        rng = np.random.default_rng(3)
        n_rays = 100_000
        centre = np.array([args.steps + 12.0, 4.0, 2.0])
        O = centre + rng.uniform(-0.5, 0.5, (n_rays, 3))
        D = rng.normal(size=(n_rays, 3))
        R = rng.uniform(1.0, 8.0, n_rays)
        ev = {"pruned": [], "unpruned": []}
        rs = {"pruned": [], "unpruned": []}
        for i in range(args.calls + 1):
            for name, g in (("pruned", P), ("unpruned", U)):
                t = wall_ms(lambda: g.ray_evidence(O, D, R, 0.05))
                f = g._forest
                r = wall_ms(lambda: (f.ransac_all(10, table, 0.01), f.apply_device_mask(), f.n_ord))
                if i:
                    ev[name].append(t), rs[name].append(r)
        rebuild = []
        for i in range(args.calls + 1):
            def again():
                b = Grid(GridConfig(voxel_edge_length=1))
                for k in range(args.steps, total):
                    b.insert_points(k, clouds[k])
                fit(b)
                b._forest.close()
            t = wall_ms(again)
            if i:
                rebuild.append(t)
        fp, fu = P._forest, U._forest
        out["window"] = {
            "poses": W, "points_per_pose": m, "steps": args.steps,
            "nodes": {"pruned": fp.n_scheme_nodes(), "unpruned": fu.n_scheme_nodes()},
            "voxels": {"pruned": len(fp.voxels), "unpruned": len(fu.voxels)},
            "prune_device_us_last_calls": _stat(prune_us[-args.calls:]),
            "prune_wall_ms_last_calls": _stat(prune_wall[-args.calls:], 3),
            "ray_evidence_100k_ms": {k: _stat(v, 3) for k, v in ev.items()},
            "ransac_apply_mask_ms": {k: _stat(v, 3) for k, v in rs.items()},
            "rebuild_ms": _stat(rebuild, 2),
            "rebuild_over_prune": round(statistics.median(rebuild) / statistics.median(prune_wall[-args.calls:]), 1)}
        for g in (P, U):
            g._forest.close()
        for c in clouds:
            c.release()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
