"""Device time of Euclidean cluster extraction on the window of tools/thin_timing.py: 16 poses of 100 k points each, every
pose another draw of the SAME planar scene (8 x 8 x 4 voxels of 1 m), Grid of 1 m voxels, subdivide(len > 64) - as
inserted and after thin(map, L/8) - at radius L/8 and L/32.  Per map and radius, medians with min - max of alternated
rounds from the library's hipEvent timers:

  (a) cluster        kernel times of k_cluster_init / _link / _flatten / _rows of cluster(map, radius), wall time of the
                     call (the index in place), clusters and the largest one
  (b) yardstick      k_sparse_mask of remove_sparse(radius, 2^31 - 1) on the same map: the same walk over the same
                     candidates with a counting sink that never saturates (it empties the map: every round builds anew)
  (c) definition     wall time of cluster_labels_np over the rows still in the map (maps of at most --definition-max points),
                     and whether the device's labels equal it

No pass/fail threshold.  Prints one JSON object.

    python tools/cluster_timing.py [--poses 16] [--points 100000] [--rounds 5]
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = ("cluster_init", "cluster_link", "cluster_flatten", "cluster_rows")


def _stat(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--k-split", type=int, default=64)
    ap.add_argument("--definition-max", type=int, default=400_000)
    args = ap.parse_args()

    from octreelib_amd import MaxPoints, cluster, cluster_labels_np, synthetic, thin
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig

    dims, L = (8, 8, 4), 1.0
    clouds = [synthetic.planar_cloud(args.points, dims, seed=1, stream=p) for p in range(args.poses)]
    ctx = nat.get_context()
    radii = {"L/8": L / 8, "L/32": L / 32}

    def build(thinned):
        g = Grid(GridConfig(voxel_edge_length=1))
        for p, P in enumerate(clouds):
            g.insert_points(p, P)
        g.subdivide([MaxPoints(args.k_split)])
        g._forest.ensure_built()
        if thinned:
            thin(g, L / 8)
        g.radius_count(clouds[0][:1], L / 8)           # (the index of every pose is in place)
        ctx.sync()
        return g

    def timed(fn, prefixes):
        ctx.set_profiling(1)
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e6
        t = ctx.timings()
        ctx.set_profiling(0)
        return {k: ms * 1e3 for k, (ms, _) in t.items() if k.startswith(prefixes)}, wall, out

    out = {"poses": args.poses, "points_per_pose": args.points, "rounds": args.rounds, "voxel_edge": L, "maps": {}}
    for name, thinned in (("as inserted", False), ("after thin(L/8)", True)):
        acc = {r: {k: [] for k in KERNELS + ("wall", "sparse_mask")} for r in radii}
        info = {}
        for i in range(args.rounds):
            for rname, r in radii.items():             # (alternated: cluster, then its yardstick, radius after radius)
                g = build(thinned)
                f = g._forest
                n = int(f.n_ord)
                if i == 0:
                    cluster(g, r)                      # (warm: tables and staging)
                    ctx.sync()
                k, wall, cl = timed(lambda: cluster(g, r), KERNELS)
                for key in KERNELS:
                    acc[rname][key].append(k[key])
                acc[rname]["wall"].append(wall)
                if i == 0:
                    info[rname] = {"radius": r, "points": n, "clusters": int(len(cl)),
                                   "largest": int(cl.sizes.max()) if len(cl) else 0,
                                   "singletons": int((cl.sizes == 1).sum())}
                    if n <= args.definition_max:
                        # (the rows that are still in the map, in the order of the clouds as inserted: ids as the device's)
                        listed = [(p, clouds[p][cl.index[cl.pose == p]]) for p in range(args.poses)]
                        t0 = time.perf_counter()
                        labels, sizes, _ = cluster_labels_np(listed, r)
                        info[rname]["definition_wall_us"] = round((time.perf_counter() - t0) * 1e6, 1)
                        info[rname]["definition_agrees"] = bool(np.array_equal(np.concatenate(labels), cl.label)
                                                                and np.array_equal(sizes, cl.sizes))
                k, _, removed = timed(lambda: g.remove_sparse(r, 2 ** 31 - 1), ("sparse_mask",))
                assert removed == n
                acc[rname]["sparse_mask"].append(k["sparse_mask"])
                print(f"{name}, {rname}, round {i}: done", file=sys.stderr, flush=True)
        out["maps"][name] = {}
        for rname in radii:
            a = acc[rname]
            row = dict(info[rname])
            row.update({f"{key}_kernel_us": _stat(a[key]) for key in KERNELS})
            row["sparse_mask_kernel_us"] = _stat(a["sparse_mask"])
            row["call_wall_us"] = _stat(a["wall"])
            row["link_over_sparse_mask"] = round(statistics.median(a["cluster_link"])
                                                 / statistics.median(a["sparse_mask"]), 3)
            out["maps"][name][rname] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
