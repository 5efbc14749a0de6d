"""Device time of the neighbour query on BASELINE config 3 (10 M planar points, Grid of 1 m voxels, subdivide(len > 64),
map_leaf_points_cuda_ransac with H = 1024, k = 6, thr = 0.01, incl. apply_mask), for 10 M and 100 k query points (a
second scan of the same scene: shuffled, and in the order a rotating LiDAR delivers it - synthetic.sweep_order).
Arms alternated in one process, medians with min - max:

  nearest k, r     kernel time of octl_forest_nearest_device from the library's hipEvent timers (the points are in HBM
                   already, the block index of the selection exists), for k = 1 with r = 0.05 and k = 8 with r = 0.3
  locate           kernel time of octl_forest_locate_device on the same queries in the same run: the walk to the
                   query's own leaf alone, the floor of any search that starts there - and the ratio to it
  nn_index         the kernels that make the index node -> run of blocks (once per forest state and pose selection)

Prints one JSON object.

    python tools/nearest_timing.py [--n 10000000] [--queries 10000000 100000] [--rounds 7]
"""

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETTINGS = ((1, 0.05), (8, 0.3))


def _stat(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, nargs="+", default=[10_000_000, 100_000])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--k-split", type=int, default=64)
    args = ap.parse_args()

    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig

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
    f.n_ord   # (books the compaction's counts)

    def timed(fn, prefixes):
        """kernel microseconds by timer name (those starting with one of `prefixes`)"""
        ctx.set_profiling(1)
        fn()
        ctx.sync()
        t = ctx.timings()
        ctx.set_profiling(0)
        return {k: ms * 1e3 for k, (ms, _) in t.items() if k.startswith(prefixes)}

    out = {"config": "config3", "n": args.n, "map_points": int(f.n_ord), "nodes": int(len(f.nodes["edge"])),
           "blocks": int(len(f.blocks["node"])), "rounds": args.rounds, "queries": {}}

    for nq in args.queries:
        scan = synthetic.planar_cloud(nq, (32, 32, 32), seed=1, stream=1)
        clouds = {"shuffled": scan, "sweep": synthetic.sweep_order(scan, seed=2)}
        bufs = []

        def dev(nbytes):
            p = C.c_void_p()
            ctx.check(lib.octl_dev_alloc(ctx.handle, int(nbytes), C.byref(p)))
            bufs.append(p)
            return p

        kmax = max(k for k, _ in SETTINGS)
        xin, d_node = dev(24 * nq), dev(4 * nq)
        d_slot, d_idx, d_d2, d_cnt = dev(4 * nq * kmax), dev(8 * nq * kmax), dev(8 * nq * kmax), dev(4 * nq)
        res = {}
        for order, Q in clouds.items():
            ctx.check(lib.octl_dev_upload(ctx.handle, xin, nat.ptr(Q), Q.nbytes))
            f.locate_device(xin, nq, d_node)            # (warm: voxel codes, the index)
            for k, r in SETTINGS:
                f.nearest_device(xin, nq, k, r, d_slot, d_idx, d_d2, d_cnt)
            ctx.sync()
            loc = []
            nn = {kr: [] for kr in SETTINGS}
            for _ in range(args.rounds):                 # arms alternated
                loc.append(timed(lambda: f.locate_device(xin, nq, d_node), ("locate",))["locate"])
                for k, r in SETTINGS:
                    t = timed(lambda: f.nearest_device(xin, nq, k, r, d_slot, d_idx, d_d2, d_cnt), ("nearest_",))
                    nn[(k, r)].append(sum(t.values()))
            rr = {"locate_kernel_us": _stat(loc)}
            for k, r in SETTINGS:
                f.nearest_device(xin, nq, k, r, d_slot, d_idx, d_d2, d_cnt)
                cnt = np.empty(nq, dtype=np.int32)
                ctx.check(lib.octl_dev_download(ctx.handle, nat.ptr(cnt), d_cnt, cnt.nbytes))
                med = statistics.median(nn[(k, r)])
                rr[f"nearest_k{k}_r{r}"] = {"kernel_us": _stat(nn[(k, r)]), "ns_per_query": round(med * 1e3 / nq, 2),
                                            "ratio_to_locate": round(med / statistics.median(loc), 2),
                                            "found_none_share": round(float((cnt == 0).mean()), 4),
                                            "full_share": round(float((cnt == k).mean()), 4)}
            res[order] = rr
        for p in bufs:
            lib.octl_dev_free(ctx.handle, p)
        out["queries"][str(nq)] = res

    # the index: "pose 0" and "all poses" are the same blocks but another selection, so every call makes it again
    idx = []
    q1 = np.ascontiguousarray(P[:256])
    for i in range(args.rounds):
        sel = [0] if i % 2 == 0 else None
        t = timed(lambda: f.nearest(q1, 1, 0.05, sel), ("nn_",))   # (nn_group covers its sort)
        idx.append(sum(t.values()))
    out["nn_index_kernels_us"] = _stat(idx)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
