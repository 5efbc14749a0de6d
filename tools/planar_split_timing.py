"""Time of a planarity-driven subdivide (NotPlanar(2.5e-4, 8) OR len > 4096, Grid of 1 m voxels, one pose of
synthetic.planar_cloud) on the device against the two things it can be compared with, arms alternating in one process:

  host      the only way to do this before octl_forest_build_planar: the criterion wrapped in a lambda, evaluated on
            the host level by level (Forest.subdivide_callable: a re-placement, a download of every point and a
            Python loop over the frontier per level).  Skipped at a size where one round would exceed --host-budget-s
            (estimated from the previous size, linear in n); the output says so.
  device    the same list given as NotPlanar / MaxPoints instances (Forest.subdivide_planar)
  count     the count-driven level loop (NO_BUCKET_BUILD, so that it is the same loop) with the largest K from
            4096, 2048, ... whose tree is at least as deep as the planar one: what the loop costs without the statistic

Every arm is timed from a fresh Grid whose points are stored already, around the subdivide call, which ends in a host
wait (median, min, max over --rounds of time.perf_counter).  One more round of the device and the count arm runs
under the library's hipEvent timers (octl_ctx_get_timings): node_moments / node_lambda beside level_hist and the
rest of the loop.  Prints one JSON object.

    python tools/planar_split_timing.py [--sizes 1000000,10000000] [--rounds 5] [--host-budget-s 120]
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-budget-s", type=float, default=120.0)
    args = ap.parse_args()

    from octreelib_amd import MaxPoints, NotPlanar, synthetic
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig

    ctx = nat.get_context()
    plane = NotPlanar(2.5e-4, 8)
    crit = [plane, MaxPoints(4096)]
    wrapped = [lambda points: plane(points), MaxPoints(4096)]   # (one unrecognised callable: the host path)

    def run(P, criteria, general=False):
        g = Grid(GridConfig(voxel_edge_length=1))
        g.insert_points(0, P)
        if general:
            ctx.set_option("NO_BUCKET_BUILD", 1)
        ctx.sync()
        t0 = time.perf_counter()
        g.subdivide(criteria)
        ctx.sync()
        dt = time.perf_counter() - t0
        if general:
            ctx.set_option("NO_BUCKET_BUILD", 0)
        info = g._forest.info
        out = (dt * 1e3, int(info.n_nodes), int(info.max_depth))
        g._forest.close()
        return out

    def summary(ts):
        return {"median_ms": round(statistics.median(ts), 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)}

    def kernels(P, criteria, general):
        ctx.set_profiling(1)
        run(P, criteria, general)
        t = ctx.timings()
        ctx.set_profiling(0)
        return {k: [round(ms, 3), n] for k, (ms, n) in sorted(t.items())}

    result = {"criterion": "NotPlanar(2.5e-4, 8) OR len > 4096", "rounds": args.rounds, "sizes": {}}
    host_ms_per_point = None
    for n in [int(x) for x in args.sizes.split(",")]:
        side = max(2, round((n / 2000.0) ** (1.0 / 3.0)))   # about 2000 points per voxel
        P = synthetic.planar_cloud(n, (side, side, side), seed=1)
        _, nodes, depth = run(P, crit)   # (warm: buffers, and the depth the count arm has to reach)
        k_count = 4096
        while k_count > 8 and run(P, [MaxPoints(k_count)], True)[2] < depth:
            k_count //= 2
        do_host = host_ms_per_point is None or host_ms_per_point * n / 1e3 <= args.host_budget_s
        ts = {"host": [], "device": [], "count": []}
        count_nodes = host_nodes = None
        for _ in range(args.rounds):
            if do_host:
                t, host_nodes, _ = run(P, wrapped)
                ts["host"].append(t)
                if t / 1e3 * (args.rounds - len(ts["host"])) > args.host_budget_s:
                    do_host = False   # (the rounds that are left would not fit)
            ts["device"].append(run(P, crit)[0])
            t, count_nodes, count_depth = run(P, [MaxPoints(k_count)], True)
            ts["count"].append(t)
        if ts["host"]:
            host_ms_per_point = statistics.median(ts["host"]) / n
        entry = {
            "dims": [side] * 3, "nodes": nodes, "depth": depth,
            "host": dict(summary(ts["host"]), rounds=len(ts["host"]), nodes=host_nodes) if ts["host"] else
            f"skipped: one round estimated above the budget of {args.host_budget_s} s",
            "device": summary(ts["device"]),
            "count": dict(summary(ts["count"]), K=k_count, nodes=count_nodes, depth=count_depth),
            "kernels_device": kernels(P, crit, False),
            "kernels_count": kernels(P, [MaxPoints(k_count)], True),
        }
        if ts["host"]:
            assert host_nodes == nodes, "host and device path built different trees"
            entry["host_over_device"] = round(statistics.median(ts["host"]) / statistics.median(ts["device"]), 1)
        entry["device_over_count"] = round(statistics.median(ts["device"]) / statistics.median(ts["count"]), 2)
        result["sizes"][str(n)] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
