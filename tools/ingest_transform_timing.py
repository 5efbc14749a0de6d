"""Time of inserting a sweep under a transform (k_ingest_xf) on BASELINE config 3's scene: a map of
planar points in one Grid of 1 m voxels and a sweep of 100 k points that arrives in the sensor frame.  Arms alternated
in one process, medians with min - max:

  kernels (the library's hipEvent timers, device sources behind an even store):
    ingest, ingest_f32            the parent's kernels on the same rows: the yardsticks (copy / widen, no transform)
    xf_f64, xf_f32                k_ingest_xf under one rigid transform
    xf_f64_sweep, xf_f32_sweep    piecewise, M = 1024, indices in sweep order (the wave-uniform path)
    xf_f64_shuffled, ..           piecewise, M = 1024, shuffled indices (the per-lane gather)
  with ns per byte moved (read + written, the 2 B index included) and the ratio to the yardstick of the same source type
  wall time from Python of one insert_points of the sweep, the stream drained:
    host_f64, host_f32, device    insert_points(p, scan, transform=T)
    numpy_then_insert             transform_np on the host, then insert_points: the only way before

Prints one JSON object.

    python tools/ingest_transform_timing.py [--map 10000000] [--n 100000] [--rounds 7]
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stat(v, digits=2):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", type=int, default=10_000_000, help="points of the map the sweep is inserted into")
    ap.add_argument("--n", type=int, default=100_000, help="points of the sweep")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()

    import octreelib_amd as oa
    from octreelib_amd import synthetic
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig
    from octreelib_amd.registration import se3_exp, transform_np

    n, M = args.n, 1024
    ctx = nat.get_context()
    rng = np.random.default_rng(0)
    scan = synthetic.planar_cloud(n, (32, 32, 32), seed=1, stream=99)
    scan32 = scan.astype(np.float32)
    T = se3_exp(np.concatenate([rng.normal(size=3) * 0.01, rng.normal(size=3) * 0.05]))
    Ts = np.stack([se3_exp(np.concatenate([rng.normal(size=3) * 0.01, rng.normal(size=3) * 0.05])) for _ in range(M)])
    sweep = (np.arange(n) * M // n).astype(np.uint16)            # firing columns in order
    shuffled = rng.permutation(sweep)
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, synthetic.planar_cloud(args.map + (args.map & 1), (32, 32, 32), seed=1))   # (an even store)
    f = g._forest
    d64, d32 = oa.upload_async(scan), oa.upload_async(scan32)
    d64.wait()
    d32.wait()
    next_pose = [1]

    def insert(points, **kw):
        g.insert_points(next_pose[0], points, **kw)
        next_pose[0] += 1

    def kernel_us(fn, label):
        ctx.sync()
        ctx.set_profiling(1)
        ctx.timings()
        fn()
        ctx.sync()
        t = ctx.timings()
        ctx.set_profiling(0)
        return t[label][0] * 1e3

    def plain_device_f64():
        f.add_pose_device(d64.ptr, n)      # (copied by k_ingest<true>, not adopted: the forest holds the map)

    kernels = {
        "ingest": (plain_device_f64, "ingest", 48 * n),
        "ingest_f32": (lambda: insert(d32), "ingest_f32", 36 * n),
        "xf_f64": (lambda: insert(d64, transform=T), "ingest_xf", 48 * n),
        "xf_f32": (lambda: insert(d32, transform=T), "ingest_xf_f32", 36 * n),
        "xf_f64_sweep": (lambda: insert(d64, transform=Ts, segment=sweep), "ingest_xf", 50 * n),
        "xf_f32_sweep": (lambda: insert(d32, transform=Ts, segment=sweep), "ingest_xf_f32", 38 * n),
        "xf_f64_shuffled": (lambda: insert(d64, transform=Ts, segment=shuffled), "ingest_xf", 50 * n),
        "xf_f32_shuffled": (lambda: insert(d32, transform=Ts, segment=shuffled), "ingest_xf_f32", 38 * n),
    }

    def keep_even():
        # every arm starts behind an even number of stored rows (the sweep may be odd)
        if n & 1:
            insert(scan[:1])

    def wall_us(fn):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e6

    walls = {
        "host_f64": lambda: insert(scan, transform=T),
        "host_f32": lambda: insert(scan32, transform=T),
        "device": lambda: insert(d64, transform=T),
        "numpy_then_insert": lambda: insert(transform_np(T, scan)),
    }
    for fn, _, _ in kernels.values():        # warm: staging buffers, the store's growth
        fn()
        keep_even()
    for fn in walls.values():
        fn()
        keep_even()
    k_us = {k: [] for k in kernels}
    w_us = {k: [] for k in walls}
    for _ in range(args.rounds):             # arms alternated
        for name, (fn, label, _) in kernels.items():
            k_us[name].append(kernel_us(fn, label))
            keep_even()
        for name, fn in walls.items():
            w_us[name].append(wall_us(fn))
            keep_even()
    out = {"config": "config3 scene, one sweep", "map_points": args.map, "sweep_points": n, "transforms": M,
           "rounds": args.rounds, "stored_points_at_end": int(sum(f.slot_sizes)), "kernel_us": {}, "ns_per_byte": {},
           "ratio_to_yardstick": {}, "wall_us": {k: _stat(v, 1) for k, v in w_us.items()}}
    for name, (_, _, nbytes) in kernels.items():
        out["kernel_us"][name] = _stat(k_us[name])
        out["ns_per_byte"][name] = round(statistics.median(k_us[name]) * 1e3 / nbytes, 5)
        yard = "ingest_f32" if "f32" in name else "ingest"
        out["ratio_to_yardstick"][name] = round(statistics.median(k_us[name]) / statistics.median(k_us[yard]), 3)
    out["wall_ratio_numpy_over_device_transform"] = {
        k: round(statistics.median(w_us["numpy_then_insert"]) / statistics.median(w_us[k]), 2)
        for k in ("host_f64", "host_f32", "device")}
    print(json.dumps(out))
    f.close()
    d64.release()
    d32.release()


if __name__ == "__main__":
    main()
