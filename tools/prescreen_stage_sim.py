#!/usr/bin/env python3
"""CPU simulation of the two-stage widened count of k_ransac's prescreen (csrc/ransac.hip, "the two-stage widened
count"): how many hypotheses are decided after the first m points of a leaf, per order of the points, and what the
shipped rule (RS_STAGE1_SLACK, RS_STAGE2_MIN) executes against the single-stage count.
    python tools/prescreen_stage_sim.py [voxels_per_axis] [seed]
Leaves: the benchmark's planar and uniform scenes at the headline density (10 M points over 32^3 voxels = 305 per
voxel, subdivided while a leaf holds more than 64 points) through the NumPy oracle (oracle/octree_np.py), so the leaf
sizes have their real distribution.  Per leaf: the reference's sample rule and plane (oracle/ransac_np.py), exact counts
of hypotheses 0..63 -> L, and for the 960 later ones the count inside the prescreen's WIDENED threshold (a float64 port
of prescreen_constants and the per-hypothesis bound; the f32 roundings the kernel adds are far below the widening).
Cost unit: one point against one wavefront of hypotheses ("row"): five VALU instructions per hypothesis of a lane;
stage 1 and the single-stage count take three hypotheses per lane, so 15 group-rows per point; a stage-2 pass takes
one hypothesis per lane, one group-row per point whatever the number of busy lanes.
No GPU, no reference checkout."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octreelib_amd import synthetic  # noqa: E402
from oracle import octree_np as onp  # noqa: E402
from oracle import ransac_np as rnp  # noqa: E402

SLACK, MIN_REST = 2, 6          # RS_STAGE1_SLACK, RS_STAGE2_MIN of csrc/ransac.hip
THR, H, LANES, K = 0.01, 1024, 64, 6
U = 2.0 ** -24
UP = 1.0 + 2.0 ** -10


def stage1_points(n, budget, slack=SLACK, min_rest=MIN_REST):
    """m1 of the kernel; None = the single-stage count."""
    m1 = min(n, (budget + slack + 3) & ~3)
    return m1 if n - m1 >= min_rest else None


def leaves_of(cloud, dims):
    og = onp.OGrid(1)
    og.insert_points(0, cloud)
    og.subdivide(64)
    return [cloud[i] for _, _, i in og.leaf_table(0) if K <= len(i) < 64]


def widened(pts, samples, thr):
    """(960, n) inlier bits inside the widened threshold, and which hypotheses the bound vouches for."""
    o = pts[0]
    loc = pts - o
    S = samples - o
    E = np.abs(loc).max()
    G = np.abs(o).sum() + E
    k1 = 16.0 * (12.0 * U + 2.0 ** -46 * G / E)
    k0 = 16.0 * (3.0 * U * E * E + 2.0 ** -46 * G * E)
    qa, qb, qc = (k1 + 2.0 ** -20 + k1 * k1 / 16) * UP, (k0 + k1 * k0 / 8) * UP, k0 * k0 / 16 * UP + 2.0 ** -98
    thrblk = (thr + 64 * U * E + 2.0 ** -21 * G) * UP
    c = S.mean(1)
    R = S - c[:, None, :]
    C = np.einsum('hki,hkj->hij', R, R)
    xx, yy, zz, xy, xz, yz = C[:, 0, 0], C[:, 1, 1], C[:, 2, 2], C[:, 0, 1], C[:, 0, 2], C[:, 1, 2]
    dx, dy, dz = yy * zz - yz * yz, xx * zz - xz * xz, xx * yy - xy * xy
    cA, cB, cC = xz * yz - xy * zz, xy * yz - xz * yy, xy * xz - yz * xx
    bx = (dx > dy) & (dx > dz)
    by = ~bx & (dy > dz)
    row = np.stack([np.where(bx, dx, np.where(by, cA, cB)), np.where(bx, cA, np.where(by, dy, cC)),
                    np.where(bx, cB, np.where(by, cC, dz))], 1)
    norm = np.sqrt((row * row).sum(1))
    T = xx + yy + zz
    mu4 = (qa * T + qb) * T + qc
    d3 = np.sort(np.stack([dx, dy, dz], 1), 1)
    ok = (norm > mu4) & (d3[:, 2] - d3[:, 1] > mu4)
    with np.errstate(all='ignore'):
        nrm = row / norm[:, None]
        thr_h = 3.5 * E * UP * mu4 / norm + thrblk
        s = np.abs(np.einsum('hi,nhi->hn', nrm, loc[:, None, :] - c[None]))
        inl = s < thr_h[:, None]
    inl[~ok] = True
    return inl, ok


def run(name, cloud, dims, table):
    ms = (6, 8, 10, 12)
    orders = ('storage', 'partition', 'sorted')
    decided = {o: {m: [] for m in ms} for o in orders}
    tot = dict(blocks=0, after_group0=0, single=0, rows_today=0, rows_stage1=0, rows_stage2=0, rows_single=0,
               queued=0, passes=0, hyps=0, survivors=0, pairs_today=0, pairs1=0, pairs2=0)
    grid = {(s, r): [0, 0] for s in (0, 2, 4, 8) for r in (4, 6, 8, 12)}   # rule -> [partition rows, sorted rows]
    for pts in leaves_of(cloud, dims):
        n = len(pts)
        idx = np.minimum((table * n).astype(np.int32), n - 1)
        plane = rnp.plane_from_points(pts[idx]).astype(np.float32).astype(np.float64)
        dist = np.abs(((plane[:, 0:1] * pts[None, :, 0] + plane[:, 1:2] * pts[None, :, 1])
                       + plane[:, 2:3] * pts[None, :, 2]) + plane[:, 3:4])
        cnt0 = (dist[:LANES] < THR).sum(1)
        L = int(cnt0.max())
        tot['blocks'] += 1
        if L == n:
            tot['after_group0'] += 1
            continue
        budget = n - L
        win = int(np.argmax(cnt0))
        inl, ok = widened(pts, pts[idx[LANES:]], THR)
        G = (H - LANES) // LANES
        tot['hyps'] += H - LANES
        tot['survivors'] += int((inl.sum(1) > L).sum())
        far = ~(dist[win] < THR)
        perm = {'storage': np.arange(n), 'partition': np.argsort(~far, kind='stable'),
                'sorted': np.argsort(-dist[win], kind='stable')}
        miss = {o: np.cumsum(~inl[:, perm[o]], 1) for o in orders}
        for o in orders:
            for m in ms:
                decided[o][m].append(float((miss[o][:, min(m, n) - 1] >= budget).mean()))
        for (s, r), acc in grid.items():
            m1 = stage1_points(n, budget, s, r)
            for j, o in enumerate(('partition', 'sorted')):
                if m1 is None:
                    acc[j] += G * n
                else:
                    alive = int((miss[o][:, m1 - 1] < budget).sum())
                    acc[j] += G * m1 + -(-alive // LANES) * (n - m1)
        tot['rows_today'] += G * n
        tot['pairs_today'] += (H - LANES) * n
        m1 = stage1_points(n, budget)
        if m1 is None:
            tot['single'] += 1
            tot['rows_single'] += G * n
            continue
        alive = int((miss['partition'][:, m1 - 1] < budget).sum())
        passes = -(-alive // LANES)
        tot['rows_stage1'] += G * m1
        tot['rows_stage2'] += passes * (n - m1)
        tot['pairs1'] += (H - LANES) * m1
        tot['pairs2'] += alive * (n - m1)
        tot['queued'] += alive
        tot['passes'] += passes
    pre = tot['blocks'] - tot['after_group0']
    print(f"== {name}: {tot['blocks']} leaves of 6..63 points, {tot['after_group0']} end with group 0, "
          f"{pre} prescreened; survivors of the widened count {tot['survivors'] / max(tot['hyps'], 1):.4f}")
    print("share of hypotheses 64..1023 dead after the first m points:")
    for o in orders:
        print(f"  {o:10s} " + "  ".join(f"m={m}: {100 * np.mean(decided[o][m]):5.1f} %" for m in ms))
    rows_new = tot['rows_stage1'] + tot['rows_stage2'] + tot['rows_single']
    print(f"shipped rule (slack {SLACK}, min rest {MIN_REST}, two-class partition):")
    print(f"  blocks on the single-stage branch {tot['single']} of {pre} ({100 * tot['single'] / max(pre, 1):.1f} %)")
    print(f"  group-rows: today {tot['rows_today']}, stage 1 {tot['rows_stage1']}, stage 2 {tot['rows_stage2']}, "
          f"single-stage {tot['rows_single']} -> {rows_new / max(tot['rows_today'], 1):.3f} of today's")
    print(f"  pairs with a live hypothesis: today {tot['pairs_today']}, stage 1 {tot['pairs1']}, stage 2 {tot['pairs2']}")
    print(f"  queued for stage 2: {tot['queued']} ({tot['queued'] / max(pre - tot['single'], 1):.1f} per two-stage block, "
          f"{tot['queued'] / max(tot['hyps'], 1):.4f} of the hypotheses), stage-2 passes {tot['passes']} "
          f"({tot['passes'] / max(pre - tot['single'], 1):.2f} per two-stage block)")
    print("  group-rows relative to today's per rule (slack, min rest): partition / sorted")
    for (s, r), acc in sorted(grid.items()):
        print(f"    slack {s} rest {r:2d}: {acc[0] / max(tot['rows_today'], 1):.3f} / {acc[1] / max(tot['rows_today'], 1):.3f}")
    return rows_new / max(tot['rows_today'], 1)


def main():
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    dims = (side, side, side)
    npts = 305 * side ** 3
    np.random.seed(0)
    table = np.random.random((H, K))
    run("planar", synthetic.planar_cloud(npts, dims, seed=seed), dims, table)
    run("uniform", synthetic.uniform_cloud(npts, dims, seed=seed), dims, table)


if __name__ == "__main__":
    main()
