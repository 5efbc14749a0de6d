#!/usr/bin/env python3
"""CPU model of k_ransac's certified exit (csrc/plane_cert.h, "the certified exit" in csrc/ransac.hip): how many leaves
end behind group 0 because no plane can hold more points than the best of hypotheses 0..63, and what the
per-hypothesis cross-product test still sends to the exact queue.
    python tools/cert_exit_sim.py [voxels_per_axis] [seed]
Leaves as in tools/prescreen_stage_sim.py: the benchmark's planar and uniform scenes at the headline density through the
NumPy oracle, the benchmark's hypothesis table.  Per leaf: the reference's planes and exact counts of all 1024
hypotheses (oracle/ransac_np.py), L = the best of the first 64, b = n - L, the certificate (tools/plane_cert_model.py, the
float64 port of the header with the kernel's t = PreConst::thrblk) and the cross-product test of the 960 later ones.
It also checks what the exit rests on: in a certified leaf every later hypothesis that beats L is one the test does
NOT vouch for (the reference's zero plane).  Forecast of a filter in front of the certificate (two f32 wave sums of the
residuals against the winner of group 0 instead of nine f64 sums; not built): the refused tests it would spare.  The counting build's shares (tools/rs_counts.py, slots 24..28) are set
beside these in profiles/r10_ransac_counts.json.
No GPU, no reference checkout."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octreelib_amd import synthetic  # noqa: E402
from oracle import octree_np as onp  # noqa: E402
from oracle import ransac_np as rnp  # noqa: E402
import plane_cert_model as pcm  # noqa: E402  (tools/plane_cert_model.py, beside this file)

THR, H, LANES, K = 0.01, 1024, 64, 6


def leaves_of(cloud):
    og = onp.OGrid(1)
    og.insert_points(0, cloud)
    og.subdivide(64)
    return [cloud[i] for _, _, i in og.leaf_table(0) if K <= len(i) < 64]


def run(name, cloud, table):
    t = dict(leaves=0, b0=0, b1=0, b2=0, b1_quiet=0, b2_quiet=0, c1=0, c2=0, later=0, queued=0, all_vouched=0,
             winners=0, zero_winners=0, slipped=0, inelig=0, r1=0, r2=0, f1=0, f2=0, lost=0)
    for pts in leaves_of(cloud):
        n = len(pts)
        idx = np.minimum((table * n).astype(np.int32), n - 1)
        plane = rnp.plane_from_points(pts[idx]).astype(np.float32).astype(np.float64)
        dist = np.abs(((plane[:, 0:1] * pts[None, :, 0] + plane[:, 1:2] * pts[None, :, 1])
                       + plane[:, 2:3] * pts[None, :, 2]) + plane[:, 3:4])
        cnt = (dist < THR).sum(1)
        L = int(cnt[:LANES].max())
        b = n - L
        t['leaves'] += 1
        if b > 2:
            continue
        t[f'b{b}'] += 1
        if b == 0:
            continue
        better = cnt[LANES:] > L
        t[f'b{b}_quiet'] += int(not better.any())
        cert = pcm.certified(pts, THR, L)
        if cert is None:
            t['inelig'] += 1
        # a filter in front of the certificate, from the residuals against the winner of group 0 (pcm.filter_skips)
        skip = cert is not None and pcm.filter_skips(pts, plane[int(np.argmax(cnt[:LANES] == L))],
                                                     pcm.block_constants(pts, THR)[1], b)
        if cert is False:
            t[f'r{b}'] += 1
            t[f'f{b}'] += int(skip)
        if not cert:
            continue
        t['lost'] += int(skip)
        t[f'c{b}'] += 1
        ok = pcm.vouched(pts, idx[LANES:])
        t['later'] += H - LANES
        t['queued'] += int((~ok).sum())
        t['all_vouched'] += int(ok.all())
        t['winners'] += int(better.any())
        t['zero_winners'] += int((better & (plane[LANES:, :3] == 0).all(1)).any())
        t['slipped'] += int((better & ok).sum())
    n = max(t['leaves'], 1)
    c = max(t['c1'] + t['c2'], 1)
    print(f"== {name}: {t['leaves']} leaves of {K}..63 points")
    print(f"  b = 0 (ends today)                    {100 * t['b0'] / n:5.1f} %")
    print(f"  b = 1                                 {100 * t['b1'] / n:5.1f} %   no later hypothesis improves in "
          f"{100 * t['b1_quiet'] / max(t['b1'], 1):.0f} % of them")
    print(f"  b = 2                                 {100 * t['b2'] / n:5.1f} %   no later hypothesis improves in "
          f"{100 * t['b2_quiet'] / max(t['b2'], 1):.0f} % of them")
    print(f"  b = 1 and certified                   {100 * t['c1'] / n:5.1f} %")
    print(f"  b = 2 and certified for every point   {100 * t['c2'] / n:5.1f} %")
    print(f"  tested leaves outside the prescreen's eligibility: {t['inelig']}")
    print(f"  certified leaves: {t['queued'] / c:.2f} of 960 later hypotheses not vouched for on average, none in "
          f"{100 * t['all_vouched'] / c:.0f} % of them; a later hypothesis wins in {t['winners']} "
          f"({t['zero_winners']} by the zero plane); vouched-for hypotheses that beat L: {t['slipped']}")
    print(f"  a filter on the residuals against the winner of group 0 would spare {t['f1']} of {t['r1']} refused tests at "
          f"b = 1 ({100 * t['f1'] / max(t['r1'], 1):.0f} %), {t['f2']} of {t['r2']} at b = 2 "
          f"({100 * t['f2'] / max(t['r2'], 1):.0f} %), and skip {t['lost']} of {t['c1'] + t['c2']} certifiable leaves")
    return t


def main():
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    dims = (side, side, side)
    npts = 305 * side ** 3
    np.random.seed(0)
    table = np.random.random((H, K))
    bad = run("planar", synthetic.planar_cloud(npts, dims, seed=seed), table)['slipped']
    bad += run("uniform", synthetic.uniform_cloud(npts, dims, seed=seed), table)['slipped']
    if bad:
        sys.exit("a vouched-for hypothesis beat L in a certified leaf: the exit would change results")


if __name__ == "__main__":
    main()
