"""Short random operation sequences with prune() among them (seeds fixed here): {insert late, subdivide, RANSAC +
apply_mask, carve_rays, remove_poses, prune} on a grid of 3 x 3 x 2 voxels of 1 m.

Two maps get every operation; only one of them, P, is ever pruned.  Every prune is checked against its definition
(query.prune_np of the tables before: test_gpu_prune._prune_and_check) and the map queries taken before it are
compared with those after through PruneResult.node_map (_queries_equal).  The pruned map and its unpruned twin T
are compared by everything a pose reads back (_reads_equal) after every prune - up to the first late pose inserted
into a map that has been pruned: from there on the two schemes differ by definition (a re-created voxel is an unsplit
root at the end of the creation order, a collapsed node that is split again has a new epoch), per-leaf operations see
other leaves, and the twin is no reference any more; the two self-checks go on to the end of the sequence.

The two sequence tests divide the work: this one holds prune against an UNPRUNED TWIN, on one Grid in f64 with seven
kinds of operation; tests/test_gpu_opseq.py (SEEDS4) draws prune among every other operation of the API - on Grid,
OctreeManager and Octree, f32 and UTM clouds, next to plane_segments, adjustment_system, transform_poses, filters and
the radius searches - against the oracle MODEL pruned by the definition, with the same two self-checks on every
drawn prune."""

import numpy as np
import pytest

from octreelib_amd import MaxPoints, synthetic
from octreelib_amd.grid import Grid, GridConfig
from tests.test_gpu_prune import (DIMS, RAYS_D, RAYS_O, RAYS_R, TABLE, THRESHOLD, _prune_and_check, _queries,
                                  _queries_equal, _reads_equal)

pytestmark = pytest.mark.gpu

SEEDS = list(range(30))
OPS = ("insert", "subdivide", "ransac", "carve", "remove", "prune", "prune")


def _cloud(rng, seed, stream):
    """300 - 800 points of the scene in a random sub-box of at least one voxel."""
    lo = np.array([rng.integers(0, d) for d in DIMS])
    hi = np.array([rng.integers(l + 1, d + 1) for l, d in zip(lo, DIMS)])
    n = int(rng.integers(300, 801))
    return synthetic.planar_cloud(n, DIMS, seed=seed, stream=stream, box=(tuple(lo.tolist()), tuple(hi.tolist())))


def _apply(g, op, arg):
    if op == "insert":
        g.insert_points(*arg)
    elif op == "subdivide":
        g.subdivide([MaxPoints(arg)])
    elif op == "ransac":
        g.map_leaf_points_cuda_ransac(poses_per_batch=2, threshold=THRESHOLD, hypotheses=TABLE)
    elif op == "carve":
        g.carve_rays(RAYS_O[arg], RAYS_D[arg], RAYS_R[arg], 0.05, min_through=1)
    elif op == "remove":
        g.remove_poses([arg])


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence(seed):
    rng = np.random.default_rng(1000 + seed)
    P, T = (Grid(GridConfig(voxel_edge_length=1)) for _ in range(2))
    poses, next_pose, stream = [], 0, 0
    log = []

    def both(op, arg):
        log.append((op, (arg[0], len(arg[1])) if op == "insert" else int(arg.sum()) if op == "carve" else arg))
        for g in (P, T):
            _apply(g, op, arg)

    for _ in range(3):
        both("insert", (next_pose, _cloud(rng, 40 + seed, stream)))
        poses.append(next_pose)
        next_pose, stream = next_pose + 1, stream + 1
    both("subdivide", int(rng.choice([8, 16, 32])))
    pruned, twin_valid, prunes = False, True, 0
    ops = list(rng.choice(OPS, size=int(rng.integers(4, 8)))) + ["prune"]
    for op in ops:
        if op == "insert":
            both("insert", (next_pose, _cloud(rng, 40 + seed, stream)))
            poses.append(next_pose)
            next_pose, stream = next_pose + 1, stream + 1
            twin_valid = twin_valid and not pruned
        elif op == "subdivide":
            both("subdivide", int(rng.choice([8, 16, 32])))
        elif op == "ransac":
            both("ransac", None)
        elif op == "carve":
            both("carve", rng.random(len(RAYS_O)) < 0.6)
        elif op == "remove":
            # (the LAST pose, so that the numbers stay dense: map_leaf_points_cuda_ransac takes pose indices as numbers)
            if len(poses) > 1:
                next_pose = poses.pop()
                both("remove", int(next_pose))
        else:
            log.append(("prune", None))
            f = P._forest
            nodes_before = {k: v.copy() for k, v in f.nodes.items()}
            before = _queries(P)
            res, _, _ = _prune_and_check(P, f"seed {seed}: {log}", expect_change=False)
            _queries_equal(before, _queries(P), res, nodes_before, P, f"seed {seed}: {log}")
            if twin_valid:
                _reads_equal(P, T, poses, f"seed {seed}: {log}")
            pruned = True
            prunes += 1
    assert prunes >= 1
    for g in (P, T):
        g._forest.close()
