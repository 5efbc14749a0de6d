"""Multi-pose plane adjustment on the host: adjustment_system_np / adjust_np (octreelib_amd/adjustment.py), the
specification the device is tested against (tests/test_gpu_adjustment.py shares the scenes below)."""

import numpy as np
import pytest

from octreelib_amd.adjustment import (AdjustmentSystem, adjust_np, adjustment_system_np, as_transforms,
                                      block_moments_np, root_box_centre, tree_depth)
from octreelib_amd.registration import se3_exp, transform_np

LD = np.longdouble
_TRIU = np.triu_indices(6)
ROOM_ORIGIN = np.array([3.25, 2.75, 1.75])
ROOM_MAX_VARIANCE = 1e-4     # a wall voxel has lambda0 ~ sigma^2 = 4e-6, a voxel on an edge or corner of the room ~ 1e-2


def sums28(s: AdjustmentSystem, k: int):
    return np.concatenate([np.asarray(s.H[k])[_TRIU], np.asarray(s.g[k]), [s.cost[k]]])


def random_rigid(rng, angle, shift, origin=None):
    w = rng.normal(size=3)
    v = rng.normal(size=3)
    return se3_exp(np.concatenate([angle * w / np.linalg.norm(w), shift * v / np.linalg.norm(v)]), origin)


def room_scene(n_poses=4, n=20000, sigma=0.002, seed=0):
    """(inserted clouds, the increments that undo their displacement): n_poses scans of one noisy box-shaped room of
    6 x 5 x 3 m whose walls lie a quarter voxel off the 1 m grid; poses 1.. are displaced by about 0.4 degrees and
    1 cm, pose 0 is where it belongs."""
    rng = np.random.default_rng(seed)
    size = np.array([6.0, 5.0, 3.0])
    clouds, truth = [], []
    for p in range(n_poses):
        face = rng.integers(0, 6, n)
        x = rng.random((n, 3)) * size
        x[np.arange(n), face // 2] = (face % 2) * size[face // 2] + rng.normal(0.0, sigma, n)
        T = np.eye(4) if p == 0 else random_rigid(rng, 0.007, 0.01, ROOM_ORIGIN)
        clouds.append(transform_np(np.linalg.inv(T), x + 0.25))
        truth.append(T)
    return clouds, np.stack(truth)


def voxel_blocks(clouds, edge=1.0):
    """(node, pose index, anchor, points) of every (voxel, pose) block, node = rank of the voxel in lexicographic
    order: the blocks of an unsubdivided grid."""
    q = [np.floor(x / edge).astype(np.int64) for x in clouds]
    vox = np.unique(np.concatenate(q), axis=0)
    rows = []
    for k, x in enumerate(clouds):
        for i, v in enumerate(vox):
            sel = np.all(q[k] == v, axis=1)
            if sel.any():
                rows.append((i, k, (v + 0.5) * edge, x[sel]))
    return rows


def worst_pose_error(T, truth):
    """Largest entry of T_p - truth_p over the poses (pose 0 is the gauge: its truth is the identity)."""
    return float(max(np.abs(np.asarray(T)[k][:3] - truth[k][:3]).max() for k in range(len(truth))))


def assert_recovers(res, truth):
    e0, e1 = worst_pose_error(np.stack([np.eye(4)] * len(truth)), truth), worst_pose_error(res.transforms, truth)
    print(f"worst pose error {e0:.5f} -> {e1:.6f}, {res.iterations} iterations, cost {res.costs[0]:.4g} -> "
          f"{res.costs[-1]:.4g}")
    assert res.converged and res.reason == "converged" and res.iterations <= 200
    assert len(res.costs) == res.iterations and res.costs[-1] < res.costs[0]
    assert 4 * e1 <= e0
    return e0, e1


@pytest.fixture(scope="module")
def room():
    clouds, truth = room_scene()
    return clouds, truth, block_moments_np(voxel_blocks(clouds), list(range(len(clouds))), ROOM_ORIGIN)


def _pointwise(rows, T, leaves, c, S):
    """The 28 sums per pose and the sums of their absolute terms, point by point from the transformed points."""
    out, mag = np.zeros((S, 28), dtype=LD), np.zeros((S, 28), dtype=LD)
    for node, k, _, x in rows:
        r_ = int(np.searchsorted(leaves.node, node))
        if not leaves.used[r_]:
            continue
        R, t = T[k][:3, :3].astype(LD), T[k][:3, 3].astype(LD)
        p = x.astype(LD) @ R.T + t
        nrm = np.tile(leaves.normal[r_].astype(LD), (len(p), 1))
        r = ((p - leaves.mean[r_].astype(LD)) * nrm).sum(axis=1)
        J = np.concatenate([np.cross(p - c.astype(LD), nrm), nrm], axis=1)
        terms = np.concatenate([J[:, _TRIU[0]] * J[:, _TRIU[1]], J * r[:, None], (r * r / 2)[:, None]], axis=1)
        out[k] += terms.sum(axis=0)
        mag[k] += np.abs(terms).sum(axis=0)
    return out, mag


def test_moment_algebra_matches_point_sums():
    rng = np.random.default_rng(5)
    S, c = 3, np.array([0.3, -0.2, 0.1])
    rows = [(leaf, k, np.array([2.0 * leaf, 1.0, -1.0]) + 0.5,
             np.array([2.0 * leaf, 1.0, -1.0]) + rng.random((int(rng.integers(1, 40)), 3)))
            for leaf in range(5) for k in range(S) if rng.random() < 0.8]
    bm = block_moments_np(rows, list(range(S)), c, dtype=LD)
    T = np.stack([random_rigid(rng, 0.8, 0.7) for _ in range(S)])
    # (the specification moves the anchor in f64; the same motion exactly: a' = R a + t with t = a' - R a is not one
    #  rigid motion per pose, so the points move by the pose's transform and the margin covers the rounding of a')
    s = adjustment_system_np(bm, T, c, min_points=1, min_poses=1, dtype=LD, leaves=True)
    assert s.leaves.used.all() and s.n_leaves == (len(s.leaves), len(s.leaves))
    want, mag = _pointwise(rows, T, s.leaves, c, S)
    for k in range(S):
        err = np.abs(sums28(s, k) - want[k])
        assert np.all(err <= 1e-12 * mag[k]), (k, float((err / mag[k]).max()))
    assert s.n_points.tolist() == [sum(len(x) for _, p, _, x in rows if p == k) for k in range(S)]
    assert s.n_blocks.tolist() == [sum(1 for _, p, _, _ in rows if p == k) for k in range(S)]


def test_g_is_the_gradient_of_the_eigen_factor_cost(room):
    _, _, bm = room
    S, h, k = 4, 1e-6, 2
    s0 = adjustment_system_np(bm, None, max_variance=ROOM_MAX_VARIANCE, leaves=True)
    assert 0 < s0.n_leaves[1] < s0.n_leaves[0]
    # (the cost is sum_l N_l lambda0_l / 2 over the used leaves: the residuals are taken about the pooled mean)
    lam = s0.leaves.lambda0[s0.leaves.used] * s0.leaves.count[s0.leaves.used]
    assert abs(float(s0.total_cost) - lam.sum() / 2) <= 1e-9 * lam.sum()
    for comp in range(6):
        cost = []
        for sign in (1.0, -1.0):
            T = np.stack([np.eye(4)] * S)
            T[k] = se3_exp(sign * h * np.eye(6)[comp], s0.origin)
            s = adjustment_system_np(bm, T, max_variance=ROOM_MAX_VARIANCE, dtype=LD, leaves=True)
            assert np.array_equal(s.leaves.used, s0.leaves.used)       # (no leaf changes its state across the probe)
            cost.append(s.total_cost)
        fd = float((cost[0] - cost[1]) / (2 * h))
        assert abs(fd - s0.g[k][comp]) <= 1e-4 * np.abs(s0.g[k]).max(), (comp, fd, s0.g[k][comp])


def test_rigid_motion_of_everything_changes_nothing(room):
    _, truth, bm = room
    rng = np.random.default_rng(2)
    G = random_rigid(rng, np.deg2rad(30.0), 2.0, ROOM_ORIGIN)
    T = np.stack([random_rigid(rng, 0.01, 0.02, ROOM_ORIGIN) for _ in range(4)])
    a = adjustment_system_np(bm, T, ROOM_ORIGIN, max_variance=ROOM_MAX_VARIANCE, dtype=LD)
    b = adjustment_system_np(bm, np.stack([G @ t for t in T]), G[:3, :3] @ ROOM_ORIGIN + G[:3, 3],
                             max_variance=ROOM_MAX_VARIANCE, dtype=LD)
    assert a.n_leaves == b.n_leaves and np.array_equal(a.n_points, b.n_points)
    D = np.zeros((6, 6))
    D[:3, :3] = D[3:, 3:] = G[:3, :3]
    for k in range(4):
        assert abs(a.cost[k] - b.cost[k]) <= 1e-9 * abs(a.cost[k])
        Hk, gk = D @ np.asarray(a.H[k], dtype=np.float64) @ D.T, D @ np.asarray(a.g[k], dtype=np.float64)
        assert np.abs(Hk - b.H[k]).max() <= 1e-9 * np.abs(Hk).max()
        assert np.abs(gk - b.g[k]).max() <= 1e-9 * np.abs(a.H[k]).max() * 1e-3


def test_gates_select_leaves_exactly():
    rng = np.random.default_rng(3)
    flat = lambda n, z: np.column_stack([rng.random(n), rng.random(n), 0.5 + rng.normal(0, z, n)])
    at = lambda leaf: np.array([3.0 * leaf, 0.0, 0.0])
    rows = [(0, 0, at(0) + 0.5, at(0) + flat(50, 1e-3)),                                   # one pose only
            (1, 0, at(1) + 0.5, at(1) + flat(3, 1e-3)), (1, 1, at(1) + 0.5, at(1) + flat(4, 1e-3)),     # 7 points
            (2, 0, at(2) + 0.5, at(2) + flat(30, 0.2)), (2, 2, at(2) + 0.5, at(2) + flat(30, 0.2)),     # thick
            (3, 1, at(3) + 0.5, at(3) + flat(20, 1e-3)), (3, 2, at(3) + 0.5, at(3) + flat(21, 1e-3))]
    c = np.array([4.0, 0.5, 0.5])
    T = np.stack([random_rigid(rng, 0.01, 0.01, c) for _ in range(3)])
    s = adjustment_system_np(block_moments_np(rows, [10, 11, 12], c), T, max_variance=1e-3, leaves=True)
    assert s.leaves.used.tolist() == [False, False, False, True] and s.n_leaves == (4, 1)
    assert s.n_points.tolist() == [0, 20, 21] and s.n_blocks.tolist() == [0, 1, 1]
    assert s.leaves.count.tolist() == [50, 7, 60, 41]
    only = adjustment_system_np(block_moments_np(rows[5:], [10, 11, 12], c), T, max_variance=1e-3)
    for k in range(3):       # (skipped, not multiplied by zero: the same bits as without the other leaves)
        assert np.array_equal(sums28(s, k), sums28(only, k))
    assert not np.any(s.H[0]) and not np.any(s.g[0]) and s.cost[0] == 0
    # each gate on its own
    loose = dict(min_points=1, min_poses=1, max_variance=None)
    for gate, unused in ((dict(min_poses=2), [0]), (dict(min_points=8), [1]), (dict(max_variance=1e-3), [2])):
        got = adjustment_system_np(block_moments_np(rows, [10, 11, 12], c), T, **{**loose, **gate}, leaves=True)
        assert np.nonzero(~got.leaves.used)[0].tolist() == unused


def test_adjust_np_recovers_the_poses(room):
    _, truth, bm = room
    system = lambda T: adjustment_system_np(bm, T, max_variance=ROOM_MAX_VARIANCE)
    first = system(None)
    assert 0 < first.n_leaves[1] < first.n_leaves[0]         # (the gate excludes the voxels on edges and corners)
    res = adjust_np(system, 4)
    assert_recovers(res, truth)
    assert np.array_equal(res.transforms[0], np.eye(4)) and res.pose_numbers == [0, 1, 2, 3]
    capped = adjust_np(system, 4, max_iterations=3)
    assert not capped.converged and capped.reason == "max_iterations" and capped.iterations == 3


def test_solve_fixes_the_gauge_and_refuses_starved_poses(room):
    _, _, bm = room
    s = adjustment_system_np(bm, None, max_variance=ROOM_MAX_VARIANCE)
    xi = s.solve()
    assert xi.shape == (4, 6) and not np.any(xi[0]) and np.all(np.any(xi[1:] != 0, axis=1))
    xi2 = s.solve(fixed=[1, 3])
    assert not np.any(xi2[1]) and not np.any(xi2[3]) and np.any(xi2[0]) and np.array_equal(xi2[2], xi[2])
    assert np.linalg.norm(s.solve(damping=1.0)[2]) < np.linalg.norm(xi[2])
    assert float(s.total_cost) == float(((s.cost[0] + s.cost[1]) + s.cost[2]) + s.cost[3])
    s.n_points = s.n_points.copy()
    s.n_points[2] = 5
    with pytest.raises(ValueError, match="pose 2"):
        s.solve()
    s.solve(fixed=[0, 2])       # (a fixed pose may be starved)
    starved = adjust_np(lambda T: s, 4)
    assert not starved.converged and starved.reason == "no correspondences" and starved.iterations == 0


def test_validation_of_transforms_and_origin(room):
    _, _, bm = room
    eye = np.stack([np.eye(4)] * 4)
    assert as_transforms(None, 2).shape == (2, 3, 4)
    assert np.array_equal(as_transforms(eye[:, :3], 4), as_transforms(eye, 4))
    for bad in (eye[:3], np.zeros((4, 3, 3)), eye * np.nan):
        with pytest.raises(ValueError):
            adjustment_system_np(bm, bad)
    broken = eye.copy()
    broken[1, 3] = [0.0, 0.0, 1.0, 1.0]
    with pytest.raises(ValueError, match="last row"):
        adjustment_system_np(bm, broken)
    for bad in ([0.0, 1.0], [0.0, np.inf, 0.0], "abc"):
        with pytest.raises(ValueError):
            adjustment_system_np(bm, None, origin=bad)
    bm_no_origin = block_moments_np([], [0, 1])
    with pytest.raises(ValueError, match="origin"):
        adjustment_system_np(bm_no_origin)
    empty = adjustment_system_np(bm_no_origin, None, [0.0, 0.0, 0.0])
    assert empty.H.shape == (2, 6, 6) and not np.any(empty.H) and empty.n_leaves == (0, 0)


def test_default_origin_and_tree_depth():
    assert np.array_equal(root_box_centre([[0, 0, 0], [2, 1, 0], [-1, 0, 3]], 1.0), [1.0, 1.0, 2.0])
    assert np.array_equal(root_box_centre([[1.0, 2.0, 3.0]], [4.0]), [3.0, 4.0, 5.0])
    assert [tree_depth(n) for n in (0, 1, 1024, 1025, 256 * 1024, 256 * 1024 + 1)] == [22, 23, 23, 23, 23, 24]


def test_plugged_grid_runs_through_the_host_map():
    from tests.test_cpu_registration import _plug_grid

    clouds, truth = room_scene(n=4000, seed=4)
    g = _plug_grid({p + 5: P for p, P in enumerate(clouds)})
    s = g.adjustment_system(max_variance=ROOM_MAX_VARIANCE, origin=ROOM_ORIGIN, leaves=True)
    assert s.pose_numbers == [5, 6, 7, 8] and 0 < s.n_leaves[1] < s.n_leaves[0]
    hm = g._host_map().adjustment_system(max_variance=ROOM_MAX_VARIANCE, origin=ROOM_ORIGIN)
    want = adjustment_system_np(block_moments_np(voxel_blocks(clouds), [5, 6, 7, 8]), None, ROOM_ORIGIN,
                                max_variance=ROOM_MAX_VARIANCE)
    for k in range(4):
        assert np.array_equal(sums28(s, k), sums28(hm, k))
        assert np.allclose(sums28(s, k), sums28(want, k), rtol=1e-9, atol=1e-12 * np.abs(want.H[k]).max())
    assert np.array_equal(s.n_points, want.n_points) and s.n_leaves == want.n_leaves
    # the default origin: the centre of the box of the top-level voxels, [0, 7) x [0, 6) x [0, 4)
    assert np.array_equal(g.adjustment_system().origin, [3.5, 3.0, 2.0])
    sub = g.adjustment_system(pose_numbers=[6, 8], max_variance=ROOM_MAX_VARIANCE)
    assert sub.pose_numbers == [6, 8] and sub.H.shape == (2, 6, 6)
    with pytest.raises(KeyError):
        g.adjustment_system(pose_numbers=[6, 99])
    res = g.adjust(max_variance=ROOM_MAX_VARIANCE, origin=ROOM_ORIGIN)
    assert_recovers(res, truth)
    same = g._host_map().adjust(max_variance=ROOM_MAX_VARIANCE, origin=ROOM_ORIGIN)
    assert np.array_equal(res.transforms, same.transforms) and res.iterations == same.iterations


def test_declared_bound_and_exported():
    import ctypes as C
    import os
    import re

    import octreelib_amd
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid
    from octreelib_amd.octree import Octree
    from octreelib_amd.octree_manager import OctreeManager

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"\s+", " ", open(os.path.join(root, "include", "octreelib_hip.h")).read())
    entries = {
        "octl_forest_adjustment_system":
            "int octl_forest_adjustment_system(octl_forest* f, const uint8_t* slot_sel, int32_t n_sel, "
            "const double* transforms, const double origin[3], int32_t min_points, int32_t min_poses, "
            "double max_variance, double* sums, int64_t* counts, int64_t n_leaves[2]);",
        "octl_forest_adjustment_tables":
            "int octl_forest_adjustment_tables(octl_forest* f, int64_t cap_leaves, int32_t* node, int64_t* count, "
            "double* mean, double* normal, double* lambda0, uint8_t* used, int64_t* n_leaves, int64_t cap_blocks, "
            "int32_t* blk_node, int32_t* blk_slot, double* blk_moments, int64_t* n_blocks);",
    }
    for name, decl in entries.items():
        assert decl in header, name
        assert nat.SIGNATURES[name][0] is C.c_int and len(nat.SIGNATURES[name][1]) == decl.count(",") + 1
    assert "#define OCTL_ABI_VERSION 1" in header
    for name in ("AdjustmentSystem", "Adjustment", "adjustment_system_np", "adjust_np"):
        assert name in octreelib_amd.__all__ and hasattr(octreelib_amd, name)
    for cls in (Grid, OctreeManager):
        assert callable(getattr(cls, "adjustment_system")) and callable(getattr(cls, "adjust"))
    assert not hasattr(Octree, "adjust") and not hasattr(Octree, "adjustment_system")
