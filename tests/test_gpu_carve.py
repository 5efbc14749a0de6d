"""carve on the device: octl_forest_carve / _carve_device and Grid / OctreeManager / Octree .carve / .carve_rays.

The checker is a second forest with the same poses and the same build that gets apply_host_mask with the mask worked
out on the host from octreelib_amd.query.carve_keep_np over its own block table: afterwards the two hold the same
block table, leaf-ordered points and permutation, and answer leaf_planes and nearest with the same bits."""

import numpy as np
import pytest

from octreelib_amd import MaxPoints, carve_keep_np, synthetic
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree_manager import OctreeManager
from octreelib_amd.query import evidence_inputs
from tests._evidence import assert_evidence_equal, evidence_of_nodes
from tests._raycast import box_rays

pytestmark = pytest.mark.gpu

CLOUDS = {p: synthetic.planar_cloud(4000, (2, 2, 2), seed=6, stream=p, sigma=0.002) for p in (0, 1, 2)}


def _grid(clouds=CLOUDS, K=48):
    g = Grid(GridConfig(voxel_edge_length=1))
    for p, P in clouds.items():
        g.insert_points(p, P)
    g.subdivide([MaxPoints(K)])
    return g


def _rays(seed=1, n=4000):
    rng = np.random.default_rng(seed)
    O, D = box_rays(rng, [0, 0, 0], [2, 2, 2], n, 0.5)
    return O, D, rng.uniform(0.3, 2.5, n)


def _point_mask(f, keep):
    """One byte per leaf-ordered point from one bool per block."""
    b = f.blocks
    mask = np.ones(f.n_ord, dtype=np.uint8)
    for s, z, k in zip(b["start"], b["size"], keep):
        mask[s:s + z] = k
    return mask


def _assert_same_map(a, b, what, Q):
    """Block table, leaf-ordered points, perm, point counts, leaf_planes and nearest of two grids."""
    fa, fb = a._forest, b._forest
    assert fa.n_ord == fb.n_ord, what
    for k in ("node", "slot", "start", "size"):
        assert np.array_equal(fa.blocks[k], fb.blocks[k]), (what, k)
    assert fa.xyz.tobytes() == fb.xyz.tobytes() and np.array_equal(fa.perm, fb.perm), what
    for p in a._slots:
        assert a.n_points(p) == b.n_points(p), (what, p)
    pa, pb = a.leaf_planes(), b.leaf_planes()
    for name in ("node", "count", "mean", "covariance", "eigenvalues", "eigenvectors"):
        assert getattr(pa, name).tobytes() == getattr(pb, name).tobytes(), (what, name)
    na, nb = a.nearest(Q, 4, max_distance=0.3), b.nearest(Q, 4, max_distance=0.3)
    for name in ("pose", "index", "distance2", "count"):
        assert getattr(na, name).tobytes() == getattr(nb, name).tobytes(), (what, name)


Q = np.ascontiguousarray(CLOUDS[0][:400] + 0.01)


def test_carve_is_apply_host_mask_of_the_keep_rule():
    O, D, r = _rays()
    for min_through, max_hits in ((2, 0), (1, 3), (5, 0)):
        a, b = _grid(), _grid()
        ev = a.ray_evidence(O, D, r, 0.05)
        assert_evidence_equal(b.ray_evidence(O, D, r, 0.05), ev, "two builds of one map")
        before = a._forest.n_ord
        removed = a.carve(ev, min_through, max_hits)
        fb = b._forest
        keep = carve_keep_np(fb.blocks["node"], fb.blocks["slot"], ev.through, ev.hits, None, min_through, max_hits)
        assert 0 < (~keep).sum() < len(keep), (min_through, max_hits)
        fb.apply_host_mask(_point_mask(fb, keep))
        assert removed == before - fb.n_ord > 0
        _assert_same_map(a, b, f"carve({min_through}, {max_hits})", Q)
        # every emptied node is free under the rule, and holds nothing now
        held = np.bincount(a._forest.blocks["node"], minlength=len(ev))
        assert held[ev.free(min_through, max_hits)].sum() == 0
        # the scheme stays: the evidence of the same rays is the same
        assert_evidence_equal(a.ray_evidence(O, D, r, 0.05), ev, "after carve")
        # nothing left to remove
        assert a.carve(ev, min_through, max_hits) == 0


def test_pose_numbers_only_those_poses_lose_points():
    O, D, r = _rays(2)
    a, b = _grid(), _grid()
    ev = a.ray_evidence(O, D, r, 0.05)
    pts = {p: a.get_points(p).copy() for p in CLOUDS}
    removed = a.carve(ev, pose_numbers=[2, 0])
    fb = b._forest
    sel = np.zeros(fb.n_slots, dtype=np.uint8)
    sel[[b._slots[2], b._slots[0]]] = 1
    keep = carve_keep_np(fb.blocks["node"], fb.blocks["slot"], ev.through, ev.hits, sel)
    fb.apply_host_mask(_point_mask(fb, keep))
    _assert_same_map(a, b, "carve, poses 2 and 0", Q)
    assert removed == sum(len(pts[p]) - a.n_points(p) for p in (0, 2)) > 0
    assert a.n_points(0) < len(pts[0]) and a.n_points(2) < len(pts[2])
    assert a.get_points(1).tobytes() == pts[1].tobytes()                # bits and order of the other pose
    with pytest.raises(KeyError):
        a.carve(ev, pose_numbers=[4])
    # refusals: evidence of another scheme, bad thresholds, a selection of the wrong length at the ABI
    from octreelib_amd import RayEvidence
    from octreelib_amd import _native as nat

    with pytest.raises(ValueError, match="nodes"):
        a.carve(RayEvidence(ev.through[:-1], ev.hits[:-1]))
    for bad in ((0, 0), (2, -1)):
        with pytest.raises(ValueError):
            a.carve(ev, *bad)
    f = a._forest
    N = len(ev)
    abi = lambda n_nodes, s, n_sel, mt, mh: f.lib.octl_forest_carve(f.handle, nat.ptr(ev.through), nat.ptr(ev.hits),
                                                                    n_nodes, nat.ptr(s), n_sel, mt, mh, None)
    n0 = f.n_ord
    assert abi(N - 1, None, 0, 2, 0) == nat.OCTL_E_INVALID and abi(N, sel, 2, 2, 0) == nat.OCTL_E_INVALID
    assert abi(N, None, 0, 0, 0) == nat.OCTL_E_INVALID and abi(N, None, 0, 2, -1) == nat.OCTL_E_INVALID
    assert f.lib.octl_forest_carve(f.handle, None, nat.ptr(ev.hits), N, None, 0, 2, 0, None) == nat.OCTL_E_INVALID
    assert f.lib.octl_forest_carve_device(f.handle, None, None, N, None, 0, 2, 0, None) == nat.OCTL_E_INVALID
    assert a.n_points(0) + a.n_points(1) + a.n_points(2) == n0


def test_a_pending_ransac_mask_goes_into_the_same_compaction():
    O, D, r = _rays(3)
    a, b = _grid(), _grid()
    ev = a.ray_evidence(O, D, r, 0.05)
    masks = []
    for g in (a, b):
        f = g._forest
        np.random.seed(0)
        f.ransac_blocks(np.ascontiguousarray(f.order), np.random.random((128, 6)), 0.01)
        masks.append(f.device_mask())
    assert np.array_equal(masks[0], masks[1]) and 0 < masks[0].sum() < len(masks[0])
    before = a._forest.n_ord
    removed = a.carve(ev, 2, 0, pose_numbers=[0, 1])
    fb = b._forest
    sel = np.zeros(fb.n_slots, dtype=np.uint8)
    sel[[b._slots[0], b._slots[1]]] = 1
    keep = carve_keep_np(fb.blocks["node"], fb.blocks["slot"], ev.through, ev.hits, sel, 2, 0)
    both = masks[1] & _point_mask(fb, keep)
    assert both.sum() < masks[1].sum() and both.sum() < _point_mask(fb, keep).sum()      # each mask removes something
    fb.apply_host_mask(both)
    assert removed == before - fb.n_ord
    _assert_same_map(a, b, "carve with a pending RANSAC mask", Q)


def test_carve_rays_is_ray_evidence_then_carve_and_the_map_lives_on():
    O, D, r = _rays(4)
    ret = np.random.default_rng(4).random(len(O)) > 0.2
    a, b = _grid(), _grid()
    ev = b.ray_evidence(O, D, r, 0.05, 0.2, ret)
    want = b.carve(ev, 2, 1, pose_numbers=[0])
    assert a.carve_rays(O, D, r, 0.05, 0.2, ret, 2, 1, pose_numbers=[0]) == want > 0
    _assert_same_map(a, b, "carve_rays", Q)
    # a later subdivide and RANSAC run on the carved map, the same on both
    for g in (a, b):
        g.subdivide([MaxPoints(20)])
        np.random.seed(2)
        g.map_leaf_points_cuda_ransac(poses_per_batch=3, threshold=0.01, hypotheses_number=128, initial_points_number=6)
    assert 0 < a._forest.n_ord < 12000 - want
    _assert_same_map(a, b, "subdivide and RANSAC after carve", Q)
    # the other classes: a manager with pose numbers, a bare octree
    rng = np.random.default_rng(5)
    m = OctreeManager(Octree, OctreeConfig(), np.array([0.0, 0.0, 0.0]), 2.0)
    for p, P in CLOUDS.items():
        m.insert_points(2 * p + 3, P)                        # (pose numbers 3, 5, 7: not the slots)
    m.subdivide([MaxPoints(48)])
    n5 = m.n_points(5)
    evm = m.ray_evidence(O, D, r, 0.05)
    inp = evidence_inputs(O, D, r, 0.05)
    assert_evidence_equal(evm, evidence_of_nodes(m._forest.nodes, *inp), "manager")
    assert m.carve(evm, pose_numbers=[5]) == n5 - m.n_points(5) > 0
    t = Octree(OctreeConfig(), np.array([0.0, 0.0, 0.0]), 2.0)
    t.insert_points(CLOUDS[0])
    t.subdivide([MaxPoints(48)])
    n0 = t.n_points
    got = t.carve_rays(O, D, r, 0.05)
    assert got == n0 - t.n_points > 0


def _scenario():
    """Pose 0: a wall at x = 3 and a blob in front of it; pose 1 sees the wall alone, through the blob's place."""
    rng = np.random.default_rng(10)
    yz = rng.uniform(0.0, 2.0, (3000, 2))
    wall0 = np.column_stack([3.0 + rng.uniform(0.0, 0.02, 3000), yz])
    blob = np.array([1.5, 1.0, 1.0]) + rng.uniform(-0.1, 0.1, (300, 3))
    wall1 = np.column_stack([3.0 + rng.uniform(0.0, 0.02, 3000), yz + rng.uniform(-1e-3, 1e-3, (3000, 2))])
    sensor = np.array([0.25, 1.0, 1.0])
    return np.concatenate([wall0, blob]), wall1, blob, wall0, sensor


def test_scenario_a_blob_that_moved_away_is_carved_and_the_wall_stays():
    pose0, wall1, blob, wall0, sensor = _scenario()
    g = _grid({0: pose0, 1: wall1}, 32)
    f = g._forest
    D = wall1 - sensor
    O = np.tile(sensor, (len(D), 1))
    r = np.sqrt((D * D).sum(axis=1))
    margin = 0.05
    # what the definition alone says about this geometry (tests/test_cpu_evidence.py has its cases)
    ref = evidence_of_nodes(f.nodes, *evidence_inputs(O, D, r, margin))
    blob_leaves = np.unique(f.locate(blob))
    wall_leaves = np.unique(f.locate(wall0))
    assert blob_leaves.min() >= 0 and wall_leaves.min() >= 0 and len(blob_leaves) >= 4
    assert np.all(ref.through[blob_leaves] >= 2) and np.all(ref.hits[blob_leaves] == 0)
    assert np.all(ref.hits[wall_leaves] >= 1)
    ev = g.ray_evidence(O, D, r, margin)
    assert_evidence_equal(ev, ref, "scenario")
    def held(slot):
        b = f.blocks
        m = b["slot"] == slot
        return np.bincount(b["node"][m], weights=b["size"][m], minlength=len(ref)).astype(np.int64)

    before0, before1 = held(g._slots[0]), held(g._slots[1])
    assert before0[blob_leaves].sum() == len(blob)
    removed = g.carve(ev, pose_numbers=[0])
    after0, after1 = held(g._slots[0]), held(g._slots[1])
    assert removed == len(blob) and after0[blob_leaves].sum() == 0
    assert np.array_equal(after0[wall_leaves], before0[wall_leaves]) and np.array_equal(after1, before1)
    assert g.n_points(0) == len(wall0) and g.n_points(1) == len(wall1)
