"""Nearest-point-to-plane registration on the host: registration.nearest_plane_registration_system_np (the definition
of octl_forest_nearest_plane_registration_system), align_np over it, the module-level functions of
octreelib_amd.matching on the caller's own plug types, and the scene of the gap the feature closes.

The scene of the gap (gap_scene): three mutually orthogonal, noise-free rectangular patches of 2 x 2, more than 1.8
apart (so no top-level voxel of edge 1 holds points of two of them, and no query within max_distance of one patch
finds a point of another); the map is two poses of ONE random sample of 4000 points per patch, subdivided by
MaxPoints(24) into leaves of edge 1/8 and below (a few of 1/4 at the rim of a patch); the scan is ANOTHER random
sample of the same patches under a rigid motion whose translation is at least 0.32 along every patch normal - more
than two leaf edges - and whose rotation is 0.02 rad.  max_distance = 0.75 covers the displacement (at most 0.63; the
test prints it).  At the true pose every residual is zero whichever stored point is matched, so the fixed point of the
new system is the truth; the point-to-point system has its fixed point where the two samplings balance, and the
own-leaf system finds no plane at the start."""

import os
import re

import numpy as np
import pytest

import octreelib_amd
from octreelib_amd import MaxPoints
from octreelib_amd import registration as reg
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree.octree_base import OctreeConfigBase
from octreelib_amd.query import Neighbours, nearest_np, point_to_plane_np
from octreelib_amd.registration import (align_np, nearest_plane_registration_system_np, point_registration_system_np,
                                        registration_system_np, se3_exp, transform_np)
from tests.test_cpu_point_registration import sums28
from tests.test_cpu_query import HostManager, HostOctree

GAP_R = 0.75                 # max_distance
GAP_LEAF = 24                # MaxPoints of the subdivision
GAP_CENTRE = [1.6, 1.6, 1.5]
GAP_MOTION = (0.012, -0.01, 0.012, 0.34, -0.33, 0.32)     # |rotation| = 0.02 rad; the translation crosses every patch
GAP_OFFSETS = (0.31, 3.31, 3.31)                          # z of patch 0, x of patch 1, y of patch 2


def _patches(rng, n):
    """n points on each of the three patches: z = 0.31 over [0, 2]^2; x = 3.31 over y in [0, 2], z in [1.7, 3.7];
    y = 3.31 over x in [0, 2], z in [1.7, 3.7]."""
    u = rng.uniform(0.0, 2.0, (3, n, 2))
    a = np.stack([u[0, :, 0], u[0, :, 1], np.full(n, GAP_OFFSETS[0])], axis=1)
    b = np.stack([np.full(n, GAP_OFFSETS[1]), u[1, :, 0], 1.7 + u[1, :, 1]], axis=1)
    c = np.stack([u[2, :, 0], np.full(n, GAP_OFFSETS[2]), 1.7 + u[2, :, 1]], axis=1)
    return [a, b, c]


def gap_scene(n_map=4000, n_scan=400):
    """(clouds [(0, P0), (1, P1)], scan Q, T_true, patch of every scan point): transform_np(T_true, Q) lies on the
    patches (to rounding), sampled independently of the map."""
    rng = np.random.default_rng(21)
    P = np.concatenate(_patches(rng, n_map))
    P = P[rng.permutation(len(P))]
    clouds = [(0, np.ascontiguousarray(P[0::2])), (1, np.ascontiguousarray(P[1::2]))]
    S = np.concatenate(_patches(np.random.default_rng(22), n_scan))
    T_true = se3_exp(GAP_MOTION, GAP_CENTRE)
    Q = transform_np(np.linalg.inv(T_true), S)
    return clouds, np.ascontiguousarray(Q), T_true, np.repeat(np.arange(3), n_scan)


def plug_grid(clouds, leaf, edge=1):
    """A Grid on the caller's own plug types holding `clouds`, subdivided by MaxPoints(leaf).  (The voxel bucketing of
    the plug path's insert_points runs on the device: done in NumPy here, as tests/test_cpu_query.py does.)"""
    g = Grid(GridConfig(octree_manager_type=HostManager, octree_type=HostOctree, octree_config=OctreeConfigBase(),
                        voxel_edge_length=edge))
    for pose, P in clouds:
        vox = (np.floor_divide(P, float(edge)) * edge).astype(int)
        uniq, inv = np.unique(vox, axis=0, return_inverse=True)
        g._plug._pose_voxels[pose] = []
        for j, coords in enumerate(uniq):
            key = tuple(int(x) for x in coords)
            if key not in g._plug._managers:
                g._plug._managers[key] = HostManager(HostOctree, OctreeConfigBase(), np.array(coords), edge)
            g._plug._pose_voxels[pose].append(key)
            g._plug._managers[key].insert_points(pose, P[inv.reshape(-1) == j])
    g.subdivide([MaxPoints(leaf)])
    return g


def assert_gap_geometry(clouds, Q, T_true, patch, node_of, edge_of_node):
    """What the scene promises, for the scheme at hand (node_of: points -> leaf ids, edge_of_node: (N,) edges)."""
    P = np.concatenate([a for _, a in clouds])
    which = np.select([P[:, 2] == GAP_OFFSETS[0], P[:, 0] == GAP_OFFSETS[1]], [0, 1], 2)
    # the patches are further apart than max_distance plus the largest displacement of a scan point
    moved = np.linalg.norm(Q - transform_np(T_true, Q), axis=1).max()
    for a in range(3):
        for b in range(a + 1, 3):
            A, B = P[which == a][::7], P[which == b][::7]
            gap = np.sqrt(((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2).min())
            assert gap > 1.8 > GAP_R + moved, (a, b, gap, moved)
    assert moved < GAP_R
    # the leaves that hold points are several times smaller than the shift across every patch
    # (edge 1/8 and below; a few leaves of 1/4 at the rim of a patch, where a cube is mostly empty)
    edges = edge_of_node[node_of(P)]
    print("points per leaf edge:", {float(e): int((edges == e).sum()) for e in np.unique(edges)})
    leaf = 0.125
    assert edges.max() <= 2 * leaf and (edges <= leaf).mean() >= 0.98
    t = T_true[:3, 3] - (np.asarray(GAP_CENTRE) - T_true[:3, :3] @ np.asarray(GAP_CENTRE))      # v of the motion
    assert np.all(np.abs(t) >= 2 * leaf)
    # ... for every scan point, rotation included: the start is at least two leaf edges off its plane
    axis = np.array([2, 0, 1])[patch]
    off = np.abs(Q[np.arange(len(Q)), axis] - np.asarray(GAP_OFFSETS)[patch])
    print(f"scan points start {off.min():.3f} .. {off.max():.3f} off their planes, moved by up to {moved:.3f}")
    assert off.min() >= 2 * leaf, off.min()


@pytest.fixture(scope="module")
def gap():
    clouds, Q, T_true, patch = gap_scene()
    g = plug_grid(clouds, GAP_LEAF)
    return g, g._host_map(), clouds, Q, T_true, patch


# ---- the composition -----------------------------------------------------------------------------------------------
def _fields_equal(a, b):
    assert sums28(a).tobytes() == sums28(b).tobytes() and (a.n_used, a.n_located) == (b.n_used, b.n_located)
    assert np.array_equal(a.origin, b.origin)
    for name in ("node", "row"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(np.asarray(a.residual).view(np.uint64), np.asarray(b.residual).view(np.uint64))


@pytest.mark.parametrize("sel", [None, [1]])
@pytest.mark.parametrize("delta", [None, 0.03])
def test_the_definition_is_a_composition(gap, sel, delta):
    _, hm, clouds, Q, T_true, _ = gap
    rng = np.random.default_rng(3)
    Qn = np.concatenate([Q + rng.normal(0.0, 0.01, Q.shape), [[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [50.0, 0.0, 0.0]]])
    T = se3_exp([0.004, -0.003, 0.002, 0.03, 0.02, -0.04], GAP_CENTRE) @ T_true
    c = np.array(GAP_CENTRE)
    chosen, planes, r, mv = hm.clouds(sel), hm.leaf_planes(sel), 0.2, 1e-6
    s = nearest_plane_registration_system_np(hm.locate, planes, chosen, Qn, T, c, max_distance=r, min_points=4,
                                             max_variance=mv, huber_delta=delta, per_point=True)
    # by hand: nearest_np, locate of the MATCHED point, point_to_plane_np of the QUERY, registration_system_np
    p = transform_np(T, Qn)
    nb = nearest_np(p, chosen, 1, max_distance=r)
    has = nb.count > 0
    m = np.zeros((len(p), 3))
    for k, a in chosen:
        of = has & (nb.pose[:, 0] == k)
        m[of] = a[nb.index[of, 0]]
    node = np.where(has, hm.locate(m), -1).astype(np.int32)
    row, res = point_to_plane_np(node, planes, p, 4, mv)
    hand = registration_system_np(None, planes, Qn, T, c, 4, mv, None, delta, answers=(node, row, res),
                                  per_point=True)
    _fields_equal(s, hand)
    assert isinstance(s.neighbours, Neighbours) and s.planes is planes
    for name in ("pose", "index", "distance2", "count"):
        assert np.array_equal(getattr(s.neighbours, name), getattr(nb, name)), name
    # ... and itself with answers=
    again = nearest_plane_registration_system_np(None, planes, None, Qn, T, c, max_distance=r, min_points=4,
                                                 max_variance=mv, huber_delta=delta, per_point=True,
                                                 answers=(s.neighbours, s.node, s.row, s.residual))
    _fields_equal(again, s)
    # every class of query is there: unmatched, matched without an accepted plane, used; n_located counts the matched
    assert s.n_located == int(has.sum()) == int((s.node >= 0).sum()) and 0 < s.n_used < s.n_located < len(Qn)
    assert np.all(np.isnan(s.residual[s.row < 0])) and np.all(np.isfinite(s.residual[s.row >= 0]))
    assert not has[-3:].any() and np.all(np.isfinite(sums28(s)))
    if delta is not None:
        assert 20 < (np.abs(s.residual[s.row >= 0]) > delta).sum() < s.n_used - 20      # (Huber bites, and not everywhere)
    # where the query's own leaf is the matched point's leaf, residual and row are those of point_to_plane_np(locate(p))
    own = hm.locate(p)
    same = has & (own == s.node)
    assert 50 < same.sum() < has.sum()              # (and elsewhere the leaf of the match is another one)
    row_own, res_own = point_to_plane_np(own, planes, p, 4, mv)
    assert np.array_equal(s.row[same], row_own[same])
    assert np.array_equal(s.residual[same].view(np.uint64), res_own[same].view(np.uint64))
    # the HostMap runs the same
    got = hm.nearest_plane_registration_system(Qn, T, max_distance=r, pose_numbers=sel, min_points=4, max_variance=mv,
                                               huber_delta=delta, origin=c, per_point=True)
    _fields_equal(got, s)


# ---- the gap -----------------------------------------------------------------------------------------------------------
def test_the_gap(gap):
    _, hm, clouds, Q, T_true, patch = gap
    assert_gap_geometry(clouds, Q, T_true, patch, hm.locate, hm.nodes["edge"])
    planes = hm.leaf_planes()
    err = lambda a: float(np.abs(a.transform - T_true).max())
    # (a) nearest point, plane of its leaf: converges to the truth
    a = align_np(lambda T, c: nearest_plane_registration_system_np(hm.locate, planes, clouds, Q, T, c,
                                                                   max_distance=GAP_R))
    print(f"nearest-plane: {a.iterations} iterations, {a.reason}, n_used {a.n_used}, error {err(a):.2e}, costs {a.costs}")
    assert a.converged and a.n_used > 0.7 * len(Q) and err(a) <= 1e-9
    assert a.costs[-1] <= 1e-20
    # (b) the plane of the query's own leaf: nothing to hold on to at this start
    s0 = registration_system_np(hm.locate, planes, Q)
    b = align_np(lambda T, c: registration_system_np(hm.locate, planes, Q, T, c))
    print(f"own leaf: n_used at the start {s0.n_used}, {b.iterations} iterations, {b.reason}, error {err(b):.2e}")
    assert s0.n_used < 6 or err(b) > 1e-3
    # (c) point to point: ends where the two samplings balance, not at the truth
    p = align_np(lambda T, c: point_registration_system_np(clouds, Q, T, c, max_distance=GAP_R))
    print(f"point to point: {p.iterations} iterations, {p.reason}, error {err(p):.2e}")
    assert err(p) > 1e-6
    # the HostMap's loop is the same loop
    h = hm.align_nearest_planes(Q, max_distance=GAP_R)
    assert h.transform.tobytes() == a.transform.tobytes() and h.iterations == a.iterations


# ---- the public functions on the plug types ----------------------------------------------------------------------------
def test_plug_types_answer_through_the_host_map(gap):
    from octreelib_amd import align_nearest_planes, nearest_plane_registration_system
    g, hm, clouds, Q, T_true, _ = gap
    s = nearest_plane_registration_system(g, Q, T_true, max_distance=GAP_R, per_point=True)
    ref = hm.nearest_plane_registration_system(Q, T_true, max_distance=GAP_R, per_point=True)
    _fields_equal(s, ref)
    assert s.n_located == len(Q) and s.n_used > 0.7 * len(Q) and s.cost < 1e-25
    one = nearest_plane_registration_system(g, Q, T_true, max_distance=GAP_R, pose_numbers=[1], min_points=4,
                                            huber_delta=0.01, origin=GAP_CENTRE)
    ref1 = hm.nearest_plane_registration_system(Q, T_true, max_distance=GAP_R, pose_numbers=[1], min_points=4,
                                                huber_delta=0.01, origin=GAP_CENTRE)
    assert sums28(one).tobytes() == sums28(ref1).tobytes() and (one.n_used, one.n_located) == (ref1.n_used, len(Q))
    a = align_nearest_planes(g, Q, max_distance=GAP_R)
    assert a.converged and np.abs(a.transform - T_true).max() <= 1e-9
    with pytest.raises(KeyError):
        nearest_plane_registration_system(g, Q, max_distance=GAP_R, pose_numbers=[9])
    with pytest.raises(TypeError):
        align_nearest_planes(g, Q)                                   # (max_distance is required)
    with pytest.raises(ValueError, match="voxel edge"):
        nearest_plane_registration_system(g, Q, max_distance=2.5)
    with pytest.raises(ValueError, match="voxel edge"):
        align_nearest_planes(g, Q, max_distance=2.5)
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            nearest_plane_registration_system(g, Q, max_distance=r)
    # an OctreeManager on plug types: one cube, pose numbers that are not slots
    m = HostManager(HostOctree, OctreeConfigBase(), np.array([0.0, 0.0, 0.0]), 4.0)
    for k, (_, P) in zip((4, 9), clouds):
        m.insert_points(k, P)
    m.subdivide([MaxPoints(GAP_LEAF)])
    sm = nearest_plane_registration_system(m, Q, T_true, max_distance=GAP_R, per_point=True)
    assert {4, 9} <= set(np.unique(sm.neighbours.pose).tolist()) and sm.n_located == len(Q) and sm.cost < 1e-25
    assert nearest_plane_registration_system(m, Q, T_true, max_distance=GAP_R, pose_numbers=[9]).n_located == len(Q)
    am = align_nearest_planes(m, Q, max_distance=GAP_R, pose_numbers=[4, 9])
    assert am.converged and np.abs(am.transform - T_true).max() <= 1e-9


def test_refusals_of_the_functions():
    from octreelib_amd import align_nearest_planes, nearest_plane_registration_system
    from octreelib_amd.octree import Octree
    Q = np.zeros((4, 3))
    for bad in (None, object(), "grid", np.zeros((3, 3))):
        with pytest.raises(TypeError, match="Grid, an OctreeManager or an Octree"):
            nearest_plane_registration_system(bad, Q, max_distance=0.1)
        with pytest.raises(TypeError, match="Grid, an OctreeManager or an Octree"):
            align_nearest_planes(bad, Q, max_distance=0.1)
    # an Octree holds one pose: pose_numbers is refused before anything is touched (no device is needed to say so)
    t = object.__new__(Octree)
    with pytest.raises(ValueError, match="pose_numbers"):
        nearest_plane_registration_system(t, Q, max_distance=0.1, pose_numbers=[0])
    with pytest.raises(ValueError, match="pose_numbers"):
        align_nearest_planes(t, Q, max_distance=0.1, pose_numbers=[0])
    with pytest.raises(TypeError):
        nearest_plane_registration_system_np(lambda p: None, None, [], Q)        # (max_distance is required)
    # no query, no match: zeros, +0.0
    e = nearest_plane_registration_system_np(lambda p: np.empty(0, np.int32), _no_planes(), [(0, np.zeros((1, 3)))],
                                             np.empty((0, 3)), max_distance=1.0)
    assert e.n_used == 0 and e.n_located == 0 and not sums28(e).any() and not np.signbit(sums28(e)).any()


def _no_planes():
    from octreelib_amd.query import pooled_leaf_statistics_np
    return pooled_leaf_statistics_np([])


def test_exports_and_abi_text():
    for name in ("nearest_plane_registration_system_np", "nearest_plane_registration_system", "align_nearest_planes"):
        assert name in octreelib_amd.__all__ and hasattr(octreelib_amd, name)
    assert "nearest_plane_registration_system_np" in reg.__all__
    assert octreelib_amd.nearest_plane_registration_system_np is nearest_plane_registration_system_np
    from octreelib_amd import matching
    assert octreelib_amd.align_nearest_planes is matching.align_nearest_planes
    assert sorted(matching.__all__) == ["align_nearest_planes", "nearest_plane_registration_system"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"\s+", " ", open(os.path.join(root, "include", "octreelib_hip.h")).read())
    from octreelib_amd import _native as nat
    for name in ("octl_forest_nearest_plane_registration_system", "octl_forest_nearest_plane_registration_system_device"):
        assert f"int {name}(octl_forest* f," in header
        restype, args = nat.SIGNATURES[name]
        assert len(args) == 19
    assert "#define OCTL_ABI_VERSION 1" in header
    # the classes keep their surface: the operation is a function, not a method
    for cls, mod in (("Grid", "octreelib_amd.grid"), ("OctreeManager", "octreelib_amd.octree_manager"),
                     ("Octree", "octreelib_amd.octree")):
        c = getattr(__import__(mod, fromlist=[cls]), cls)
        assert not hasattr(c, "nearest_plane_registration_system") and not hasattr(c, "align_nearest_planes")
