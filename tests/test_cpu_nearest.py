"""nearest_np, the brute-force definition of the neighbour query (octreelib_amd/query.py), and HostMap.nearest - what a
grid on the caller's own plug types answers with.  No GPU: the device kernel is compared with nearest_np bit for bit in
tests/test_gpu_nearest.py."""

import math

import numpy as np
import pytest

import octreelib_amd
from octreelib_amd import MaxPoints, Neighbours, nearest_np
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree.octree_base import OctreeConfigBase
from octreelib_amd.query import NN_MAX_K, HostMap
from tests.test_cpu_query import HostManager, HostOctree


def lattice_case():
    """The tie case of the issue: the lattice {0, 1/8, .., 15/8}^3 as pose 0, every third lattice point again as pose 1,
    every seventh lattice point as a query, k = 8, r = 1/8.  Every coordinate and every d2 is exact in f64."""
    t = np.arange(16) / 8.0
    P0 = np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(-1, 3)
    return P0, P0[::3].copy(), P0[::7].copy(), 8, 0.125


def assert_lattice_situations(res: Neighbours, k, r):
    """The three situations the lattice exists for all occur: neighbours exactly on the radius, full rows with a tie
    at the k-th place (the (k+1)-th candidate has the same d2, so (slot, index) decided), and rows that are not full."""
    r2 = r * r
    assert (res.distance2 == r2).sum() > 1000
    full = res.count == k
    assert (full & (res.distance2[:, k - 1] == r2)).sum() > 100      # (more than k candidates end on the radius there)
    assert (~full).sum() > 10 and (res.count > 0).all()


def _python_reference(Q, clouds, k, r):
    r2 = r * r
    out = []
    for q in Q.tolist():
        cand = []
        if all(math.isfinite(x) for x in q):
            for s, (_, P) in enumerate(clouds):
                for j, p in enumerate(P.tolist()):
                    dx, dy, dz = q[0] - p[0], q[1] - p[1], q[2] - p[2]
                    d2 = (dx * dx + dy * dy) + dz * dz
                    if d2 <= r2:
                        cand.append((d2, s, j))
        out.append(sorted(cand)[:k])
    return out


def test_nearest_np_against_a_python_loop():
    rng = np.random.default_rng(1)
    clouds = [(4, rng.random((1200, 3))), (9, rng.random((800, 3)))]
    # duplicates across and inside the poses: ties that only (slot, index) can order
    clouds[1][1][:50] = clouds[0][1][:50]
    clouds[0][1][100:120] = clouds[0][1][200:220]
    Q = np.concatenate([rng.random((250, 3)), clouds[0][1][:30], clouds[0][1][200:220]])
    assert len(Q) == 300
    names = [4, 9]
    for k, r in ((1, 0.05), (3, 0.1), (8, 0.1)):
        res = nearest_np(Q, clouds, k, max_distance=r)
        ref = _python_reference(Q, clouds, k, r)
        assert res.pose.dtype == np.int32 and res.index.dtype == np.int64 and res.distance2.dtype == np.float64
        assert res.count.dtype == np.int32 and res.pose.shape == res.index.shape == res.distance2.shape == (300, k)
        for i, row in enumerate(ref):
            c = len(row)
            assert res.count[i] == c
            assert res.distance2[i, :c].tolist() == [d for d, _, _ in row]
            assert res.pose[i, :c].tolist() == [names[s] for _, s, _ in row]
            assert res.index[i, :c].tolist() == [j for _, _, j in row]
            assert np.all(res.pose[i, c:] == -1) and np.all(res.index[i, c:] == -1)
            assert np.all(np.isposinf(res.distance2[i, c:]))
        assert (res.count < k).any() and (res.count == k).any()
    # the chunking does not show
    a, b = nearest_np(Q, clouds, 8, max_distance=0.1, chunk=7), nearest_np(Q, clouds, 8, max_distance=0.1)
    assert all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("pose", "index", "distance2", "count"))


class _Leaf:
    def __init__(self, corner, edge, points):
        self.corner_min, self.edge_length, self._p = corner, edge, points

    def get_points(self):
        return self._p


def test_lattice_ties_and_inclusive_radius():
    P0, P1, Q, k, r = lattice_case()
    assert len(P0) == 4096 and len(Q) == 586
    res = nearest_np(Q, [(0, P0), (1, P1)], k, max_distance=r)
    assert_lattice_situations(res, k, r)
    # ties: pose 0 before pose 1, ascending index inside a pose
    for i in (0, 100, 585):
        c = res.count[i]
        key = list(zip(res.distance2[i, :c].tolist(), res.pose[i, :c].tolist(), res.index[i, :c].tolist()))
        assert key == sorted(key)
    # the query itself (d2 = 0) comes first, from pose 0; every third query is also a point of pose 1
    assert np.all(res.distance2[:, 0] == 0.0) and np.all(res.pose[:, 0] == 0)
    assert np.array_equal(res.index[:, 0], np.arange(0, 4096, 7))
    twice = (np.arange(0, 4096, 7) % 3) == 0
    assert np.all(res.pose[twice, 1] == 1) and np.all(res.distance2[twice, 1] == 0.0)
    assert np.array_equal(res.index[twice, 1], np.arange(0, 4096, 7)[twice] // 3)
    # ... and through a HostMap whose leaves are the eight unit voxels: the indices refer to the leaves' concatenation,
    # every other column is the same
    vox = np.floor(P0).astype(int)
    roots, leaves = [], {0: [], 1: []}
    for key in sorted({tuple(v) for v in vox.tolist()}):
        c = np.array(key, dtype=np.float64)
        roots.append((c, 1.0))
        for p, P in ((0, P0), (1, P1)):
            leaves[p].append(_Leaf(c, 1.0, P[np.all(np.floor(P).astype(int) == key, axis=1)]))
    hm = HostMap(0, 1.0, roots, leaves)
    got = hm.nearest(Q, k, max_distance=r)
    assert np.array_equal(got.count, res.count) and np.array_equal(got.distance2, res.distance2)
    assert np.array_equal(got.pose, res.pose)
    # (which of several tied points of one pose is kept depends on the numbering: the answer is checked against the
    #  definition on the HostMap's own numbering, and every returned index names a point at the returned distance)
    own = nearest_np(Q, hm.clouds(), k, max_distance=r)
    assert np.array_equal(got.index, own.index) and not np.array_equal(got.index, res.index)
    stored = dict(hm.clouds())
    for p in (0, 1):
        i, j = np.nonzero(got.pose == p)
        d = Q[i] - stored[p][got.index[i, j]]
        assert np.array_equal((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], got.distance2[i, j])
    only1 = hm.nearest(Q, k, max_distance=r, pose_numbers=[1])
    assert np.all(only1.pose[only1.pose >= 0] == 1) and only1.count.sum() < res.count.sum()


def test_plug_grid_nearest_on_the_host():
    rng = np.random.default_rng(12)
    g = Grid(GridConfig(octree_manager_type=HostManager, octree_type=HostOctree, octree_config=OctreeConfigBase(),
                        voxel_edge_length=2))
    clouds = {0: rng.uniform(-2, 4, (2500, 3)) * [1, 1, 0.2], 1: rng.uniform(0, 4, (1200, 3))}
    # (the voxel bucketing of the plug path's insert_points runs on the device: done in NumPy here, as
    #  tests/test_cpu_query.py does)
    for pose, P in clouds.items():
        vox = (np.floor_divide(P, 2.0) * 2).astype(int)
        uniq, inv = np.unique(vox, axis=0, return_inverse=True)
        g._plug._pose_voxels[pose] = []
        for j, coords in enumerate(uniq):
            key = tuple(int(c) for c in coords)
            if key not in g._plug._managers:
                g._plug._managers[key] = HostManager(HostOctree, OctreeConfigBase(), np.array(coords), 2)
            g._plug._pose_voxels[pose].append(key)
            g._plug._managers[key].insert_points(pose, P[inv.reshape(-1) == j])
    g.subdivide([MaxPoints(40)])
    Q = np.concatenate([clouds[1][:300] + 0.01, [[np.nan, 0.0, 0.0], [50.0, 0.0, 0.0]]])
    got = g.nearest(Q, 4, max_distance=0.3)
    ref = nearest_np(Q, [(0, clouds[0]), (1, clouds[1])], 4, max_distance=0.3)
    assert isinstance(got, Neighbours)
    assert np.array_equal(got.count, ref.count) and np.array_equal(got.distance2, ref.distance2)
    assert np.array_equal(got.pose, ref.pose) and got.count[-2:].tolist() == [0, 0] and (got.count == 4).any()
    one = g.nearest(Q, 4, max_distance=0.3, pose_numbers=[1])
    ref1 = nearest_np(Q, [(1, clouds[1])], 4, max_distance=0.3)
    assert np.array_equal(one.distance2, ref1.distance2) and np.array_equal(one.pose, ref1.pose)
    with pytest.raises(KeyError):
        g.nearest(Q, 1, max_distance=0.3, pose_numbers=[5])
    with pytest.raises(ValueError):
        g.nearest(Q, 1, max_distance=4.5)            # more than twice the voxel edge
    with pytest.raises(TypeError):
        g.nearest(Q, 1)                              # max_distance is required


def test_padding_bad_queries_empty_input_and_argument_errors():
    P = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0]])
    Q = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [1e300, 0.0, 0.0],
                  [10.0, 10.0, 10.0], [0.5, 0.0, 0.0]])
    res = nearest_np(Q, [(7, P)], 4, max_distance=1.0)
    assert res.count.tolist() == [2, 0, 0, 0, 0, 0, 2]
    assert res.pose[0].tolist() == [7, 7, -1, -1] and res.index[0].tolist() == [0, 1, -1, -1]
    assert res.distance2[0].tolist() == [0.0, 1.0, np.inf, np.inf]          # (d2 == r2: the radius is inclusive)
    assert res.index[6].tolist() == [0, 1, -1, -1] and res.distance2[6, :2].tolist() == [0.25, 0.25]
    assert np.all(res.pose[1:6] == -1) and np.all(res.index[1:6] == -1) and np.all(np.isposinf(res.distance2[1:6]))
    # float32 queries are widened exactly; lists work
    q32 = np.array([[0.1, 0.2, 0.3]], dtype=np.float32)
    a, b = nearest_np(q32, [(0, P)], 2, max_distance=3.0), nearest_np(q32.astype(np.float64), [(0, P)], 2, max_distance=3.0)
    assert np.array_equal(a.distance2, b.distance2) and np.array_equal(a.index, b.index)
    assert nearest_np([[0.0, 0.0, 0.0]], [(0, P.tolist())], 1, max_distance=0.5).index.tolist() == [[0]]
    # n = 0, no clouds, empty clouds
    e = nearest_np(np.empty((0, 3)), [(0, P)], 3, max_distance=1.0)
    assert e.pose.shape == e.index.shape == e.distance2.shape == (0, 3) and e.count.shape == (0,)
    for clouds in ([], [(0, np.empty((0, 3)))]):
        z = nearest_np(Q, clouds, 2, max_distance=1.0)
        assert z.count.tolist() == [0] * len(Q) and np.all(z.pose == -1) and np.all(np.isposinf(z.distance2))
    # argument errors
    for k in (0, -1, NN_MAX_K + 1, 1.5, True):
        with pytest.raises(ValueError):
            nearest_np(Q, [(0, P)], k, max_distance=1.0)
    for r in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            nearest_np(Q, [(0, P)], 1, max_distance=r)
    with pytest.raises(TypeError):
        nearest_np(Q, [(0, P)], 1)
    with pytest.raises(ValueError):
        nearest_np(np.zeros((3, 2)), [(0, P)], 1, max_distance=1.0)
    assert NN_MAX_K == 8
    for name in ("Neighbours", "nearest_np"):
        assert name in octreelib_amd.__all__ and hasattr(octreelib_amd, name)


def test_declared_and_in_the_signature_table():
    import ctypes as C
    import os
    import re

    from octreelib_amd import _native as nat

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "octreelib_hip.h")).read()
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "#define OCTL_NN_MAX_K 8" in header
    p, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    for name in ("octl_forest_nearest", "octl_forest_nearest_device"):
        assert f"int {name}(octl_forest* f, const double* xyz" in header
        assert nat.SIGNATURES[name] == (C.c_int, [p, p, i64, i32, f64, p, i32, p, p, p, p])
