"""neighbourhood_statistics_np and point_statistics_np, the definitions of the neighbourhood statistics
(octreelib_amd/neighbourhood.py), HostMap.neighbourhood_statistics / point_statistics - what the classes on the
caller's own plug types answer with - and orient_towards.  No GPU: the device kernels are compared with these
definitions in tests/test_gpu_neighbourhood.py, the kernels' code on the host in
tests/test_cpu_neighbourhood_host.py."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import octreelib_amd
from octreelib_amd import (PointStatistics, neighbourhood_statistics, neighbourhood_statistics_np, orient_towards,
                           point_statistics, point_statistics_np, radius_count_np)
from octreelib_amd.leaf_stats import LeafStatistics
from oracle.octree_np import OGrid
from tests._neighbourhood import assert_exact_bound, neighbours_of, pick_rows
from tests.test_cpu_map_operations import UNKNOWN, _on_plug_types
from tests.test_cpu_query import _depths, _grid_map
from tests.test_cpu_radius import _two_clouds
from tests.test_cpu_raycast_host import _cube_map


def test_the_definition_equals_a_plain_loop_and_counts_as_radius_count_np():
    clouds, Q = _two_clouds()
    r = 0.1
    r2 = r * r
    st = neighbourhood_statistics_np(Q, clouds, r)
    assert isinstance(st, LeafStatistics) and st.count.dtype == np.int64
    assert st.mean.shape == (len(Q), 3) and st.covariance.shape == (len(Q), 3, 3)
    assert st.eigenvalues.shape == (len(Q), 3) and st.eigenvectors.shape == (len(Q), 3, 3)
    for radius in (0.04, r, 0.2):
        for sub in (clouds, clouds[1:]):
            assert np.array_equal(neighbourhood_statistics_np(Q, sub, radius, eigen=False).count,
                                  radius_count_np(Q, sub, radius))
    assert st.count.max() > 8 and np.all(st.count[-4:] == 0)
    small = neighbourhood_statistics_np(Q, clouds, 0.05)
    assert (small.count[:250] == 0).any() and (small.count == 1).any()
    for st, r2, i, q in [(s, rr * rr, i, q) for s, rr in ((st, r), (small, 0.05)) for i, q in enumerate(Q[:40].tolist())]:
        near = []
        for _, P in clouds:
            for p in P.tolist():
                dx, dy, dz = q[0] - p[0], q[1] - p[1], q[2] - p[2]
                if (dx * dx + dy * dy) + dz * dz <= r2:
                    near.append(p)
        assert st.count[i] == len(near)
        if not near:
            assert np.isnan(st.mean[i]).all() and np.isnan(st.covariance[i]).all()
            assert np.isnan(st.eigenvalues[i]).all() and np.isnan(st.eigenvectors[i]).all()
            continue
        N = np.array(near)
        assert np.allclose(st.mean[i], N.mean(axis=0), rtol=0, atol=1e-14)
        cov = np.cov(N.T, bias=True) if len(N) > 1 else np.zeros((3, 3))
        assert np.allclose(st.covariance[i], cov, rtol=0, atol=1e-15)
        w = np.linalg.eigvalsh(st.covariance[i])
        assert np.allclose(st.eigenvalues[i], w, rtol=0, atol=1e-15)
        v = st.eigenvectors[i]
        assert np.allclose(st.covariance[i] @ v, v * st.eigenvalues[i], rtol=0, atol=1e-15)
        assert all(v[np.argmax(np.abs(v[:, c])), c] > 0 for c in range(3))          # the library's sign rule
    # rows without a neighbour are NaN, single neighbours have no spread
    st = small
    none, one = st.count == 0, st.count == 1
    assert none.any() and one.any()
    assert np.isnan(st.mean[none]).all() and np.isnan(st.covariance[none]).all() and np.isnan(st.eigenvalues[none]).all()
    assert np.all(st.covariance[one] == 0.0) and np.all(st.surface_variation[one] == 0.0)
    # the two-pass moments in longdouble agree with exact rationals far below the bound of the device
    st = neighbourhood_statistics_np(Q, clouds, r)
    lists = neighbours_of(Q, clouds, r)
    hi = neighbourhood_statistics_np(Q, clouds, r, dtype=np.longdouble, eigen=False)
    assert hi.mean.dtype == np.longdouble and hi.eigenvalues is None and hi.eigenvectors is None
    rows = pick_rows(st.count, limit=24, max_n=40)
    assert len(rows) >= 12
    for ref in (st, LeafStatistics(hi.count, hi.mean.astype(np.float64), hi.covariance.astype(np.float64))):
        assert_exact_bound(ref, Q, lists, rows, "definition")
    # chunking does not show; empty inputs
    assert neighbourhood_statistics_np(np.empty((0, 3)), clouds, r).count.shape == (0,)
    empty = neighbourhood_statistics_np(Q[:5], [], r)
    assert empty.count.tolist() == [0] * 5 and np.isnan(empty.mean).all() and np.isnan(empty.eigenvectors).all()


def test_point_statistics_np_rows_poses_and_indices():
    rng = np.random.default_rng(7)
    A, B, Cc = rng.random((120, 3)), rng.random((80, 3)), rng.random((30, 3))
    clouds = [(4, A), (9, B)]
    r = 0.2
    st = point_statistics_np(clouds, None, r)
    assert isinstance(st, PointStatistics) and st.pose.dtype == np.int32 and st.index.dtype == np.int32
    assert st.pose.tolist() == [4] * 120 + [9] * 80 and st.index.tolist() == list(range(120)) + list(range(80))
    whole = neighbourhood_statistics_np(np.concatenate([A, B]), clouds, r)
    assert np.array_equal(st.count, whole.count) and np.array_equal(st.mean, whole.mean)
    assert np.array_equal(st.covariance, whole.covariance) and np.array_equal(st.eigenvectors, whole.eigenvectors)
    assert st.count.min() >= 1                                          # a point counts itself (PCL's convention)
    assert np.array_equal(st.count, radius_count_np(np.concatenate([A, B]), clouds, r))
    # one tested pose of the two; a tested pose that is not counted has no point of its own among its neighbours
    one = point_statistics_np(clouds, [9], r)
    assert one.pose.tolist() == [9] * 80 and np.array_equal(one.count, st.count[120:])
    mixed = point_statistics_np(clouds, [4, (5, Cc)], r, eigen=False)
    assert mixed.pose.tolist() == [4] * 120 + [5] * 30 and mixed.index.tolist() == list(range(120)) + list(range(30))
    assert mixed.eigenvalues is None and np.array_equal(mixed.count[120:], radius_count_np(Cc, clouds, r))
    alone = point_statistics_np([(4, A)], [(9, B)], 0.05)
    assert alone.pose.tolist() == [9] * 80 and (alone.count == 0).any() and np.isnan(alone.mean[alone.count == 0]).all()
    with pytest.raises(ValueError):
        point_statistics_np(clouds, [5], r)                             # brings no points
    with pytest.raises(ValueError):
        point_statistics_np(clouds, [(4, A)], r)
    assert len(point_statistics_np([], None, r)) == 0 and len(point_statistics_np(clouds, [], r)) == 0


def test_host_map_on_a_grid_and_on_one_cube():
    rng = np.random.default_rng(3)
    clouds = {0: rng.uniform(-1.0, 2.0, (900, 3)) * [1.0, 1.0, 0.4], 3: rng.uniform(-1.0, 2.0, (600, 3)) * [1.0, 1.0, 0.4],
              7: rng.uniform(0.0, 1.0, (60, 3)) * [1.0, 1.0, 0.4]}
    og = OGrid(1)
    for p, P in clouds.items():
        og.insert_points(p, P)
    og.subdivide(12)
    hm = _grid_map(og, 1)
    assert _depths(hm.nodes).max() >= 2
    stored = hm.clouds()
    assert [p for p, _ in stored] == [0, 3, 7]
    Q = np.concatenate([rng.uniform(-1.2, 2.2, (200, 3)) * [1.0, 1.0, 0.4], stored[0][1][:40], [[np.nan, 0.0, 0.0]]])
    r = 0.25
    got = hm.neighbourhood_statistics(Q, r)
    ref = neighbourhood_statistics_np(Q, stored, r, dtype=np.longdouble)
    assert got.mean.dtype == np.float64 and np.array_equal(got.count, radius_count_np(Q, stored, r))
    assert np.array_equal(got.mean, ref.mean.astype(np.float64), equal_nan=True)
    assert np.array_equal(got.eigenvalues, ref.eigenvalues, equal_nan=True) and got.count.max() > 8
    sub = hm.neighbourhood_statistics(Q, r, pose_numbers=[3], eigen=False)
    assert np.array_equal(sub.count, radius_count_np(Q, stored[1:2], r)) and sub.eigenvectors is None
    lists = neighbours_of(Q, stored, r)
    assert_exact_bound(got, Q, lists, pick_rows(got.count, limit=16, max_n=60), "host map")
    # the self-query: every pose, the newest against the whole map, the newest against the older ones only
    ps = hm.point_statistics(r)
    assert ps.pose.tolist() == sum(([p] * len(P) for p, P in stored), [])
    assert ps.index.tolist() == sum((list(range(len(P))) for _, P in stored), [])
    assert np.array_equal(ps.count, radius_count_np(np.concatenate([P for _, P in stored]), stored, r))
    new = hm.point_statistics(r, pose_numbers=[7])
    assert new.pose.tolist() == [7] * 60 and np.array_equal(new.count, ps.count[-60:])
    assert np.array_equal(new.covariance, ps.covariance[-60:])
    old = hm.point_statistics(r, pose_numbers=[7, 0], among=[0, 3], eigen=False)
    assert old.pose.tolist() == [0] * 900 + [7] * 60 and old.eigenvalues is None      # insertion order, not the order given
    assert np.array_equal(old.count[900:], radius_count_np(stored[2][1], stored[:2], r))
    assert np.all(old.count[900:] == new.count - radius_count_np(stored[2][1], stored[2:], r))
    with pytest.raises(ValueError, match="voxel edge"):
        hm.neighbourhood_statistics(Q, 2.5)
    with pytest.raises(ValueError, match="voxel edge"):
        hm.point_statistics(2.5)
    # one cube whose corner is not dyadic: no cap on the radius
    c0, e0 = 0.1, 3.3
    P = c0 + rng.random((1500, 3)) * e0 * [1.0, 1.0, 0.3]
    cube = _cube_map(P, [c0, c0, c0], e0, 20)
    stored = cube.clouds()
    got = cube.neighbourhood_statistics(P[:100], 0.3)
    assert np.array_equal(got.count, radius_count_np(P[:100], stored, 0.3)) and got.count.min() >= 1
    assert cube.neighbourhood_statistics(P[:3], 50.0).count.tolist() == [len(P)] * 3
    assert len(cube.point_statistics(0.3)) == len(P)


@pytest.mark.parametrize("name", ["Grid", "OctreeManager"])
def test_plug_types_and_refusals(name):
    obj = _on_plug_types(name)
    pts = obj._host_map().clouds()[0][1]
    Q = np.concatenate([pts[:20], [[0.5, 0.5, 0.5], [np.nan, 0.0, 0.0], [9.0, 9.0, 9.0]]])
    got = neighbourhood_statistics(obj, Q, 0.25, pose_numbers=[0])
    ref = neighbourhood_statistics_np(Q, [(0, pts)], 0.25, dtype=np.longdouble)
    assert np.array_equal(got.count, radius_count_np(Q, [(0, pts)], 0.25)) and got.count[:20].min() >= 1
    assert np.array_equal(got.covariance, ref.covariance.astype(np.float64), equal_nan=True)
    assert neighbourhood_statistics(obj, Q, 0.25, eigen=False).eigenvalues is None
    ps = point_statistics(obj, 0.25)                                                 # (reads the map: no NotImplementedError)
    assert isinstance(ps, PointStatistics) and ps.pose.tolist() == [0] * 50 and ps.index.tolist() == list(range(50))
    assert np.array_equal(ps.count, radius_count_np(pts, [(0, pts)], 0.25))
    assert len(point_statistics(obj, 0.25, pose_numbers=[0], among=[0], eigen=False)) == 50
    for call in (lambda: neighbourhood_statistics(obj, Q, 0.25, pose_numbers=[UNKNOWN]),
                 lambda: point_statistics(obj, 0.25, pose_numbers=[UNKNOWN]),
                 lambda: point_statistics(obj, 0.25, among=[UNKNOWN])):
        with pytest.raises(KeyError):
            call()
    for bad in (0.0, -1.0, np.nan, np.inf, None, "x"):
        with pytest.raises(ValueError, match="neighbourhood_statistics"):
            neighbourhood_statistics(obj, Q, bad)
        with pytest.raises(ValueError, match="point_statistics"):
            point_statistics(obj, bad)
        with pytest.raises(ValueError):
            neighbourhood_statistics_np(Q, [(0, pts)], bad)
        with pytest.raises(ValueError):
            point_statistics_np([(0, pts)], None, bad)
    if name == "Grid":
        with pytest.raises(ValueError, match="voxel edge"):
            neighbourhood_statistics(obj, Q, 4.5)
        with pytest.raises(ValueError, match="voxel edge"):
            point_statistics(obj, 4.5)
    else:
        assert neighbourhood_statistics(obj, Q[:2], 100.0).count.tolist() == [50, 50]    # one cube has no cap
    for other in (None, 3, np.zeros((4, 3)), obj._host_map()):
        with pytest.raises(TypeError):
            neighbourhood_statistics(other, Q, 0.25)
        with pytest.raises(TypeError):
            point_statistics(other, 0.25)
    with pytest.raises(ValueError):
        neighbourhood_statistics(obj, np.zeros((3, 2)), 0.25)


def test_orient_towards():
    n = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    p = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 5.0], [2.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    out = orient_towards(n, p, [0.0, 0.0, 3.0])
    assert out.tolist() == [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]   # (a tie stays)
    assert n[1].tolist() == [0.0, 0.0, 1.0]                                                       # a new array
    per_point = np.array([[0.0, 0.0, -3.0], [0.0, 0.0, 9.0], [5.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    out = orient_towards(n, p, per_point)
    assert out.tolist() == [[0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]
    rng = np.random.default_rng(2)
    N, P = rng.normal(size=(200, 3)), rng.normal(size=(200, 3))
    out = orient_towards(N, P, [1.0, 2.0, 3.0])
    assert np.all(np.einsum("ij,ij->i", out, np.array([1.0, 2.0, 3.0]) - P) >= 0) and np.all(np.abs(out) == np.abs(N))
    assert orient_towards(np.empty((0, 3)), np.empty((0, 3)), [0.0, 0.0, 0.0]).shape == (0, 3)


def test_exported_declared_and_in_the_signature_table():
    from octreelib_amd import _native as nat

    for name in ("PointStatistics", "neighbourhood_statistics", "neighbourhood_statistics_np", "point_statistics",
                 "point_statistics_np", "orient_towards"):
        assert name in octreelib_amd.__all__ and hasattr(octreelib_amd, name)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "octreelib_hip.h")).read()
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    p, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    for name in ("octl_forest_neighbourhood_stats", "octl_forest_neighbourhood_stats_device"):
        assert f"int {name}(octl_forest* f, const double* xyz" in header
        assert nat.SIGNATURES[name] == (C.c_int, [p, p, i64, f64, p, i32, p, p, p, p, p])
    assert "int octl_forest_point_stats(octl_forest* f, double radius, const uint8_t* slot_sel," in header
    assert nat.SIGNATURES["octl_forest_point_stats"] == (C.c_int, [p, f64, p, i32, p, i32, i64, C.POINTER(C.c_int64),
                                                                   p, p, p, p, p, p, p])
    # each says that the reference has nothing like it
    for name in ("octl_forest_neighbourhood_stats", "octl_forest_neighbourhood_stats_device", "octl_forest_point_stats"):
        before = text[:text.index(f"int {name}(")]
        assert "No reference counterpart" in before[before.rindex("/*"):]
