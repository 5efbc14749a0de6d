"""cluster_labels_np and small_cluster_keep_np, the definitions of the Euclidean clusters (octreelib_amd/clustering.py),
and HostMap.cluster / remove_small_clusters - what the classes on the caller's own plug types answer with.  The
definitions hash the points into cells; here they are held to a plain adjacency matrix plus breadth-first search
(tests/_cluster.py) on at most 300 points.  No GPU: the device kernels are compared with these definitions in
tests/test_gpu_cluster.py, the kernels' code on the host in tests/test_cpu_cluster_host.py."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import octreelib_amd
from octreelib_amd import clustering
from octreelib_amd.clustering import (Clusters, check_cluster_args, cluster, cluster_labels_np, remove_small_clusters,
                                      small_cluster_keep_np)
from oracle.octree_np import OGrid
from tests._cell import lattice01, ulp_neighbours
from tests._cluster import CHAIN_RADIUS, adjacency, brute_labels, diagonal_chain
from tests.test_cpu_map_operations import UNKNOWN, _on_plug_types
from tests.test_cpu_query import _depths, _grid_map
from tests.test_cpu_raycast_host import _cube_map


def _same(got, want):
    assert len(got[0]) == len(want[0])
    for a, b in zip(got[0], want[0]):
        assert a.dtype == np.int32 and np.array_equal(a, b)
    assert got[1].dtype == np.int64 and np.array_equal(got[1], want[1])
    assert got[2].shape == (len(want[1]), 2) and np.array_equal(got[2], want[2])


def _blobs(rng, n_blobs, spread, lo=1, hi=30):
    return np.concatenate([rng.uniform(-1.0, 2.0, 3) + rng.normal(0.0, spread, (int(m), 3))
                           for m in rng.integers(lo, hi, n_blobs)])


def test_the_definition_equals_adjacency_and_breadth_first_search():
    rng = np.random.default_rng(0)
    P = _blobs(rng, 20, 0.05)[:300]
    for split in ([len(P)], [100, 37, len(P) - 137], [0, len(P), 0]):
        cuts = np.cumsum(split)[:-1]
        clouds = [(7 * i + 3, part) for i, part in enumerate(np.split(P, cuts))]
        for r in (0.02, 0.06, 0.15, 0.5, 10.0):
            _same(cluster_labels_np(clouds, r), brute_labels(clouds, r))
    labels, sizes, first = cluster_labels_np([(0, P)], 0.06)
    assert 1 < len(sizes) < len(P) and sizes.sum() == len(P) and sizes.max() > 5
    assert np.all(np.diff(first[:, 1]) > 0) and first[0].tolist() == [0, 0]          # numbered by smallest id
    # duplicates are neighbours; a point alone is a cluster of one; a row that is not finite joins nothing
    D = np.concatenate([P[:40], P[:40], P[:5], [[50.0, 50.0, 50.0]], [[np.nan, 0.0, 0.0]], [[np.inf, 0.0, 0.0]]])
    got = cluster_labels_np([(0, D[:60]), (1, D[60:])], 1e-9)
    _same(got, brute_labels([(0, D[:60]), (1, D[60:])], 1e-9))
    assert sorted(got[1].tolist()) == [1] * 3 + [2] * 35 + [3] * 5
    # nothing stored
    for clouds in ([], [(0, np.empty((0, 3)))]):
        labels, sizes, first = cluster_labels_np(clouds, 0.1)
        assert len(sizes) == 0 and first.shape == (0, 2) and all(len(a) == 0 for a in labels)
    assert small_cluster_keep_np([], 0.1, 3) == []


def test_the_lattice_and_an_ulp_either_side():
    P, _ = lattice01(-3, 3)
    up, down = ulp_neighbours(P)
    X = np.concatenate([P, up[::5], down[::7]])
    assert len(X) <= 300
    # fl(k 0.1) steps either side of 0.1: pairs of lattice neighbours straddle d2 == r2
    adj = adjacency(P, 0.1)
    axis_neighbours = np.isclose(np.abs(P[:, None, :] - P[None, :, :]).sum(axis=2), 0.1)
    assert (adj & axis_neighbours).any() and (~adj & axis_neighbours).any()
    rng = np.random.default_rng(4)
    for pts in (P, X, X[rng.permutation(len(X))]):
        clouds = [(0, pts[::2]), (1, pts[1::2])]
        for r in (0.1, np.nextafter(0.1, 1.0), np.nextafter(0.1, 0.0), 0.15):
            _same(cluster_labels_np(clouds, r), brute_labels(clouds, r))
    assert len(cluster_labels_np([(0, P)], 0.1)[1]) > 1 and len(cluster_labels_np([(0, P)], 0.15)[1]) == 1
    # the chain: d2 == r2 joins, one ulp more does not
    chain = diagonal_chain()
    labels, sizes, first = cluster_labels_np([(0, chain)], CHAIN_RADIUS)
    assert sizes.tolist() == [41, 19] and first.tolist() == [[0, 0], [0, 41]]
    assert cluster_labels_np([(0, chain)], np.nextafter(CHAIN_RADIUS, 0.0))[1].tolist() == [1] * 60
    _same(cluster_labels_np([(0, chain)], CHAIN_RADIUS), brute_labels([(0, chain)], CHAIN_RADIUS))
    # far from the origin and with huge gaps: the cells are hashed, never laid out
    far = np.concatenate([chain + 3.0e9, chain - 7.0e12, chain])
    _same(cluster_labels_np([(0, far)], 0.25), brute_labels([(0, far)], 0.25))


def test_gating_numbering_and_the_keep_rule():
    rng = np.random.default_rng(2)
    P = _blobs(rng, 25, 0.03)[:300]
    P = P[rng.permutation(len(P))]
    clouds = [(4, P[:120]), (2, P[120:])]
    r = 0.08
    every = cluster_labels_np(clouds, r)
    sizes = every[1]
    assert len(set(sizes.tolist())) > 4
    for lo, hi in ((1, None), (3, None), (1, 4), (3, 9), (5, 5), (2 ** 31 - 1, None), (1, 2 ** 31 - 1)):
        got = cluster_labels_np(clouds, r, lo, hi)
        _same(got, brute_labels(clouds, r, lo, hi))
        inside = (sizes >= lo) & (sizes <= (hi if hi is not None else sizes.max()))
        assert np.array_equal(got[1], sizes[inside]) and np.array_equal(got[2], every[2][inside])
        # the same components, renumbered in the same order; the others -1
        renumber = np.where(inside, np.cumsum(inside) - 1, -1)
        for a, b in zip(got[0], every[0]):
            assert np.array_equal(a, renumber[b])
        # ascending in (position of the pose, row): the smallest id
        key = got[2][:, 0] * 10 ** 6 + got[2][:, 1]
        assert np.all(np.diff(key) > 0)
        for c, (where, row) in enumerate(got[2].tolist()):
            assert got[0][where][row] == c
            assert not (got[0][where][:row] == c).any() and all((got[0][w] != c).all() for w in range(where))
    for m in (1, 2, 3, 7, 50):
        keep = small_cluster_keep_np(clouds, r, m)
        assert [k.dtype for k in keep] == [bool, bool]
        for k, lab in zip(keep, every[0]):
            assert np.array_equal(k, sizes[lab] >= m)
        # one round is enough: what stays keeps its whole component
        left = [(p, c[k]) for (p, c), k in zip(clouds, keep)]
        assert all(k.all() for k in small_cluster_keep_np(left, r, m))
    assert all(k.all() for k in small_cluster_keep_np(clouds, r, 1))


def test_a_large_map_in_seconds():
    rng = np.random.default_rng(6)
    P = rng.random((100000, 3)) * [20.0, 20.0, 2.0]
    labels, sizes, first = cluster_labels_np([(0, P[:60000]), (1, P[60000:])], 0.12)
    assert sizes.sum() == len(P) and 100 < len(sizes) < len(P) and sizes.max() > 10
    # spot check: every point of a few clusters has all its neighbours inside the cluster
    label = np.concatenate(labels)
    for c in rng.integers(0, len(sizes), 20):
        members = np.nonzero(label == c)[0]
        assert len(members) == sizes[c]
        for i in members[:5]:
            d = P - P[i]
            near = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= np.float64(0.12) * np.float64(0.12)
            assert (label[near] == c).all()


def test_host_map_on_a_grid_and_on_one_cube():
    rng = np.random.default_rng(3)
    flat = [1.0, 1.0, 0.4]
    clouds = {0: _blobs(rng, 30, 0.04) * flat, 3: _blobs(rng, 20, 0.04) * flat, 7: _blobs(rng, 5, 0.04) * flat}
    og = OGrid(1)
    for p, P in clouds.items():
        og.insert_points(p, P)
    og.subdivide(12)
    hm = _grid_map(og, 1)
    assert _depths(hm.nodes).max() >= 2
    stored = hm.clouds()
    assert [p for p, _ in stored] == [0, 3, 7]
    r = 0.1
    cl = hm.cluster(r)
    assert isinstance(cl, Clusters)
    labels, sizes, first = cluster_labels_np(stored, r)
    assert cl.pose.tolist() == sum(([p] * len(P) for p, P in stored), [])
    assert cl.index.tolist() == sum((list(range(len(P))) for _, P in stored), [])
    assert cl.label.dtype == np.int32 and np.array_equal(cl.label, np.concatenate(labels))
    assert np.array_equal(cl.sizes, sizes) and len(cl) == len(sizes)
    assert np.array_equal(cl.first_pose, np.array([0, 3, 7])[first[:, 0]]) and np.array_equal(cl.first_index, first[:, 1])
    for c in (0, len(cl) - 1):
        m = cl.members(c)
        assert len(m) == cl.sizes[c] and (cl.pose[m[0]], cl.index[m[0]]) == (cl.first_pose[c], cl.first_index[c])
    with pytest.raises(IndexError):
        cl.members(len(cl))
    # the selected poses are the whole graph, in insertion order whatever the order given
    sub = hm.cluster(r, pose_numbers=[7, 0], min_points=3, max_points=40)
    want = cluster_labels_np([stored[0], stored[2]], r, 3, 40)
    assert sub.pose.tolist() == [0] * len(stored[0][1]) + [7] * len(stored[2][1])
    assert np.array_equal(sub.label, np.concatenate(want[0])) and np.array_equal(sub.sizes, want[1])
    assert (sub.label == -1).any() and set(sub.first_pose.tolist()) <= {0, 7}
    keep = hm.remove_small_clusters(r, 4, pose_numbers=[3, 0])
    assert [p for p, _ in keep] == [0, 3]
    for (_, k), w in zip(keep, small_cluster_keep_np(stored[:2], r, 4)):
        assert np.array_equal(k, w)
    assert not all(k.all() for _, k in keep)
    for call in (lambda: hm.cluster(2.5), lambda: hm.remove_small_clusters(2.5, 2)):
        with pytest.raises(ValueError, match="voxel edge"):
            call()
    # one cube whose corner is not dyadic: no cap on the radius
    c0, e0 = 0.1, 3.3
    P = c0 + rng.random((1500, 3)) * e0 * [1.0, 1.0, 0.3]
    cube = _cube_map(P, [c0, c0, c0], e0, 20)
    stored = cube.clouds()
    got = cube.cluster(0.1, min_points=2)
    want = cluster_labels_np(stored, 0.1, 2)
    assert np.array_equal(got.label, want[0][0]) and np.array_equal(got.sizes, want[1]) and len(got) > 3
    assert cube.cluster(50.0).sizes.tolist() == [len(P)]


@pytest.mark.parametrize("name", ["Grid", "OctreeManager"])
def test_plug_types_and_refusals(name):
    obj = _on_plug_types(name)
    pts = obj._host_map().clouds()[0][1]
    cl = cluster(obj, 0.25, pose_numbers=[0])                                       # (reads the map: no NotImplementedError)
    want = cluster_labels_np([(0, pts)], 0.25)
    assert isinstance(cl, Clusters) and cl.pose.tolist() == [0] * 50 and cl.index.tolist() == list(range(50))
    assert np.array_equal(cl.label, want[0][0]) and np.array_equal(cl.sizes, want[1])
    assert np.array_equal(cl.first_index, want[2][:, 1]) and (cl.first_pose == 0).all()
    gated = cluster(obj, 0.25, min_points=2, max_points=10)
    assert np.array_equal(gated.label, cluster_labels_np([(0, pts)], 0.25, 2, 10)[0][0])
    with pytest.raises(NotImplementedError, match="HostMap.remove_small_clusters gives the decision"):
        remove_small_clusters(obj, 0.25, 3)
    with pytest.raises(NotImplementedError, match="on the caller's own plug types"):
        remove_small_clusters(obj, 0.25, 3, pose_numbers=[UNKNOWN])                  # by name, before the pose lookup
    keep = obj._host_map().remove_small_clusters(0.25, 3)
    assert keep[0][0] == 0 and np.array_equal(keep[0][1], small_cluster_keep_np([(0, pts)], 0.25, 3)[0])
    with pytest.raises(KeyError):
        cluster(obj, 0.25, pose_numbers=[UNKNOWN])
    for bad in (0.0, -1.0, np.nan, np.inf, None, "x"):
        with pytest.raises(ValueError, match="cluster: radius"):
            cluster(obj, bad)
        with pytest.raises(ValueError, match="radius"):
            cluster_labels_np([(0, pts)], bad)
        with pytest.raises(ValueError, match="remove_small_clusters: radius"):
            small_cluster_keep_np([(0, pts)], bad, 2)
    for bad in (0, -3, 2 ** 31, 1.5, True, None, "2"):
        with pytest.raises(ValueError, match="cluster: min_points"):
            cluster(obj, 0.25, min_points=bad)
        with pytest.raises(ValueError, match="remove_small_clusters: min_points"):
            small_cluster_keep_np([(0, pts)], 0.25, bad)
        with pytest.raises(ValueError, match="remove_small_clusters: min_points"):
            obj._host_map().remove_small_clusters(0.25, bad)
        if bad is not None:
            with pytest.raises(ValueError, match="cluster: max_points"):
                cluster(obj, 0.25, max_points=bad)
    with pytest.raises(ValueError, match="max_points = 2 is below min_points = 3"):
        cluster(obj, 0.25, min_points=3, max_points=2)
    assert check_cluster_args("0.5", np.int64(3), 3) == (0.5, 3, 3) and check_cluster_args(1) == (1.0, 1, None)
    if name == "Grid":
        with pytest.raises(ValueError, match="voxel edge"):
            cluster(obj, 4.5)
    else:
        assert cluster(obj, 100.0).sizes.tolist() == [50]                           # one cube has no cap
    for other in (None, 3, np.zeros((4, 3)), obj._host_map()):
        with pytest.raises(TypeError, match="cluster"):
            cluster(other, 0.25)
        with pytest.raises(TypeError, match="remove_small_clusters"):
            remove_small_clusters(other, 0.25, 2)


def test_exported_declared_and_in_the_signature_table():
    from octreelib_amd import _native as nat

    names = ["Clusters", "cluster_labels_np", "small_cluster_keep_np", "check_cluster_args", "cluster",
             "remove_small_clusters"]
    for name in names:
        assert name in octreelib_amd.__all__ and getattr(octreelib_amd, name) is getattr(clustering, name)
    assert sorted(clustering.__all__) == sorted(names)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "octreelib_hip.h")).read()
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    p, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    assert ("int octl_forest_cluster_points(octl_forest* f, double radius, const uint8_t* slot_sel, int32_t n_sel, "
            "int64_t cap, int64_t* n_rows, int32_t* slot, int32_t* index, int64_t* first, int32_t* size);") in header
    assert nat.SIGNATURES["octl_forest_cluster_points"] == (C.c_int, [p, f64, p, i32, i64, C.POINTER(C.c_int64),
                                                                      p, p, p, p])
    assert ("int octl_forest_remove_small_clusters(octl_forest* f, double radius, int32_t min_points, const uint8_t* "
            "slot_sel, int32_t n_sel, int64_t* n_alive);") in header
    assert nat.SIGNATURES["octl_forest_remove_small_clusters"] == (C.c_int, [p, f64, i32, p, i32, C.POINTER(C.c_int64)])
    # each says that the reference has nothing like it
    for name in ("octl_forest_cluster_points", "octl_forest_remove_small_clusters"):
        before = text[:text.index(f"int {name}(")]
        assert "No reference counterpart" in before[before.rindex("/*"):]
