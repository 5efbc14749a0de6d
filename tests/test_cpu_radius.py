"""radius_count_np and sparse_keep_np, the brute-force definitions of the radius count and of radius outlier removal
(octreelib_amd/query.py), and HostMap.radius_count / remove_sparse - what the classes on the caller's own plug types
answer with.  No GPU: the device kernels are compared with these definitions count for count in
tests/test_gpu_radius.py."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import octreelib_amd
from octreelib_amd import nearest_np, radius_count_np, sparse_keep_np
from octreelib_amd.query import COUNT_MAX, HostMap, check_radius_args, sparse_counts_np


def lattice():
    """{0, 1/8, .., 15/8}^3: every coordinate and every d2 is exact in f64, and d2 == r2 holds exactly between
    lattice neighbours at r = 1/8."""
    t = np.arange(16) / 8.0
    return np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(-1, 3)


def lattice_expected(P):
    """Points within 1/8 of a lattice point, itself included: 7 interior, 6 face, 5 edge, 4 corner."""
    on_wall = ((P == 0.0) | (P == 15 / 8.0)).sum(axis=1)
    return (7 - on_wall).astype(np.int32)


class _Leaf:
    def __init__(self, corner, edge, points):
        self.corner_min, self.edge_length, self._p = corner, edge, points

    def get_points(self):
        return self._p


def _two_clouds(seed=1):
    rng = np.random.default_rng(seed)
    clouds = [(4, rng.random((1200, 3))), (9, rng.random((800, 3)))]
    clouds[1][1][:50] = clouds[0][1][:50]             # duplicates across and inside the poses
    clouds[0][1][100:120] = clouds[0][1][200:220]
    Q = np.concatenate([rng.random((250, 3)), clouds[0][1][:30], clouds[0][1][200:220],
                        [[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [1e300, 0.0, 0.0]]])
    return clouds, Q


def test_counts_equal_the_candidates_of_nearest_np_and_caps_saturate():
    clouds, Q = _two_clouds()
    seen_small = seen_large = False
    for r in (0.04, 0.07, 0.2):
        full = radius_count_np(Q, clouds, r)
        assert full.dtype == np.int32 and full.shape == (len(Q),)
        nn = nearest_np(Q, clouds, 8, max_distance=r)
        small = full <= 8
        assert np.array_equal(full[small], nn.count[small])          # wherever the true count fits the list
        assert np.all(nn.count[~small] == 8)
        seen_small, seen_large = seen_small or small[:300].any(), seen_large or (~small).any()
        for cap in (1, 3, 7, 8, 1000, COUNT_MAX):
            assert np.array_equal(radius_count_np(Q, clouds, r, max_count=cap), np.minimum(full, cap))
        assert np.all(full[-4:] == 0)                               # queries that are not finite count 0
        # one cloud of the two; the chunking does not show
        one = radius_count_np(Q, clouds[1:], r)
        assert np.array_equal(np.minimum(one, 8), nearest_np(Q, clouds[1:], 8, max_distance=r).count)
        assert one.sum() < full.sum()
        assert np.array_equal(radius_count_np(Q, clouds, r, chunk=7), full)
    assert seen_small and seen_large
    # a python loop over one small case
    r = 0.1
    r2 = r * r
    got = radius_count_np(Q[:40], clouds, r)
    for i, q in enumerate(Q[:40].tolist()):
        c = 0
        for _, P in clouds:
            for p in P.tolist():
                dx, dy, dz = q[0] - p[0], q[1] - p[1], q[2] - p[2]
                c += (dx * dx + dy * dy) + dz * dz <= r2
        assert got[i] == c


def test_lattice_counts_are_exact_and_the_radius_is_inclusive():
    P = lattice()
    assert len(P) == 4096
    want = lattice_expected(P)
    assert sorted(np.unique(want).tolist()) == [4, 5, 6, 7]
    assert ((want == 7).sum(), (want == 6).sum(), (want == 5).sum(), (want == 4).sum()) == (14 ** 3, 6 * 14 * 14, 12 * 14, 8)
    got = radius_count_np(P, [(0, P)], 0.125)
    assert np.array_equal(got, want)
    # just below the radius only the point itself is left: the six neighbours were counted by d2 == r2
    assert np.all(radius_count_np(P, [(0, P)], np.nextafter(0.125, 0.0)) == 1)
    keep = sparse_keep_np([(0, P)], None, 0.125, 6)
    assert np.array_equal(keep[0], want - 1 >= 6) and keep[0].sum() == 14 ** 3
    # ... and through a HostMap whose leaves are the eight unit voxels
    roots, leaves = [], {0: []}
    for key in sorted({tuple(v) for v in np.floor(P).astype(int).tolist()}):
        c = np.array(key, dtype=np.float64)
        roots.append((c, 1.0))
        leaves[0].append(_Leaf(c, 1.0, P[np.all(np.floor(P).astype(int) == key, axis=1)]))
    hm = HostMap(0, 1.0, roots, leaves)
    assert np.array_equal(hm.radius_count(P, 0.125), want)
    assert np.array_equal(hm.radius_count(P, 0.125, max_count=5), np.minimum(want, 5))
    (pose, k), = hm.remove_sparse(0.125, 6)
    stored = hm.clouds()[0][1]
    assert pose == 0 and np.array_equal(k, lattice_expected(stored) - 1 >= 6)
    with pytest.raises(ValueError, match="voxel edge"):
        hm.radius_count(P, 2.5)
    with pytest.raises(ValueError, match="voxel edge"):
        hm.remove_sparse(2.5, 1)


def test_sparse_keep_np_on_hand_made_cases():
    far = np.array([[100.0, 0.0, 0.0]])
    pair = np.array([[50.0, 50.0, 50.0], [50.0, 50.0, 50.0]])           # two duplicates far from everything
    cluster = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.1, 0.0], [0.0, 0.0, 0.1]])
    A = np.concatenate([cluster, pair, far])
    keep, = sparse_keep_np([(0, A)], None, 0.5, 1)
    assert keep.tolist() == [True] * 4 + [True, True] + [False]         # the duplicates keep each other; the single point goes
    keep, = sparse_keep_np([(0, A)], None, 0.5, 2)
    assert keep.tolist() == [True] * 4 + [False, False, False]
    keep, = sparse_keep_np([(0, A)], None, 0.5, 4)
    assert not keep.any()                                               # three others each: the point itself never counts
    assert [c.tolist() for c in sparse_counts_np([(0, A)], None, 0.5)] == [[3, 3, 3, 3, 1, 1, 0]]
    # exactly on the radius counts; a point that is not finite has no neighbour and is none
    B = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]])
    assert sparse_keep_np([(3, B)], None, 0.5, 1)[0].tolist() == [True, True, False, False]
    assert sparse_keep_np([(3, B)], None, np.nextafter(0.5, 0.0), 1)[0].tolist() == [False] * 4
    # tested / among: identity is (pose, row) - the same coordinates in another pose are a neighbour
    X, Y = np.array([[0.0, 0.0, 0.0], [9.0, 9.0, 9.0]]), np.array([[0.0, 0.0, 0.0], [20.0, 0.0, 0.0]])
    both = [(1, X), (2, Y)]
    kx, ky = sparse_keep_np(both, None, 0.25, 1)
    assert kx.tolist() == [True, False] and ky.tolist() == [True, False]
    kx, ky = sparse_keep_np(both, [2], 0.25, 1)
    assert kx.tolist() == [True, True] and ky.tolist() == [True, False]                 # pose 1 is not judged
    kx, = sparse_keep_np([(1, X)], [1], 0.25, 1)
    assert kx.tolist() == [False, False]                                                # among pose 1 alone
    # a tested pose that is not counted: no point of its own to exclude
    k1, ky = sparse_keep_np([(1, X)], [(2, Y)], 0.25, 1)
    assert k1.tolist() == [True, True] and ky.tolist() == [True, False]
    k1, k2, ky = sparse_keep_np([(1, X), (2, Y)], [1, (5, Y)], 0.25, 2)
    assert k1.tolist() == [False, False] and k2.tolist() == [True, True] and ky.tolist() == [True, False]
    with pytest.raises(ValueError):
        sparse_keep_np([(1, X)], [2], 0.25, 1)                                          # brings no points
    with pytest.raises(ValueError):
        sparse_keep_np([(1, X)], [(1, X)], 0.25, 1)
    # empty inputs
    assert [k.tolist() for k in sparse_keep_np([(0, np.empty((0, 3)))], None, 1.0, 1)] == [[]]
    assert sparse_keep_np([], None, 1.0, 1) == []


def test_host_map_agrees_with_the_definitions():
    rng = np.random.default_rng(5)
    roots = [(np.array([0.0, 0.0, 0.0]), 2.0), (np.array([2.0, 0.0, 0.0]), 2.0)]
    pts = {p: rng.uniform(0.0, 4.0, (n, 3)) * [1.0, 0.5, 0.5] for p, n in ((3, 700), (8, 500), (11, 40))}
    leaves = {p: [_Leaf(c, e, P[(P[:, 0] >= c[0]) & (P[:, 0] < c[0] + e)]) for c, e in roots] for p, P in pts.items()}
    hm = HostMap(0, 2.0, roots, leaves)
    clouds = hm.clouds()
    assert [p for p, _ in clouds] == [3, 8, 11]
    Q = np.concatenate([rng.uniform(-0.5, 4.5, (300, 3)) * [1.0, 0.5, 0.5], [[np.nan, 0.0, 0.0]]])
    for cap in (None, 1, 3, 7):
        assert np.array_equal(hm.radius_count(Q, 0.3, max_count=cap), radius_count_np(Q, clouds, 0.3, max_count=cap))
    assert np.array_equal(hm.radius_count(Q, 0.3, pose_numbers=[8]), radius_count_np(Q, clouds[1:2], 0.3))
    assert (hm.radius_count(Q, 0.3) > 8).any()
    got = hm.remove_sparse(0.2, 3)
    ref = sparse_keep_np(clouds, None, 0.2, 3)
    assert [p for p, _ in got] == [3, 8, 11] and all(np.array_equal(k, r) for (_, k), r in zip(got, ref))
    assert 0 < sum(int(k.sum()) for _, k in got) < sum(len(k) for _, k in got)
    # the newest pose against the whole map; against the older poses only (it is not counted itself)
    (p, k), = hm.remove_sparse(0.2, 3, pose_numbers=[11])
    assert p == 11 and np.array_equal(k, sparse_keep_np(clouds, [11], 0.2, 3)[2])
    (p, k), = hm.remove_sparse(0.2, 3, pose_numbers=[11], among=[3, 8])
    assert p == 11 and np.array_equal(k, sparse_keep_np(clouds[:2], [clouds[2]], 0.2, 3)[2])
    assert np.array_equal(k, radius_count_np(clouds[2][1], clouds[:2], 0.2) >= 3)


def test_argument_refusals():
    P = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    for r in (0.0, -1.0, np.nan, np.inf, -np.inf, None, "x"):
        with pytest.raises(ValueError):
            check_radius_args(r)
        with pytest.raises(ValueError):
            radius_count_np(P, [(0, P)], r)
        with pytest.raises(ValueError):
            sparse_keep_np([(0, P)], None, r, 1)
    for bad in (0, -1, 2 ** 31, 1.5, 2.0, True, "3"):
        with pytest.raises(ValueError):
            check_radius_args(1.0, max_count=bad)
        with pytest.raises(ValueError):
            check_radius_args(1.0, min_neighbours=bad)
        with pytest.raises(ValueError):
            radius_count_np(P, [(0, P)], 1.0, max_count=bad)
        with pytest.raises(ValueError):
            sparse_keep_np([(0, P)], None, 1.0, bad)
    with pytest.raises(ValueError):
        sparse_keep_np([(0, P)], None, 1.0, None)                    # min_neighbours is required
    assert check_radius_args(np.float32(0.5), np.int64(3), 2 ** 31 - 1) == (0.5, 3, COUNT_MAX)
    assert check_radius_args(2, None, None) == (2.0, None, None)
    with pytest.raises(ValueError):
        radius_count_np(np.zeros((3, 2)), [(0, P)], 1.0)
    assert radius_count_np(np.empty((0, 3)), [(0, P)], 1.0).shape == (0,)
    assert radius_count_np(P, [], 1.0).tolist() == [0, 0] and radius_count_np(P, [(0, np.empty((0, 3)))], 1.0).tolist() == [0, 0]
    assert radius_count_np(P.astype(np.float32), [(0, P)], 1.0).tolist() == [2, 2]
    for name in ("radius_count_np", "sparse_keep_np"):
        assert name in octreelib_amd.__all__ and hasattr(octreelib_amd, name)


def test_declared_and_in_the_signature_table():
    from octreelib_amd import _native as nat

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "octreelib_hip.h")).read()
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    p, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    for name in ("octl_forest_radius_count", "octl_forest_radius_count_device"):
        assert f"int {name}(octl_forest* f, const double* xyz" in header
        assert nat.SIGNATURES[name] == (C.c_int, [p, p, i64, f64, i32, p, i32, p])
    assert "int octl_forest_remove_sparse(octl_forest* f, double radius, int32_t min_neighbours," in header
    assert nat.SIGNATURES["octl_forest_remove_sparse"] == (C.c_int, [p, f64, i32, p, i32, p, i32, C.POINTER(C.c_int64)])
