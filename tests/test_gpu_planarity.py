"""Planarity-driven subdivision on the device (octl_forest_build_planar, octl_forest_get_split_stats; NotPlanar
through Grid / OctreeManager / Octree.subdivide).

Two arithmetics decide the same predicate: the device's one-pass shifted f64 reduction and NumPy's two-pass form in
NotPlanar.__call__ (the definition, which the oracle and the library's host path evaluate).  They may disagree only
on a node whose statistic is within the device's error bound of the threshold, so every scene here is CHOSEN so
that no node the oracle evaluates has |lambda - max_variance| <= 1e-9 e^2 (e = node edge); _oracle_nodes asserts
that on the oracle's own values before anything is compared, and then the trees must be identical, no node excused.

The arithmetic itself is checked through octl_forest_get_split_stats against a longdouble two-pass value:
|lambda_dev - lambda| <= (4 gamma + 64 eps) * 3 (e/2)^2 * n / (n - ddof), gamma = (ceil(c/64) + ceil(c/4096) + 16) eps
with c = the node's points over ALL poses (c = n when every pose drives the scheme): DESIGN 4.7."""

import ctypes as C
import math

import numpy as np
import pytest

from octreelib_amd import MaxPoints, NotPlanar, synthetic
from octreelib_amd import _native as nat
from octreelib_amd._engine import Forest
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree_manager import OctreeManager
from oracle import octree_np as onp
from tests._util import (_longdouble_lambda, _oracle_nodes, _scheme_nodes, assert_same_leaves,
                         canon_from_list)

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
MV = 2.5e-4


# ---- helpers ---------------------------------------------------------------------------------------------------
def _wrapped(crit):
    """The same criteria as lambdas: not recognised, so the library evaluates them on the host."""
    return [(lambda points, c=c: c(points)) for c in crit]


def _views_table(leaves, pts):
    index = {pts[i].tobytes(): i for i in range(len(pts))}
    assert len(index) == len(pts)
    return canon_from_list([(v.corner_min, v.edge_length, [index[r.tobytes()] for r in v.get_points()])
                            for v in leaves])


def _device_nodes(forest):
    nd = forest.nodes
    cnt, lam = forest.split_stats()
    keys = [((nd["corner"][i] + 0.0).tobytes(), float(nd["edge"][i])) for i in range(len(cnt))]
    assert len(set(keys)) == len(keys)
    return keys, cnt, lam, nd["first_child"] >= 0


def _check_arithmetic(forest, oracle_nodes, crit, K, all_counts=None):
    keys, cnt, lam, internal = _device_nodes(forest)
    assert set(keys) == set(oracle_nodes)
    checked = 0
    for i, k in enumerate(keys):
        e, n, _, o_internal, rows = oracle_nodes[k]
        assert int(cnt[i]) == n
        if n < crit.min_points:
            assert math.isnan(lam[i])
        else:
            c = n if all_counts is None else all_counts[k]
            assert c >= n
            gamma = (math.ceil(c / 64) + math.ceil(c / 4096) + 16) * EPS
            ref, _ = _longdouble_lambda(rows, crit.ddof)
            bound = (4 * gamma + 64 * EPS) * 3 * (e / 2) ** 2 * n / (n - crit.ddof)
            assert abs(lam[i] - ref) <= bound, (i, n, e, lam[i], ref, bound)
            checked += 1
        # the decision is the stored value's, exactly
        want = (K >= 0 and n > K) or (n >= crit.min_points and lam[i] > crit.max_variance)
        assert bool(internal[i]) == want == o_internal
    return checked


def _syncs():
    c = C.c_uint64(0)
    nat.load().octl_debug_host_syncs(C.byref(c))
    return c.value


def _grid(clouds, crit, pose_numbers=None):
    g = Grid(GridConfig(voxel_edge_length=1))
    for p, pts in clouds.items():
        g.insert_points(p, pts)
    g.subdivide(crit, pose_numbers)
    return g


def _ogrid(clouds, crit, pose_numbers=None):
    og = onp.OGrid(1)
    for p, pts in clouds.items():
        og.insert_points(p, np.asarray(pts, dtype=np.float64))
    og.subdivide(crit, pose_numbers)
    return og


def _assert_grid_equal(g, other, clouds, ordered=True):
    """Grid `g` against an OGrid or another Grid: leaf tables, listing order, counters of every pose."""
    for p, pts in clouds.items():
        got = _views_table(g.get_leaf_points(p), np.asarray(pts, dtype=np.float64))
        if isinstance(other, onp.OGrid):
            want = canon_from_list(other.leaf_table(p))
        else:
            want = _views_table(other.get_leaf_points(p), np.asarray(pts, dtype=np.float64))
        assert_same_leaves(got, want, ordered=ordered)
        assert g.n_nodes(p) == other.n_nodes(p) and g.n_leaves(p) == other.n_leaves(p)
        assert g.n_points(p) == other.n_points(p) == len(pts)


# ---- 4. exact trees ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,ddof,K", [(np.float64, 0, 2000), (np.float64, 1, None), (np.float32, 0, None),
                                          (np.float32, 1, 2000)])
def test_grid_one_pose(dtype, ddof, K):
    pts = synthetic.planar_cloud(60000, dims=(4, 4, 4), seed=1).astype(dtype)
    plane = NotPlanar(MV, 8, ddof)
    crit = [plane] + ([MaxPoints(K)] if K is not None else [])
    clouds = {0: pts}
    og = _ogrid(clouds, crit)
    _, evaluated = _oracle_nodes([m.scheme for m in og.managers.values()], plane, -1 if K is None else K)
    assert evaluated > 3000
    g = _grid(clouds, crit)
    _assert_grid_equal(g, og, clouds)
    if dtype is np.float64 and ddof == 0 and K == 2000:   # (the figures of the CPU test of the same scene)
        assert (evaluated, g.n_nodes(0), g.n_leaves(0)) == (4147, 13480, 8764)
    host = _grid(clouds, _wrapped(crit))
    _assert_grid_equal(g, host, clouds)


@pytest.mark.parametrize("pose_numbers,ddof", [(None, 0), ([0], 0), ([1, 2], 1)])
def test_grid_poses_subset_and_late_pose(pose_numbers, ddof):
    clouds = {p: synthetic.planar_cloud(40000, dims=(3, 3, 3), seed=1, stream=p) for p in range(3)}
    late = synthetic.planar_cloud(20000, dims=(3, 3, 3), seed=1, stream=7)
    plane = NotPlanar(MV, 8, ddof)
    crit = [plane, MaxPoints(2000)]
    og = _ogrid(clouds, crit, pose_numbers)
    _oracle_nodes([m.scheme for m in og.managers.values()], plane, 2000)
    g = _grid(clouds, crit, pose_numbers)
    host = _grid(clouds, _wrapped(crit), pose_numbers)
    _assert_grid_equal(g, og, clouds)
    _assert_grid_equal(g, host, clouds)
    # a pose inserted after the subdivide inherits the scheme
    for x in (g, host, og):
        x.insert_points(9, late)
    clouds[9] = late
    _assert_grid_equal(g, og, clouds)
    _assert_grid_equal(g, host, clouds)


def test_two_poses_figures():
    clouds = {p: synthetic.planar_cloud(40000, dims=(3, 3, 3), seed=1, stream=p) for p in (0, 1)}
    plane = NotPlanar(MV, 8)
    crit = [plane, lambda points: len(points) > 2000]
    og = _ogrid(clouds, crit)
    _, evaluated = _oracle_nodes([m.scheme for m in og.managers.values()], plane, 2000)
    g = _grid(clouds, crit)
    _assert_grid_equal(g, og, clouds)
    assert (evaluated, g.n_nodes(0), g.n_leaves(0)) == (3588, 13907, 7022)


@pytest.mark.parametrize("ddof", [0, 1])
def test_bare_octree(ddof):
    pts = synthetic.planar_cloud(50000, dims=(1, 1, 1), seed=4) * 8.0 + 16.0
    plane = NotPlanar(MV * 64, 8, ddof)
    ot = onp.OTree(np.array([16.0, 16.0, 16.0]), 8.0)
    ot.insert_points(pts)
    ot.subdivide([plane])
    _oracle_nodes([ot], plane, -1)
    assert ot.n_nodes > 100
    trees = []
    for crit in ([plane], _wrapped([plane])):
        t = Octree(OctreeConfig(), np.array([16.0, 16.0, 16.0]), 8.0)
        t.insert_points(pts)
        t.subdivide(crit)
        trees.append(t)
        assert_same_leaves(_views_table(t.get_leaf_points(), pts), canon_from_list(onp.tree_leaf_table(ot)))
        assert (t.n_nodes, t.n_leaves, t.n_points) == (ot.n_nodes, ot.n_leaves, ot.n_points)


@pytest.mark.parametrize("pose_numbers", [None, [0, 2]])
def test_octree_manager(pose_numbers):
    clouds = {p: synthetic.planar_cloud(30000, dims=(1, 1, 1), seed=6, stream=p) * 4.0 for p in range(4)}
    plane = NotPlanar(MV * 16, 8)
    crit = [plane, MaxPoints(5000)]
    om = onp.OManager(np.zeros(3), 4.0)
    for p, pts in clouds.items():
        om.insert_points(p, pts)
    om.subdivide(crit, pose_numbers)
    _oracle_nodes([om.scheme], plane, 5000)
    late = synthetic.planar_cloud(10000, dims=(1, 1, 1), seed=6, stream=8) * 4.0
    managers = []
    for c in (crit, _wrapped(crit)):
        m = OctreeManager(Octree, OctreeConfig(), np.zeros(3), 4.0)
        for p, pts in clouds.items():
            m.insert_points(p, pts)
        m.subdivide(c, pose_numbers)
        m.insert_points(8, late)
        managers.append(m)
    om.insert_points(8, late)
    for p, pts in list(clouds.items()) + [(8, late)]:
        want = canon_from_list(onp.tree_leaf_table(om.octrees[p]))
        for m in managers:
            assert_same_leaves(_views_table(m.get_leaf_points(pose_number=p), pts), want)
            assert (m.n_nodes(p), m.n_leaves(p), m.n_points(p)) == (om.n_nodes(p), om.n_leaves(p), om.n_points(p))


# ---- 5. the arithmetic ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ddof,K", [(0, 2000), (1, -1)])
def test_split_stats_grid(ddof, K):
    pts = synthetic.planar_cloud(60000, dims=(4, 4, 4), seed=1)
    plane = NotPlanar(MV, 8, ddof)
    crit = [plane] + ([MaxPoints(K)] if K >= 0 else [])
    og = _ogrid({0: pts}, crit)
    nodes, evaluated = _oracle_nodes([m.scheme for m in og.managers.values()], plane, K)
    g = _grid({0: pts}, crit)
    assert _check_arithmetic(g._forest, nodes, plane, K) == evaluated


def test_split_stats_far_from_origin():
    """Coordinates around 5e6 with a 1 m voxel: an unshifted one-pass sum of squares (2.5e13 per point, ulp 4e-3)
    cannot resolve a variance of 2.5e-4."""
    pts = synthetic.planar_cloud(40000, dims=(3, 3, 3), seed=2) + np.array([5000000.0, 4999000.0, 5001000.0])
    plane = NotPlanar(MV, 8)
    crit = [plane, MaxPoints(3000)]
    og = _ogrid({0: pts}, crit)
    nodes, evaluated = _oracle_nodes([m.scheme for m in og.managers.values()], plane, 3000)
    g = _grid({0: pts}, crit)
    assert _check_arithmetic(g._forest, nodes, plane, 3000) == evaluated > 1000
    _assert_grid_equal(g, og, {0: pts})


def test_split_stats_big_root_and_pose_subset():
    """One cube, 320 000 points at the root (79 chunks) from four poses of which two drive the scheme: the chunked
    path, and positions that are not scheme points."""
    clouds = {p: synthetic.planar_cloud(80000, dims=(1, 1, 1), seed=9, stream=p, sigma=0.02) * 2.0 for p in range(4)}
    plane = NotPlanar(1.2e-3, 8)
    K, scheme = 20000, [1, 3]
    om = onp.OManager(np.zeros(3), 2.0)
    for p, pts in clouds.items():
        om.insert_points(p, pts)
    om.subdivide([plane, MaxPoints(K)], scheme)
    nodes, evaluated = _oracle_nodes([om.scheme], plane, K)
    everything = np.vstack(list(clouds.values()))
    _, lst = _scheme_nodes(om.scheme, everything)
    counts = {((c + 0.0).tobytes(), e): len(idx) for c, e, _, idx in lst}
    m = OctreeManager(Octree, OctreeConfig(), np.zeros(3), 2.0)
    for p, pts in clouds.items():
        m.insert_points(p, pts)
    m.subdivide([plane, MaxPoints(K)], scheme)
    assert max(counts.values()) == 320000 and max(v[1] for v in nodes.values()) == 160000
    assert _check_arithmetic(m._forest, nodes, plane, K, counts) == evaluated > 50
    for p, pts in clouds.items():
        assert_same_leaves(_views_table(m.get_leaf_points(pose_number=p), pts),
                           canon_from_list(onp.tree_leaf_table(om.octrees[p])))


def test_split_stats_without_planar_build():
    pts = synthetic.planar_cloud(20000, dims=(2, 2, 2), seed=1)
    g = _grid({0: pts}, [MaxPoints(500)])
    cnt, lam = g._forest.split_stats()
    assert len(cnt) == len(g._forest.nodes["edge"]) and not cnt.any() and np.isnan(lam).all()
    g.subdivide([NotPlanar(MV)])
    cnt, lam = g._forest.split_stats()
    assert cnt[:8].sum() == len(pts) and np.isfinite(lam[:8]).all()
    g.subdivide([MaxPoints(500)])
    assert np.isnan(g._forest.split_stats()[1]).all()


# ---- 6. it ran on the device ---------------------------------------------------------------------------------------
def test_criterion_is_not_called(monkeypatch):
    pts = synthetic.planar_cloud(60000, dims=(4, 4, 4), seed=1)
    want = _grid({0: pts}, [NotPlanar(MV), MaxPoints(2000)])

    def boom(self, points):
        raise AssertionError("NotPlanar.__call__ ran on the host")

    monkeypatch.setattr(NotPlanar, "__call__", boom)
    g = _grid({0: pts}, [NotPlanar(MV), MaxPoints(2000)])
    assert g.n_nodes(0) == want.n_nodes(0) == 13480
    t = Octree(OctreeConfig(), np.zeros(3), 4.0)
    t.insert_points(pts)
    t.subdivide([NotPlanar(MV)])
    assert t.n_nodes > 1


def test_host_waits_depend_on_levels_only():
    """One readback per level, as in the count-driven level loop: the same number of host waits for scenes of very
    different size whose trees have the same number of levels.  Counted on the THIRD build of a forest: a device
    buffer that grows is reallocated behind a stream synchronisation (every build path's allocator does that, the
    count-driven loop's too), and both node tables of a forest have reached their size only then."""
    lib, ctx = nat.load(), nat.get_context()

    def build(n, dims):
        f = Forest(0, np.zeros(3), 1.0)
        f.add_pose(synthetic.planar_cloud(n, dims=dims, seed=1))
        info = nat.BuildInfo()
        for _ in range(3):
            before = _syncs()
            ctx.check(lib.octl_forest_build_planar(f.handle, 2000, MV, 8, 0, None, 0, 0, C.byref(info)))
            used = _syncs() - before
        f.close()
        return used, info.n_levels, info.n_nodes

    runs = [build(60000, (4, 4, 4)), build(15000, (2, 2, 2)), build(120000, (4, 4, 8))]
    assert runs[2][2] > 4 * runs[1][2]
    # waits = a + levels, with the same a (a build's fixed readbacks) whatever the points and nodes
    assert len({used - levels for used, levels, _ in runs}) == 1, runs


# ---- 7. determinism and neighbours ---------------------------------------------------------------------------------
def test_same_bits_twice_and_without_the_neighbours():
    pts = synthetic.planar_cloud(60000, dims=(4, 4, 4), seed=1)
    crit = [NotPlanar(MV), MaxPoints(2000)]
    a, b = _grid({0: pts}, crit), _grid({0: pts}, crit)
    ka, ca, la, _ = _device_nodes(a._forest)
    kb, cb, lb, _ = _device_nodes(b._forest)
    assert ka == kb and ca.tobytes() == cb.tobytes() and la.tobytes() == lb.tobytes()
    # the points of one voxel alone: its nodes get the same bits
    sel = (np.floor(pts) == np.array([1.0, 2.0, 3.0])).all(axis=1)
    assert 500 < sel.sum() < 2000
    c = _grid({0: pts[sel]}, crit)
    kc, cc, lc, _ = _device_nodes(c._forest)
    full = {k: (int(n), l.tobytes()) for k, n, l in zip(ka, ca, la)}
    assert len(kc) > 8
    for k, n, l in zip(kc, cc, lc):
        assert full[k] == (int(n), l.tobytes())


def test_downstream_operations_match_host_scheme():
    pts = synthetic.planar_cloud(60000, dims=(4, 4, 4), seed=1)
    crit = [NotPlanar(MV), MaxPoints(2000)]
    dev, host = _grid({0: pts}, crit), _grid({0: pts}, _wrapped(crit))
    sa, sb = dev.leaf_statistics(0), host.leaf_statistics(0)
    for x, y in ((sa.count, sb.count), (sa.mean, sb.mean), (sa.covariance, sb.covariance),
                 (sa.eigenvalues, sb.eigenvalues)):
        assert x.tobytes() == y.tobytes()
    for g in (dev, host):
        np.random.seed(0)
        g.map_leaf_points_cuda_ransac(hypotheses_number=256)
    _assert_grid_equal_after_mask(dev, host, pts)
    for g in (dev, host):
        g.filter([lambda points: len(points) > 20])
    _assert_grid_equal_after_mask(dev, host, pts)
    for g in (dev, host):
        g.subdivide([MaxPoints(100)])
    _assert_grid_equal_after_mask(dev, host, pts)


def _assert_grid_equal_after_mask(a, b, pts):
    ta, tb = _views_table(a.get_leaf_points(0), pts), _views_table(b.get_leaf_points(0), pts)
    assert_same_leaves(ta, tb)
    assert (a.n_nodes(0), a.n_leaves(0), a.n_points(0)) == (b.n_nodes(0), b.n_leaves(0), b.n_points(0))
    assert 0 < a.n_points(0) <= len(pts)


# ---- 8. errors -----------------------------------------------------------------------------------------------------
def test_depth_limit_and_invalid_parameters():
    lib, ctx = nat.load(), nat.get_context()
    pts = synthetic.planar_cloud(60000, dims=(4, 4, 4), seed=1)
    f = Forest(0, np.zeros(3), 1.0)
    f.add_pose(pts)
    info = nat.BuildInfo()
    assert lib.octl_forest_build_planar(f.handle, 2000, MV, 8, 0, None, 0, 2, C.byref(info)) == nat.OCTL_E_DEPTH
    assert b"depth" in lib.octl_last_error(ctx.handle)
    n = C.c_int64(0)
    assert lib.octl_forest_get_nodes(f.handle, 0, None, None, None, None, None, None, None, C.byref(n)) \
        == nat.OCTL_E_STATE   # no scheme ...
    for bad in ((2000, 0.0, 8, 0), (2000, -1.0, 8, 0), (2000, float("nan"), 8, 0), (2000, float("inf"), 8, 0),
                (2000, MV, 3, 0), (2000, MV, 8, 2), (2000, MV, 8, -1)):
        assert lib.octl_forest_build_planar(f.handle, bad[0], bad[1], bad[2], bad[3], None, 0, 0, C.byref(info)) \
            == nat.OCTL_E_INVALID
        assert b"build_planar" in lib.octl_last_error(ctx.handle)
    mask = np.ones(3, dtype=np.uint8)
    assert lib.octl_forest_build_planar(f.handle, 2000, MV, 8, 0, nat.ptr(mask), 3, 0, C.byref(info)) \
        == nat.OCTL_E_INVALID
    # ... but the points are kept: the same forest builds with room enough
    ctx.check(lib.octl_forest_build_planar(f.handle, 2000, MV, 8, 0, None, 0, 0, C.byref(info)))
    assert (info.n_points, info.n_nodes) == (60000, 13480)
    f.close()
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, pts)
    with pytest.raises(RecursionError):
        g._forest.subdivide_planar((2000, MV, 8, 0), None, max_depth=2)
    g.subdivide([NotPlanar(MV), MaxPoints(2000)])
    assert g.n_nodes(0) == 13480
