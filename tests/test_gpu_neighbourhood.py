"""Neighbourhood statistics and point normals on the device: octl_forest_neighbourhood_stats / _device /
octl_forest_point_stats and octreelib_amd.neighbourhood_statistics / point_statistics over a Grid, an OctreeManager and
an Octree.

The contract, derived and not measured: count[i] EQUALS radius_count and radius_count_np; with n >= 1
neighbours within R = max |p - q|_inf of the query and g = (n + 16) 2^-53 every mean component is within 2 g R + 2^-53 |m|
and every covariance entry within 4 g R^2 of the exact moments of the f64 neighbour rows - checked against exact
rationals on at most 64 rows of at most 100 neighbours per case and against the longdouble definition on the rest; the
eigen-decomposition satisfies tests/test_gpu_leaf_stats.py: _assert_eigen on the device's own covariance; and the same
map and the same query bits give the same row bits however the query arrives.  Maps hold at most 20 k points, batches
at most 2 k queries."""

import ctypes as C
import functools

import numpy as np
import pytest

from octreelib_amd import (DeviceCloud, MaxPoints, PointStatistics, neighbourhood_statistics,
                           neighbourhood_statistics_np, point_statistics, radius_count_np, synthetic, thin)
from octreelib_amd import _native as nat
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree_manager import OctreeManager
from oracle.octree_np import OGrid
from tests._neighbourhood import assert_exact_bound, assert_reference_bound, neighbours_of, pick_rows
from tests.test_cpu_query import _grid_map
from tests.test_cpu_radius import lattice
from tests.test_gpu_leaf_stats import _assert_eigen
from tests.test_gpu_query import BAD, _counter, _DevBuf

pytestmark = pytest.mark.gpu

FIELDS = ("count", "mean", "covariance", "eigenvalues", "eigenvectors")


# ---- helpers -------------------------------------------------------------------------------------------------------
def _grid(clouds, K, L=1):
    g = Grid(GridConfig(voxel_edge_length=L))
    for p, P in clouds.items():
        g.insert_points(p, P)
    g.subdivide([MaxPoints(K)])
    return g


def _bytes(st, rows=slice(None)):
    return tuple(getattr(st, k)[rows].tobytes() for k in FIELDS if getattr(st, k) is not None)


def _check(obj, Q, clouds, r, what, pose_numbers=None, octree=False, limit=64):
    """neighbourhood_statistics of `obj` against the definition over `clouds`: the counts, the NaN rows, the bound
    (rationals on `limit` rows, the longdouble definition on every row), the eigen contract, eigen=False.  Returns
    (statistics, counts of the definition)."""
    kw = {} if octree else {"pose_numbers": pose_numbers}
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    assert len(Q) <= 2000 and sum(len(c) for _, c in clouds) <= 20000, what
    st = neighbourhood_statistics(obj, Q, r, **kw)
    want = radius_count_np(Q, clouds, r)
    assert st.count.dtype == np.int64 and st.mean.shape == (len(Q), 3) and st.covariance.shape == (len(Q), 3, 3), what
    assert st.eigenvalues.shape == (len(Q), 3) and st.eigenvectors.shape == (len(Q), 3, 3), what
    if not np.array_equal(st.count, want):
        bad = np.nonzero(st.count != want)[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(Q)} counts differ, first {int(bad[0])} at "
                             f"{Q[bad[0]].tolist()}: got {int(st.count[bad[0]])}, expected {int(want[bad[0]])}")
    assert np.array_equal(obj.radius_count(Q, r, **kw), want), what
    none = want == 0
    for k in FIELDS[1:]:
        a = getattr(st, k)
        assert np.isnan(a[none]).all() and np.isfinite(a[~none]).all(), (what, k)
    lists = neighbours_of(Q, clouds, r)
    worst = assert_exact_bound(st, Q, lists, pick_rows(want, limit), what)
    print(f"{what}, r={r}: n up to {int(want.max())}; largest error / bound on the exact rows: mean {worst[0]:.3f}, "
          f"covariance {worst[1]:.3f}")
    ref = neighbourhood_statistics_np(Q, clouds, r, dtype=np.longdouble, eigen=False)
    assert_reference_bound(st, ref, Q, lists, np.nonzero(~none)[0], what)
    _assert_eigen(st.eigenvalues[~none], st.eigenvectors[~none], st.covariance[~none], gap_check=False)
    one = want == 1
    assert np.all(st.covariance[one] == 0.0) and np.all(st.eigenvalues[one] == 0.0), what
    assert np.all(st.surface_variation[one] == 0.0), what
    plain = neighbourhood_statistics(obj, Q, r, eigen=False, **kw)
    assert plain.eigenvalues is None and plain.eigenvectors is None and _bytes(plain) == _bytes(st)[:3], what
    return st, want


@functools.lru_cache(maxsize=None)
def _scene():
    """About 4 k points in two poses over the voxels (0,0,0), (1,0,0), (0,1,0) - (1,1,0) is missing - with rows snapped to
    the 1/8 lattice (on leaf and voxel walls), and the queries of test 1: stored points, points on leaf and voxel walls,
    points in the missing voxel and outside every voxel, queries that are not finite."""
    rng = np.random.default_rng(4)
    P = np.concatenate([np.array(v, dtype=np.float64) + rng.random((1300, 3)) for v in ((0, 0, 0), (1, 0, 0), (0, 1, 0))])
    P[::7] = np.floor(P[::7] * 8) / 8
    clouds = {0: np.ascontiguousarray(P[::2]), 1: np.ascontiguousarray(P[1::2])}
    walls = rng.random((200, 3)) * [2.0, 1.0, 1.0]
    walls[:100, 0] = 1.0                                                    # the wall between two voxels
    walls[100:, 1] = np.floor(walls[100:, 1] * 8) / 8                       # leaf walls
    outside = np.concatenate([[1.0, 1.0, 0.0] + rng.random((100, 3)), rng.uniform(-0.6, 0.0, (100, 3)),
                              [0.0, 0.0, 1.0] + rng.random((50, 3)) * [2.0, 1.0, 0.1]])
    Q = np.concatenate([P[rng.permutation(len(P))[:400]], P[::7][:200], walls, outside, BAD])
    for a in (*clouds.values(), Q):
        a.setflags(write=False)
    return clouds, np.ascontiguousarray(Q)


def _listed(clouds, names=None):
    return [(p, clouds[p]) for p in (clouds if names is None else names)]


def _alive(obj, clouds):
    """{pose: sorted rows of the cloud as inserted that are still in the map}, read from the leaf-ordered arrays: the
    store index of every position against the offsets of the poses, checked against the coordinates."""
    f = obj._forest
    names = [p for p, _ in sorted(getattr(obj, "_slots", {0: 0}).items(), key=lambda kv: kv[1])]   # (an Octree: pose 0)
    off = np.concatenate([[0], np.cumsum(f.slot_sizes)]).astype(np.int64)
    perm = np.asarray(f.perm, dtype=np.int64)
    slot = np.searchsorted(off, perm, side="right") - 1
    index = perm - off[slot]
    out = {}
    for s, p in enumerate(names):
        rows = np.sort(index[slot == s])
        assert np.asarray(clouds[p])[index[slot == s]].tobytes() == f.xyz[slot == s].tobytes()
        out[p] = rows
    return out


def _check_points(obj, clouds, r, what, pose_numbers=None, among=None, limit=32):
    """point_statistics of `obj` against the definition over the rows of `clouds` that are still in the map (or, with
    pending: before a pending mask is applied): rows, (pose, index), counts, the bound, the eigen contract."""
    alive = _alive(obj, clouds)
    names = list(alive)
    counted = [(p, clouds[p][alive[p]]) for p in names if among is None or p in among]
    tested = [p for p in names if pose_numbers is None or p in pose_numbers]
    ps = point_statistics(obj, r, pose_numbers=pose_numbers, among=among)
    assert isinstance(ps, PointStatistics) and ps.pose.dtype == np.int32 and ps.index.dtype == np.int32, what
    assert ps.pose.tolist() == sum(([p] * len(alive[p]) for p in tested), []), what
    assert np.array_equal(ps.index, np.concatenate([alive[p] for p in tested] + [np.empty(0, dtype=np.int64)])), what
    X = np.concatenate([clouds[p][alive[p]] for p in tested] + [np.empty((0, 3))])
    assert len(X) <= 20000, what
    want = radius_count_np(X, counted, r)
    assert np.array_equal(ps.count, want), what
    rows = np.unique(np.linspace(0, len(X) - 1, min(len(X), 400)).astype(np.int64)) if len(X) else np.empty(0, dtype=np.int64)
    sub = LeafRows(ps, rows)
    lists = neighbours_of(X[rows], counted, r)
    assert_exact_bound(sub, X[rows], lists, pick_rows(want[rows], limit), what)
    some = want[rows] > 0
    _assert_eigen(sub.eigenvalues[some], sub.eigenvectors[some], sub.covariance[some], gap_check=False)
    for k in FIELDS[1:]:
        assert np.isnan(getattr(ps, k)[want == 0]).all(), (what, k)
    return ps, X


class LeafRows:
    """The rows `rows` of a statistics object, as the checkers read them."""

    def __init__(self, st, rows):
        for k in FIELDS:
            setattr(self, k, getattr(st, k)[rows])


# ---- 1. small neighbourhoods against Fractions -------------------------------------------------------------------------
def test_small_neighbourhoods_against_exact_moments():
    clouds, Q = _scene()
    g = _grid(clouds, 16)
    assert g._forest.nodes["depth"].max() >= 2 and len(g._forest.voxels) == 3
    st, c = _check(g, Q, _listed(clouds), 0.15, "scene")
    n_stored = 600
    assert c[:n_stored].min() >= 1 and c.max() > 16 and (c[n_stored:-len(BAD)] == 0).any() and np.all(c[-len(BAD):] == 0)
    assert c[n_stored:n_stored + 200].min() >= 1 and c[n_stored:n_stored + 200].mean() > 8     # the queries on the walls
    # normals of a plane: the smallest eigenvalue's vector, up to sign
    _check(g, Q[::3], _listed(clouds, [1]), 0.15, "scene, pose 1", pose_numbers=[1], limit=24)


# ---- 2. exact ties on the sphere ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0.25, 0.375])
def test_ties_on_the_sphere_enter_the_moments(r):
    P = lattice()
    clouds = {0: np.ascontiguousarray(P[::2]), 1: np.ascontiguousarray(P[1::2])}
    g = _grid(clouds, 8)
    assert g._forest.nodes["depth"].max() >= 2
    S = np.ascontiguousarray(P[::5])
    inside = radius_count_np(S, _listed(clouds), np.nextafter(r, 0.0))
    st, c = _check(g, S, _listed(clouds), r, f"lattice r={r}")
    assert (c > inside).all()                                               # d2 == r2 holds for neighbours of every query
    # an ulp off the lattice, a neighbour on the sphere is lost or kept as the definition's d2 says
    up, down = np.nextafter(S[::2], np.inf), np.nextafter(S[::2], -np.inf)
    Qu = np.concatenate([np.column_stack([up[:, 0], S[::2, 1], S[::2, 2]]), np.column_stack([down[:, 0], up[:, 1], down[:, 2]])])
    _, cu = _check(g, Qu, _listed(clouds), r, f"lattice r={r}, an ulp off", limit=32)
    assert (cu < np.tile(c[::2], 2)).any()


# ---- 3. the radius at the cap ------------------------------------------------------------------------------------------
def test_the_radius_at_the_cap_a_cube_and_an_octree():
    rng = np.random.default_rng(8)
    vox = np.argwhere(np.ones((3, 3, 2), dtype=bool)) - [2, 1, 1]
    P = np.concatenate([v + rng.random((70, 3)) for v in vox])
    clouds = {3: np.ascontiguousarray(P[::2]), 5: np.ascontiguousarray(P[1::2])}
    g = _grid(clouds, 12)
    Q = np.concatenate([P[::9], rng.uniform(-3.0, 2.0, (100, 3)), BAD])
    _, c = _check(g, Q, _listed(clouds), 2.0, "grid at 2 L", limit=8)
    assert c.max() > 600
    # one cube whose corner is not dyadic, under a manager (no cap on the radius) ...
    c0, e0 = 0.1, 3.3
    X = c0 + rng.random((3000, 3)) * e0 * [1.0, 1.0, 0.3]
    X = X[np.all((X - c0 >= 0) & (X - c0 < e0), axis=1)]
    m = OctreeManager(Octree, OctreeConfig(), np.array([c0, c0, c0]), e0)
    m.insert_points(4, X[::2])
    m.insert_points(9, X[1::2])
    m.subdivide([MaxPoints(20)])
    assert m._forest.nodes["depth"].max() >= 3
    Qm = np.concatenate([X[:300] + rng.normal(0.0, 0.01, (300, 3)), X[:100], rng.uniform(-0.5, 4.0, (100, 3)), BAD])
    cm = [(4, X[::2]), (9, X[1::2])]
    _, c = _check(m, Qm, cm, 0.2, "manager", limit=32)
    assert c.max() > 16 and (c == 0).any()
    _, c9 = _check(m, Qm[::4], cm[1:], 0.2, "manager, pose 9", pose_numbers=[9], limit=8)
    assert (c9 <= c[::4]).all() and (c9 < c[::4]).any()
    _, call = _check(m, Qm[:40], cm, 7.0, "manager, every point", limit=1)
    assert np.all(call == len(X))
    # ... and as an Octree
    t = Octree(OctreeConfig(), np.array([c0, c0, c0]), e0)
    t.insert_points(X)
    t.subdivide([MaxPoints(20)])
    st, c = _check(t, Qm, [(0, X)], 0.2, "octree", octree=True, limit=16)
    ps, _ = _check_points(t, {0: X}, 0.2, "octree, self-query")
    assert len(ps) == len(X) and np.all(ps.pose == 0)


# ---- 4. a large neighbourhood ------------------------------------------------------------------------------------------
def test_a_large_neighbourhood_across_many_leaves():
    rng = np.random.default_rng(12)
    d = rng.normal(size=(6000, 3))
    blob = [0.5, 0.5, 0.5] + 0.2 * d / np.linalg.norm(d, axis=1)[:, None] * rng.random((6000, 1)) ** (1.0 / 3.0)
    back = rng.random((2000, 3)) * [2.0, 1.0, 1.0]
    clouds = {0: np.ascontiguousarray(np.concatenate([blob[:3000], back])), 1: np.ascontiguousarray(blob[3000:])}
    g = _grid(clouds, 64)
    assert (g._forest.nodes["first_child"] < 0).sum() > 64
    Q = np.concatenate([[[0.5, 0.5, 0.5]], [0.5, 0.5, 0.5] + rng.normal(0.0, 0.03, (40, 3)), blob[:20]])
    st, c = _check(g, Q, _listed(clouds), 0.25, "blob", limit=4)
    assert c[0] >= 6000 and (c > 4096).sum() > 20
    # isotropic scatter: the surface variation is near a third
    assert abs(st.surface_variation[0] - 1.0 / 3.0) < 0.03


# ---- 5. far from the origin --------------------------------------------------------------------------------------------
def test_the_bound_does_not_know_the_magnitude_of_the_coordinates():
    clouds, Q = _scene()
    off = 2.0 ** 20
    far = {p: c + off for p, c in clouds.items()}
    Qf = Q + off                                                            # (every sum exact: 1/8-lattice rows stay on it)
    g = _grid(far, 16)
    st, c = _check(g, Qf, _listed(far), 0.15, "scene at 2^20")
    _, c0 = _check(_grid(clouds, 16), Q[:300], _listed(clouds), 0.15, "scene", limit=8)
    assert c.max() > 16 and c[:300].min() >= 1
    m = OctreeManager(Octree, OctreeConfig(), np.array([off - 1.0, off - 1.0, off - 1.0]), 4.0)
    for p, X in far.items():
        m.insert_points(p, X)
    m.subdivide([MaxPoints(16)])
    _check(m, Qf[::2], _listed(far), 0.15, "scene at 2^20, manager", limit=32)


# ---- 6. selections and edits -------------------------------------------------------------------------------------------
def test_selections_edits_and_a_pending_mask():
    clouds = {p: synthetic.planar_cloud(2500, (2, 2, 2), seed=6, stream=p, sigma=0.002) for p in (0, 1, 2, 3)}
    g = _grid(clouds, 48)
    f = g._forest
    r = 0.08
    every, X = _check_points(g, clouds, r, "as inserted")
    assert len(every) == 10000 and every.count.min() >= 1 and every.count.max() > 8       # a point counts itself
    new, _ = _check_points(g, clouds, r, "newest pose", pose_numbers=[3])
    assert np.array_equal(new.count, every.count[every.pose == 3]) and _bytes(new) == _bytes(every, every.pose == 3)
    # a tested pose that is not counted has no point of its own among its neighbours
    old, _ = _check_points(g, clouds, r, "newest pose against the older ones", pose_numbers=[3], among=[0, 1, 2])
    assert (old.count < new.count).all()
    mixed, _ = _check_points(g, clouds, r, "two tested, two counted", pose_numbers=[2, 0], among=[0, 1])
    assert mixed.pose.tolist() == [0] * 2500 + [2] * 2500
    Q = np.ascontiguousarray(np.concatenate([clouds[1][:300] + 0.003, BAD]))
    _, c = _check(g, Q, _listed(clouds, [2, 0]), r, "poses 2 and 0", pose_numbers=[2, 0], limit=16)
    assert c.max() > 4
    stamp = (f.n_ord, len(f.nodes["depth"]))
    # a pending RANSAC mask: what it is about to drop still has rows and still counts
    np.random.seed(0)
    f.ransac_blocks(np.ascontiguousarray(f.order), np.random.random((128, 6)), 0.01)
    mask = f.device_mask()
    assert 0 < mask.sum() < len(mask)
    pend, _ = _check_points(g, clouds, r, "a mask is pending")
    assert _bytes(pend) == _bytes(every) and np.array_equal(pend.index, every.index)
    assert np.array_equal(f.device_mask(), mask) and (f.n_ord, len(f.nodes["depth"])) == stamp   # nothing changed
    # edits: what left has no row and does not count, the rows of the rest keep their index
    keep = np.random.default_rng(1).random(f.n_ord) < 0.8
    f.apply_host_mask(keep.astype(np.uint8))
    n = [f.n_ord]
    masked, _ = _check_points(g, clouds, r, "after apply_mask")
    assert len(masked) == n[0] < 10000
    from tests._raycast import box_rays

    rng = np.random.default_rng(2)
    O, D = box_rays(rng, [0, 0, 0], [2, 2, 2], 3000, 0.5)
    assert g.carve_rays(O, D, rng.uniform(0.3, 2.5, 3000), 0.05) > 0
    _check_points(g, clouds, r, "after carve", limit=16)
    assert g.remove_sparse(0.05, 6) > 0
    _check_points(g, clouds, r, "after remove_sparse", limit=16)
    assert thin(g, 0.02) > 0
    thinned, _ = _check_points(g, clouds, r, "after thin", limit=16)
    assert g.remove_poses([1]) > 0
    left, _ = _check_points(g, clouds, r, "after remove_poses", limit=16)
    assert sorted(set(left.pose.tolist())) == [0, 2, 3] and len(left) == f.n_ord < len(thinned)
    # a row that survived every edit names the same row of its cloud
    key = lambda ps: set(zip(ps.pose.tolist(), ps.index.tolist()))
    assert key(left) < key(thinned) < key(masked) < key(every)
    _check_points(g, clouds, r, "after remove_poses, poses 3 and 2", pose_numbers=[3, 2], among=[2], limit=16)
    with pytest.raises(KeyError):
        point_statistics(g, r, pose_numbers=[1])


# ---- 7. the same bits --------------------------------------------------------------------------------------------------
def test_the_same_query_bits_give_the_same_row_bits():
    clouds, Q = _scene()
    g = _grid(clouds, 16)
    r = 0.15
    st = neighbourhood_statistics(g, Q, r)
    assert _bytes(neighbourhood_statistics(g, Q, r)) == _bytes(st)                       # a second call
    assert _bytes(neighbourhood_statistics(g, DeviceCloud(Q), r)) == _bytes(st)          # read where it lies
    perm = np.random.default_rng(0).permutation(len(Q))
    assert _bytes(neighbourhood_statistics(g, Q[perm], r)) == _bytes(st, perm)           # a permuted batch
    assert _bytes(neighbourhood_statistics(g, Q[5:6], r)) == _bytes(st, slice(5, 6))     # alone
    assert _bytes(neighbourhood_statistics(g, Q.astype(np.float64).tolist(), r)) == _bytes(st)
    sub = neighbourhood_statistics(g, Q, r, pose_numbers=[1])
    assert _bytes(sub) != _bytes(st) and _bytes(neighbourhood_statistics(g, DeviceCloud(Q), r, pose_numbers=[1])) == _bytes(sub)
    plain = neighbourhood_statistics(g, DeviceCloud(Q), r, eigen=False)
    assert plain.eigenvalues is None and _bytes(plain) == _bytes(st)[:3]
    # the row of a stored point in the self-query is the row of the query with the same bits and the same selection
    for tested, among in ((None, None), ([1], None), ([0], [1]), ([1, 0], [0])):
        ps = point_statistics(g, r, pose_numbers=tested, among=among)
        X = np.concatenate([clouds[p][ps.index[ps.pose == p]] for p in sorted(set(ps.pose.tolist()))])
        assert len(ps) == sum(len(clouds[p]) for p in (tested or clouds)) and len(X) == len(ps)
        rows = np.unique(np.linspace(0, len(X) - 1, 1500).astype(np.int64))
        one = neighbourhood_statistics(g, X[rows], r, pose_numbers=among)
        assert _bytes(one) == _bytes(ps, rows), (tested, among)
        assert (ps.count > 1).any()
    with pytest.raises(ValueError, match="float64"):
        neighbourhood_statistics(g, DeviceCloud(Q[:10].astype(np.float32)), r)


# ---- 8. degenerate rows ------------------------------------------------------------------------------------------------
def test_degenerate_rows_and_an_empty_map():
    rng = np.random.default_rng(3)
    lone = np.array([[0.5, 0.5, 0.5], [3.5, 0.5, 0.5], [3.5, 0.5, 0.5], [5.25, 0.5, 0.5], [5.375, 0.5, 0.5]])
    P = np.concatenate([lone, [7.0, 0.0, 0.0] + rng.random((200, 3))])
    g = _grid({0: P}, 16)
    Q = np.concatenate([[[0.6, 0.45, 0.5], [0.5, 0.5, 0.5], [3.5, 0.5, 0.5], [5.3125, 0.5, 0.5], [1.5, 0.5, 0.5]], BAD])
    st, c = _check(g, Q, [(0, P)], 0.2, "degenerate")
    assert c.tolist() == [1, 1, 2, 2, 0] + [0] * len(BAD)
    assert np.all(st.covariance[:2] == 0.0) and np.all(st.eigenvalues[:2] == 0.0) and np.all(st.surface_variation[:2] == 0.0)
    assert np.array_equal(st.eigenvectors[0], np.eye(3)) and st.mean[1].tolist() == [0.5, 0.5, 0.5]
    assert np.all(st.covariance[2] == 0.0) and st.mean[2].tolist() == [3.5, 0.5, 0.5]      # two duplicates: no spread
    assert st.covariance[3, 0, 0] == 2.0 ** -8 and np.count_nonzero(st.covariance[3]) == 1  # 1/8 apart along x
    assert st.normal[3, 0] == 0.0 and st.surface_variation[3] == 0.0
    assert np.isnan(st.mean[4:]).all() and np.isnan(st.covariance[4:]).all() and np.isnan(st.eigenvalues[4:]).all()
    assert np.isnan(st.eigenvectors[4:]).all()
    ps = point_statistics(g, 0.2)
    assert ps.count[:5].tolist() == [1, 2, 2, 2, 2] and np.all(ps.covariance[:3] == 0.0) and len(ps) == len(P)
    e = neighbourhood_statistics(g, np.empty((0, 3)), 0.2)
    assert len(e) == 0 and e.mean.shape == (0, 3) and e.eigenvectors.shape == (0, 3, 3)
    # a map that has lost every point, and one cube that never had one
    g.filter([lambda pts: False])
    assert g._forest.n_ord == 0
    st = neighbourhood_statistics(g, Q, 0.2)
    assert np.all(st.count == 0) and np.isnan(st.mean).all() and np.isnan(st.eigenvectors).all()
    ps = point_statistics(g, 0.2)
    assert len(ps) == 0 and ps.mean.shape == (0, 3) and ps.pose.shape == (0,)


# ---- 9. refusals -------------------------------------------------------------------------------------------------------
def test_refusals():
    clouds, Q = _scene()
    g = Grid(GridConfig(voxel_edge_length=1))
    for p, P in clouds.items():
        g.insert_points(p, P)
    f = g._forest
    lib, h = f.lib, f.handle
    n = len(Q)
    mean, cov = np.full((n, 3), -7.0), np.full((n, 6), -7.0)

    def abi(m, r, sel=None, n_sel=0, q=Q):
        return lib.octl_forest_neighbourhood_stats(h, nat.ptr(q), m, r, nat.ptr(sel), n_sel, None, nat.ptr(mean),
                                                   nat.ptr(cov), None, None)

    rows = C.c_int64(-5)
    self_abi = lambda r, cap=0, sel=None, n_sel=0: lib.octl_forest_point_stats(
        h, r, nat.ptr(sel), n_sel, None, 0, cap, C.byref(rows), None, None, None, None, None, None, None)
    assert abi(100, 0.1) == nat.OCTL_E_STATE and b"neighbourhood_stats before build" in lib.octl_last_error(f.ctx.handle)
    assert self_abi(0.1) == nat.OCTL_E_STATE and b"point_stats before build" in lib.octl_last_error(f.ctx.handle)
    g.subdivide([MaxPoints(16)])
    for r in (0.0, -0.5, float("nan"), float("inf"), 2.0000001):
        assert abi(100, r) == nat.OCTL_E_INVALID and self_abi(r) == nat.OCTL_E_INVALID
        with pytest.raises(ValueError):
            neighbourhood_statistics(g, Q[:10], r)
        with pytest.raises(ValueError):
            point_statistics(g, r)
    assert b"voxel edge" in lib.octl_last_error(f.ctx.handle)
    with pytest.raises(ValueError, match="neighbourhood_statistics"):
        neighbourhood_statistics(g, Q[:10], "x")
    with pytest.raises(ValueError, match="point_statistics"):
        point_statistics(g, None)
    assert abi(-1, 0.1) == nat.OCTL_E_INVALID and abi(2 ** 31, 0.1) == nat.OCTL_E_INVALID
    assert abi(100, 0.1, q=None) == nat.OCTL_E_INVALID
    assert abi(100, 0.1, np.ones(3, dtype=np.uint8), 3) == nat.OCTL_E_INVALID
    assert self_abi(0.1, sel=np.ones(3, dtype=np.uint8), n_sel=3) == nat.OCTL_E_INVALID
    assert self_abi(0.1, cap=-1) == nat.OCTL_E_INVALID
    assert lib.octl_forest_neighbourhood_stats(h, nat.ptr(Q), 10, 0.1, None, 0, None, None, None, nat.ptr(mean), None) \
        == nat.OCTL_E_INVALID                                                              # eigenvalues without vectors
    assert np.all(mean == -7.0) and np.all(cov == -7.0) and rows.value == -5               # nothing ran
    a = _counter("octl_debug_launches")
    assert abi(0, 0.1) == 0 and lib.octl_forest_neighbourhood_stats_device(h, None, 0, 0.1, None, 0, None, None, None,
                                                                          None, None) == 0
    assert _counter("octl_debug_launches") == a                                            # no kernel
    assert self_abi(0.1) == 0 and rows.value == sum(len(c) for c in clouds.values())        # a size query
    assert abi(100, 2.0) == 0                                                              # (twice the voxel edge is allowed)
    with pytest.raises(ValueError):
        neighbourhood_statistics(g, np.zeros((4, 2)), 0.1)
    for call in (lambda: neighbourhood_statistics(g, Q[:10], 0.1, pose_numbers=[7]),
                 lambda: point_statistics(g, 0.1, pose_numbers=[7]), lambda: point_statistics(g, 0.1, among=[7])):
        with pytest.raises(KeyError):
            call()
    with pytest.raises(ValueError, match="float64"):
        neighbourhood_statistics(g, DeviceCloud(Q[:10].astype(np.float32)), 0.1)
    for other in (None, 3, np.zeros((4, 3)), f):
        with pytest.raises(TypeError):
            neighbourhood_statistics(other, Q[:10], 0.1)
        with pytest.raises(TypeError):
            point_statistics(other, 0.1)
    t = Octree(OctreeConfig(), np.zeros(3), 2.0)
    t.insert_points(clouds[0][:500])
    t.subdivide([MaxPoints(16)])
    with pytest.raises(ValueError, match="single pose"):
        neighbourhood_statistics(t, Q[:10], 0.1, pose_numbers=[0])
    with pytest.raises(ValueError, match="single pose"):
        point_statistics(t, 0.1, pose_numbers=[0])
    with pytest.raises(ValueError, match="single pose"):
        point_statistics(t, 0.1, among=[0])
    assert neighbourhood_statistics(t, Q[:10], 5.0).count.tolist() == [500] * 10           # one cube has no cap
    # rows moved outside their leaves: no cube bounds what it holds
    g.map_leaf_points(lambda p: p + np.array([0.0, 0.0, 0.4]), [1])
    with pytest.raises(RuntimeError, match="outside their leaves"):
        neighbourhood_statistics(g, Q[:10], 0.1)
    with pytest.raises(RuntimeError, match="outside their leaves"):
        point_statistics(g, 0.1)
    assert abi(100, 0.1) == nat.OCTL_E_STATE and self_abi(0.1) == nat.OCTL_E_STATE


# ---- 10. launches ------------------------------------------------------------------------------------------------------
def _launches(fn):
    a, b = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
    out = fn()
    return out, (_counter("octl_debug_launches") - a, _counter("octl_debug_host_syncs") - b)


def test_launches_and_waits_do_not_depend_on_the_sizes():
    P = synthetic.planar_cloud(20000, (3, 3, 2), seed=3)
    rng = np.random.default_rng(7)
    Q = np.ascontiguousarray(P[rng.permutation(20000)[:2000]] + rng.normal(0.0, 0.01, (2000, 3)))
    seen = {}
    for size in (2000, 20000):
        g = _grid({0: P[:size // 2], 1: P[size // 2:size]}, 64)
        f = g._forest
        lib, h = f.lib, f.handle
        n = len(Q)
        outs = [np.empty(n, dtype=np.int64), np.empty((n, 3)), np.empty((n, 6)), np.empty((n, 3)), np.empty((n, 9))]
        host = lambda m: lib.octl_forest_neighbourhood_stats(h, nat.ptr(Q), m, 0.1, None, 0, *[nat.ptr(a) for a in outs])
        xin = _DevBuf(f.ctx, Q.nbytes)
        bufs = [_DevBuf(f.ctx, a.nbytes) for a in outs]
        try:
            xin.upload(Q)
            dev = lambda m: lib.octl_forest_neighbourhood_stats_device(h, xin.p, m, 0.1, None, 0, *[b.p for b in bufs])
            for name, fn, expect in (("host", host, (1, 1)), ("device", dev, (1, 0))):
                assert fn(n) == 0                  # (warm: staging allocated, voxel codes and the index on the device)
                f.ctx.sync()
                for m in (1, 100, 2000):
                    rc, got = _launches(lambda: fn(m))
                    assert rc == 0 and got == expect, (name, size, m, got)
                f.ctx.sync()
            for a, b in zip(outs, bufs):
                assert b.download(a.shape, a.dtype).tobytes() == a.tobytes()
        finally:
            xin.free()
            for b in bufs:
                b.free()
        assert (outs[0] > 1).any()
        point_statistics(g, 0.1)                   # (warm)
        for kw in ({}, {"pose_numbers": [1]}):
            point_statistics(g, 0.1, **kw)
            ps, got = _launches(lambda: point_statistics(g, 0.1, **kw))
            assert len(ps) == (size if not kw else size // 2) and (ps.count > 1).any()
            seen.setdefault(str(kw), []).append(got)
    for kw, costs in seen.items():
        assert costs[0] == costs[1] and costs[0][0] <= 2 and costs[0][1] <= 2, (kw, costs)   # a fill and the kernel


# ---- 11. the plug path -------------------------------------------------------------------------------------------------
def test_the_plug_path_agrees_within_the_bound():
    clouds, Q = _scene()
    og = OGrid(1)
    for p, P in clouds.items():
        og.insert_points(p, P)
    og.subdivide(16)
    hm = _grid_map(og, 1)
    g = _grid(clouds, 16)
    r = 0.15
    Qs = Q[::2]
    dev, host = neighbourhood_statistics(g, Qs, r), hm.neighbourhood_statistics(Qs, r)
    assert np.array_equal(dev.count, host.count) and (dev.count > 1).any()
    lists = neighbours_of(Qs, hm.clouds(), r)
    some = np.nonzero(dev.count > 0)[0]
    assert_reference_bound(dev, host, Qs, lists, some, "plug path", rounded=True)
    assert_exact_bound(host, Qs, lists, pick_rows(host.count, 24), "plug path, host")
    hp, dp = hm.point_statistics(r, pose_numbers=[1]), point_statistics(g, r, pose_numbers=[1])
    # (a HostMap knows a pose through its leaves: its rows are in leaf order, the device's in insertion order)
    assert sorted(hp.count.tolist()) == sorted(dp.count.tolist()) and len(hp) == len(dp) == len(clouds[1])
