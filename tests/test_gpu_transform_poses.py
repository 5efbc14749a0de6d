"""Write adjusted poses back into the map: octl_forest_transform_poses and Grid / OctreeManager .transform_poses.

The oracle is a TWIN: map A is built, fitted and filtered, then moved in place; map B is a fresh object into which the
surviving rows of every pose (store order, from Forest.perm) are inserted again, those of the selected poses through
registration.transform_np.  Both sides are defined by transform_np, so every comparison is np.array_equal on bits -
there is no tolerance to state.  The only difference the definition allows: A's rows keep their store positions, so
its neighbour indices name rows of the clouds as they were first inserted (index_A == rows[index_B]).

The kernel takes 1024 rows per workgroup and two pairs of rows per thread (store.hip: XF_ROWS_PER_WG, XF_PAIRS; the CPU
test pins the constant), hence the pose sizes of test_shapes."""

import dataclasses

import numpy as np
import pytest

from octreelib_amd import MaxPoints, NotPlanar, synthetic
from octreelib_amd import _native as nat
from octreelib_amd.feed import DeviceCloud
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree_manager import OctreeManager
from octreelib_amd.registration import se3_exp, transform_np
from tests._util import assert_same_leaves, canon
from tests.test_gpu_query import _counter

pytestmark = pytest.mark.gpu

ROWS_PER_WG = 1024          # store.hip: XF_ROWS_PER_WG
LAUNCHES_PER_CALL = 1       # one kernel (the table is one copy, the box one 32-byte copy)
COUNT = [MaxPoints(48)]
PLANAR = [MaxPoints(400), NotPlanar(2.5e-4, min_points=8)]


# ---- helpers -------------------------------------------------------------------------------------------------------
def _grid():
    return Grid(GridConfig(voxel_edge_length=1))


def _rigid(axis, angle, t):
    """A rotation of `angle` radians about `axis` through the origin, then the translation t: 4x4."""
    w = np.asarray(axis, dtype=np.float64)
    return se3_exp(np.concatenate([w / np.linalg.norm(w) * angle, np.asarray(t, dtype=np.float64)]))


def _rows(f):
    """Per slot: the rows of the inserted cloud that are still alive, in store order (ascending)."""
    off = np.concatenate([[0], np.cumsum(f.slot_sizes)]).astype(np.int64)
    f._perm = None
    perm = f.perm
    return [np.sort(perm[(perm >= off[s]) & (perm < off[s + 1])]) - off[s] for s in range(f.n_slots)]


def _twin(make, clouds, rows, moved):
    """A fresh object with, in insertion order, the surviving rows of every pose - moved where the pose is selected."""
    B = make()
    for s, (p, P) in enumerate(clouds):
        X = np.ascontiguousarray(P[rows[s]], dtype=np.float64).reshape(-1, 3)
        B.insert_points(p, transform_np(moved[p], X) if p in moved else X)
    return B


def _same_bits(a, b, what):
    if dataclasses.is_dataclass(a):
        assert type(a) is type(b), what
        for fld in dataclasses.fields(a):
            _same_bits(getattr(a, fld.name), getattr(b, fld.name), f"{what}.{fld.name}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same_bits(x, y, f"{what}[{i}]")
    elif a is None or b is None:
        assert a is None and b is None, what
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.dtype == y.dtype and x.shape == y.shape, (what, x.dtype, y.dtype, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), f"{what}: bits differ"


def _table(leaves):
    sizes = [v.n_points for v in leaves]
    return canon([np.asarray(v.corner_min, dtype=np.float64) for v in leaves], [v.edge_length for v in leaves], sizes,
                 np.arange(int(np.sum(sizes)), dtype=np.int64))


def _leaf_points(leaves):
    return np.concatenate([v.get_points() for v in leaves] + [np.empty((0, 3))])


def _assert_same_grid(A, B, poses, what, leaves=lambda m, p, non_empty: m.get_leaf_points(p, non_empty)):
    for p in poses:
        for count in ("n_points", "n_leaves", "n_nodes"):
            assert getattr(A, count)(p) == getattr(B, count)(p), (what, count, p)
        for non_empty in (True, False):
            la, lb = leaves(A, p, non_empty), leaves(B, p, non_empty)
            assert_same_leaves(_table(la), _table(lb))
            _same_bits(_leaf_points(la), _leaf_points(lb), f"{what}: leaf points of pose {p}")
        _same_bits(A.get_points(p), B.get_points(p), f"{what}: get_points({p})")


def _assert_same_manager(A, B, poses, what):   # (OctreeManager.get_leaf_points takes its arguments the other way round)
    _assert_same_grid(A, B, poses, what, lambda m, p, non_empty: m.get_leaf_points(non_empty, p))


def _assert_same_neighbours(A, B, Q, rows, poses, what):
    """Equal answers, A's indices naming rows of the clouds as first inserted: index_A == rows[pose][index_B]."""
    na, nb = A.nearest(Q, 4, max_distance=0.3), B.nearest(Q, 4, max_distance=0.3)
    _same_bits(na.pose, nb.pose, what + ": pose")
    _same_bits(na.distance2, nb.distance2, what + ": distance2")
    _same_bits(na.count, nb.count, what + ": count")
    want = nb.index.copy()
    for s, p in enumerate(poses):
        m = nb.pose == p
        want[m] = rows[s][nb.index[m]]
    _same_bits(na.index, want, what + ": index")
    assert (na.count > 0).any(), what
    return na


def _split(P, sizes):
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [(p, P[off[p]:off[p + 1]]) for p in range(len(sizes))]


def _fitted_grid(clouds, criteria, table):
    g = _grid()
    for p, P in clouds:
        g.insert_points(p, P)
    g.subdivide(criteria)
    g.map_leaf_points_cuda_ransac(poses_per_batch=2, threshold=0.01, hypotheses=table)
    g.filter([lambda pts: len(pts) >= 10])
    return g


# ---- the twin on a fitted planar scene, both split rules ---------------------------------------------------------------
@pytest.mark.parametrize("criteria", [COUNT, PLANAR], ids=["count", "planar-or-count"])
def test_twin_after_ransac_and_filter(criteria):
    P = synthetic.planar_cloud(14000, (3, 3, 2), seed=11, sigma=0.002)
    clouds = _split(P, [3500, 3501, 3499, 3500])
    poses = [p for p, _ in clouds]
    table = np.random.default_rng(4).random((128, 6))
    A = _fitted_grid(clouds, criteria, table)
    f = A._forest
    rows = _rows(f)
    for s, (p, X) in enumerate(clouds):   # the scene's condition: every pose has dead and alive rows
        assert 0 < len(rows[s]) < len(X), (p, len(rows[s]))
    # answers that are cached on the device and in the host mirror before the write-back
    Q = np.ascontiguousarray(P[::7] + 0.01)
    stale = (A.leaf_planes(), A.nearest(Q, 4, max_distance=0.3), A.plane_segments(max_variance=1e-3))
    moved = {0: _rigid((0, 0, 1), 0.3, (4.0, -3.0, 2.0)), 2: _rigid((1, 1, 0), -0.2, (-5.0, 6.0, 3.0)),
             3: _rigid((1, 0, 0), 0.25, (2.0, 2.0, -4.0))}
    A.transform_poses([moved[p] for p in sorted(moved)], pose_numbers=[3, 0, 2])   # (ascending slot order, as adjust)
    assert not f.has_scheme and f.epoch == 0 and f.info is None and f._dirty
    B = _twin(_grid, clouds, rows, moved)
    _assert_same_grid(A, B, poses, "before any subdivide")
    A.subdivide(criteria)
    B.subdivide(criteria)
    _assert_same_grid(A, B, poses, "after subdivide")
    assert A.n_points(1) == len(rows[1]) and A._forest.nodes["depth"].max() >= 1
    # the map queries answer for the moved map, not from what was cached
    Q2 = np.ascontiguousarray(np.concatenate([B.get_points(p)[::5] for p in poses]) + 0.01)
    planes = A.leaf_planes()
    _same_bits(planes, B.leaf_planes(), "leaf_planes")
    assert len(planes) != len(stale[0]) or planes.mean.tobytes() != stale[0].mean.tobytes()
    _same_bits(A.plane_segments(max_variance=1e-3), B.plane_segments(max_variance=1e-3), "plane_segments")
    _same_bits(A.adjustment_system(max_variance=1e-3), B.adjustment_system(max_variance=1e-3), "adjustment_system")
    _assert_same_neighbours(A, B, Q2, rows, poses, "nearest")
    na, nb = A.nearest(Q, 4, max_distance=0.3), B.nearest(Q, 4, max_distance=0.3)
    _same_bits(na.distance2, nb.distance2, "nearest at the old queries")
    assert na.distance2.tobytes() != stale[1].distance2.tobytes()
    # the RANSAC mask of the same table
    for g in (A, B):
        g._forest.ransac_all(2, table, 0.01)
    ma, mb = A._forest.device_mask(), B._forest.device_mask()
    _same_bits(ma, mb, "RANSAC mask")
    assert 0 < int(ma.sum()) < len(ma)
    # a late pose into both
    late = synthetic.planar_cloud(1500, (3, 3, 2), seed=11, stream=5, sigma=0.002) + [1.0, 0.0, 0.0]
    A.insert_points(7, late)
    B.insert_points(7, late)
    _assert_same_grid(A, B, poses + [7], "after a late pose")


# ---- shapes at which the kernel can go wrong ---------------------------------------------------------------------------
SHAPES = {
    # poses start at store rows 0, 1, 4098, 4100: both parities, a boundary inside one thread's pair and inside a tile
    "pose-boundaries": ([1, 4097, 2, 2049], [0, 1, 3], 0.0),
    "one-less-than-a-workgroup": ([500, ROWS_PER_WG - 501], [0, 1], 0.0),
    "a-workgroup": ([500, ROWS_PER_WG - 500], [1], 0.0),
    "one-more-than-a-workgroup": ([500, ROWS_PER_WG - 499], [0, 1], 0.0),
    "one-point": ([1], [0], 0.0),
    "empty-pose-in-the-middle": ([700, 0, 601], [0, 1, 2], 0.0),
    "utm": ([1500, 1501], [0, 1], 5.0e6),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    sizes, selected, far = SHAPES[name]
    total = int(np.sum(sizes))
    P = synthetic.planar_cloud(total, (2, 2, 2), seed=21, sigma=0.002)
    clouds = _split(P, sizes)
    poses = list(range(len(sizes)))
    A = _grid()
    for p, X in clouds:
        A.insert_points(p, X)
    A.subdivide(COUNT)
    f = A._forest
    if total > 1:   # a mask over the ordered positions: a quarter of the rows die, wherever they are stored
        keep = (np.random.default_rng(2).random(f.n_ord) < 0.75).astype(np.uint8)
        f.apply_host_mask(keep)
        assert 0 < f.n_ord < total
    rows = _rows(f)
    moved = {p: _rigid((1 + p, 2, 3), 0.2 + 0.1 * p, (far + 3.0 + p, -4.0, 5.0 - p)) for p in selected}
    A.transform_poses([moved[p] for p in selected], pose_numbers=selected)
    B = _twin(_grid, clouds, rows, moved)
    _assert_same_grid(A, B, poses, name + ": before any subdivide")
    A.subdivide(COUNT)
    B.subdivide(COUNT)
    _assert_same_grid(A, B, poses, name + ": after subdivide")
    assert sum(A.n_points(p) for p in poses) == sum(len(r) for r in rows)
    Q = np.ascontiguousarray(np.concatenate([B.get_points(p) for p in poses])[::3] + 0.01)
    _assert_same_neighbours(A, B, Q, rows, poses, name)


# ---- directed cases ----------------------------------------------------------------------------------------------------
def test_unselected_rows_keep_their_bits_and_identity_follows_the_formula():
    P = synthetic.planar_cloud(3000, (2, 2, 1), seed=5)
    clouds = _split(P.copy(), [1000, 1001, 999])
    for _, X in clouds:
        X[3] = [-0.0, 0.5, 0.25]      # floor(-0.0) is voxel 0
    A = _grid()
    for p, X in clouds:
        A.insert_points(p, X)
    moved = {0: np.eye(4), 2: _rigid((0, 0, 1), 0.3, (3.0, 1.0, 0.0))}
    A.transform_poses([moved[0], moved[2]], pose_numbers=[0, 2])
    got = {p: A.get_points(p) for p in (0, 1, 2)}
    zero = {p: got[p][(got[p][:, 0] == 0.0) & (got[p][:, 1] == 0.5)] for p in (0, 1)}
    assert len(zero[0]) == 1 and len(zero[1]) == 1
    assert np.signbit(zero[1][0, 0]) and not np.signbit(zero[0][0, 0])    # copied / 1 * -0.0 + 0 * y = +0.0
    assert not np.signbit(transform_np(np.eye(4), clouds[0][1][3:4])[0, 0])
    B = _twin(_grid, clouds, [np.arange(len(X)) for _, X in clouds], moved)
    _assert_same_grid(A, B, [0, 1, 2], "subset")
    # bit for bit the inserted rows, as a multiset of rows
    same = lambda a, b: sorted(r.tobytes() for r in a) == sorted(r.tobytes() for r in np.ascontiguousarray(b))
    assert same(got[1], clouds[1][1]) and same(got[0], transform_np(np.eye(4), clouds[0][1]))


def test_write_back_twice_is_sequential_application():
    P = synthetic.planar_cloud(6000, (2, 2, 2), seed=8, sigma=0.002)
    clouds = _split(P, [2000, 2001, 1999])
    table = np.random.default_rng(1).random((64, 6))
    A = _fitted_grid(clouds, COUNT, table)
    rows = _rows(A._forest)
    T1 = {0: _rigid((0, 1, 0), 0.3, (3.0, 0.0, 1.0)), 1: _rigid((1, 0, 0), 0.2, (0.0, 4.0, 0.0))}
    T2 = {1: _rigid((0, 0, 1), -0.4, (-2.0, 1.0, 3.0)), 2: _rigid((1, 1, 1), 0.1, (5.0, 5.0, 5.0))}
    A.transform_poses([T1[0], T1[1]], pose_numbers=[0, 1])
    A.transform_poses([T2[1], T2[2]], pose_numbers=[1, 2])
    B = _grid()
    for s, (p, X) in enumerate(clouds):
        Y = X[rows[s]]
        for T in (T1, T2):
            if p in T:
                Y = transform_np(T[p], Y)     # (two rounded applications, not one product of matrices)
        B.insert_points(p, Y)
    A.subdivide(COUNT)
    B.subdivide(COUNT)
    _assert_same_grid(A, B, [0, 1, 2], "twice")


def test_before_any_build():
    P = synthetic.planar_cloud(5000, (2, 2, 2), seed=9)
    clouds = _split(P, [2501, 2499])
    A = _grid()
    for p, X in clouds:
        A.insert_points(p, X)
    moved = {1: _rigid((0, 0, 1), 0.5, (6.0, 0.0, -3.0))}
    A.transform_poses([moved[1]], pose_numbers=[1])
    B = _twin(_grid, clouds, [np.arange(len(X)) for _, X in clouds], moved)
    A.subdivide(PLANAR)
    B.subdivide(PLANAR)
    _assert_same_grid(A, B, [0, 1], "before any build")


def _snapshot(f, obj, Q):
    f._invalidate()
    near = obj.nearest(Q, 4, max_distance=0.3)
    return (f.perm.copy(), f.xyz.copy(), f.blocks["node"].copy(), f.blocks["start"].copy(), f.nodes["corner"].copy(),
            near.pose, near.index, near.distance2, near.count)


def test_failure_is_atomic():
    P = synthetic.planar_cloud(6000, (2, 2, 2), seed=12)
    clouds = _split(P, [3000, 3000])
    table = np.random.default_rng(3).random((64, 6))
    A = _fitted_grid(clouds, COUNT, table)
    f = A._forest
    rows = _rows(f)
    Q = np.ascontiguousarray(P[::9] + 0.01)
    before = _snapshot(f, A, Q)
    leaves_before = _leaf_points(A.get_leaf_points(0))
    mirror = (f.epoch, f.has_scheme, f._dirty, list(f.slot_epoch))
    huge = np.eye(4)
    huge[:3, :3] = 1e300               # finite, so as_transforms takes it; the products overflow
    far = np.eye(4)
    far[0, 3] = 2.0 ** 31              # 2^31 voxel edges
    for T in (huge, far):
        with pytest.raises(nat.DomainError, match="unchanged"):
            A.transform_poses([np.eye(4), T])
        assert (f.epoch, f.has_scheme, f._dirty, list(f.slot_epoch)) == mirror and f.info is not None
        _same_bits(_snapshot(f, A, Q), before, "after a refused call")
        _same_bits(_leaf_points(A.get_leaf_points(0)), leaves_before, "leaf points after a refused call")
    with pytest.raises(ValueError):
        A.transform_poses([np.eye(4)])                    # one transform for two poses
    with pytest.raises(ValueError):
        A.transform_poses([np.eye(4), np.full((4, 4), np.nan)])
    with pytest.raises(KeyError):
        A.transform_poses([np.eye(4)], pose_numbers=[5])
    moved = {1: _rigid((0, 0, 1), 0.2, (1.0, 2.0, 3.0))}
    A.transform_poses([moved[1]], pose_numbers=[1])       # a valid call goes through afterwards
    B = _twin(_grid, clouds, rows, moved)
    A.subdivide(COUNT)
    B.subdivide(COUNT)
    _assert_same_grid(A, B, [0, 1], "after the refused calls")

    # one cube: a point pushed out of it
    make = lambda: OctreeManager(Octree, OctreeConfig(), np.array([-4.0, -4.0, -4.0]), 8.0)
    rng = np.random.default_rng(6)
    mc = [(4, rng.uniform(-3.5, 3.5, (1500, 3)) * [1, 1, 0.2]), (9, rng.uniform(-3.5, 3.5, (1501, 3)) * [1, 0.2, 1])]
    for _, X in mc:
        X[:, 0] = np.minimum(X[:, 0], 3.4)
    mc[1][1][77, 0] = 3.45              # the one point a push of 0.56 takes out of the cube [-4, 4)
    M = make()
    for p, X in mc:
        M.insert_points(p, X)
    M.subdivide([MaxPoints(25)])
    M.filter([lambda pts: len(pts) >= 3])
    fm = M._forest
    mrows = _rows(fm)
    assert all(0 < len(r) for r in mrows) and 77 in mrows[1]
    Qm = np.ascontiguousarray(mc[0][1][::5] + 0.01)
    mbefore = _snapshot(fm, M, Qm)
    push = np.eye(4)
    push[0, 3] = 0.56                   # 3.45 + 0.56 >= 4: outside; every other point stays below 3.96
    with pytest.raises(nat.DomainError, match="unchanged"):
        M.transform_poses([np.eye(4), push])
    _same_bits(_snapshot(fm, M, Qm), mbefore, "manager after a refused call")
    ok = {9: _rigid((0, 0, 1), 0.1, (0.25, 0.0, 0.0))}
    M.transform_poses([ok[9]], pose_numbers=[9])
    MB = _twin(make, mc, mrows, ok)
    _assert_same_manager(M, MB, [4, 9], "manager before subdivide")
    M.subdivide([MaxPoints(25)])
    MB.subdivide([MaxPoints(25)])
    _assert_same_manager(M, MB, [4, 9], "manager after subdivide")


def test_borrowed_store_is_never_written():
    P = np.ascontiguousarray(synthetic.planar_cloud(5001, (2, 2, 2), seed=14))
    dc = DeviceCloud(P)
    A = _grid()
    A.insert_points(0, dc)
    f = A._forest
    assert f.reads_in_place(dc)
    A.subdivide(COUNT)
    A.filter([lambda pts: len(pts) >= 30])
    rows = _rows(f)
    assert 0 < len(rows[0]) < len(P) and f.reads_in_place(dc)
    moved = {0: _rigid((0, 1, 1), 0.3, (4.0, 4.0, -2.0))}
    A.transform_poses([moved[0]])
    assert not f.reads_in_place(dc)
    back = np.empty_like(P)
    f.ctx.check(f.lib.octl_dev_download(f.ctx.handle, nat.ptr(back), dc.ptr, back.nbytes))
    _same_bits(back, P, "the caller's buffer")
    B = _twin(_grid, [(0, P)], rows, moved)
    A.subdivide(COUNT)
    B.subdivide(COUNT)
    _assert_same_grid(A, B, [0], "borrowed store")
    _same_bits(np.sort(_rows(f)[0]), rows[0], "store positions")   # perm still names rows of the inserted cloud
    A._forest.close()
    dc.release()


def _deltas(fn):
    a = (_counter("octl_debug_launches"), _counter("octl_debug_host_syncs"))
    fn()
    return _counter("octl_debug_launches") - a[0], _counter("octl_debug_host_syncs") - a[1]


def test_launch_shape_does_not_depend_on_the_size():
    T = _rigid((0, 0, 1), 0.2, (2.0, 0.0, 0.0))
    seen = []
    for n in (100, 20006):
        P = synthetic.planar_cloud(n, (2, 2, 2), seed=15)
        g = _grid()
        g.insert_points(0, P[: n // 3])
        g.insert_points(1, P[n // 3:])
        g.subdivide(COUNT)
        g.filter([lambda pts: len(pts) >= 4])
        assert g.n_points(0) > 0
        g._forest.ctx.sync()
        seen.append(_deltas(lambda: g.transform_poses([T], pose_numbers=[1])))
        seen.append(_deltas(lambda: g.transform_poses([T, T])))     # (a second call: no buffer grows)
    assert seen == [(LAUNCHES_PER_CALL, 1)] * 4, seen


def test_no_ops_change_no_state():
    P = synthetic.planar_cloud(3000, (2, 2, 1), seed=16)
    g = _grid()
    g.insert_points(0, P[:1500])
    g.insert_points(1, P[1500:])
    g.subdivide(COUNT)
    f = g._forest
    perm, epoch = f.perm.copy(), f.epoch
    assert _deltas(lambda: g.transform_poses(np.empty((0, 4, 4)), pose_numbers=[])) == (0, 0)
    assert f.has_scheme and not f._dirty and f.epoch == epoch and f.info is not None
    assert _deltas(f.ensure_built) == (0, 0)          # nothing to rebuild
    f._invalidate()
    _same_bits(f.perm, perm, "perm after S = 0")
    assert f.lib.octl_forest_transform_poses(f.handle, None, 0, None) == nat.OCTL_E_INVALID
    sel = np.ones(3, dtype=np.uint8)
    assert f.lib.octl_forest_transform_poses(f.handle, nat.ptr(sel), 3, nat.ptr(np.zeros(36))) == nat.OCTL_E_INVALID
    # an empty map, built: it stays built
    e = _grid()
    e.insert_points(0, np.empty((0, 3)))
    e.insert_points(1, np.empty((0, 3)))
    assert e.n_points(0) == 0
    fe = e._forest
    assert _deltas(lambda: e.transform_poses([_rigid((0, 0, 1), 0.1, (1, 1, 1))] * 2)) == (0, 0)
    assert not fe._dirty and fe.info is not None and _deltas(fe.ensure_built) == (0, 0)
    # no pose at all
    _grid().transform_poses([])


def test_straight_after_an_asynchronous_apply_mask():
    P = synthetic.planar_cloud(8000, (2, 2, 2), seed=17, sigma=0.002)
    clouds = _split(P, [4001, 3999])
    table = np.random.default_rng(5).random((128, 6))
    moved = {0: _rigid((0, 0, 1), 0.2, (3.0, 3.0, 0.0)), 1: _rigid((0, 1, 0), 0.2, (0.0, -3.0, 3.0))}

    def fitted():
        g = _grid()
        for p, X in clouds:
            g.insert_points(p, X)
        g.subdivide(COUNT)
        g.map_leaf_points_cuda_ransac(poses_per_batch=2, threshold=0.01, hypotheses=table)
        return g

    ref = fitted()
    rows = _rows(ref._forest)         # (waits for the compaction; the same table gives the same mask)
    assert all(0 < len(r) < len(X) for r, (_, X) in zip(rows, clouds))
    A = fitted()
    assert A._forest._n_ord_pending   # the compaction's counts are still on their way
    A.transform_poses([moved[0], moved[1]])
    B = _twin(_grid, clouds, rows, moved)
    _assert_same_grid(A, B, [0, 1], "behind an asynchronous apply_mask")
    A.subdivide(COUNT)
    B.subdivide(COUNT)
    _assert_same_grid(A, B, [0, 1], "behind an asynchronous apply_mask, subdivided")
