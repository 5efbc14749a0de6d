"""The neighbour query on the device: octl_forest_nearest / _nearest_device and Grid / OctreeManager / Octree .nearest.

One contract: all four fields of the answer (pose, index, distance2, count) EQUAL those of the brute force
octreelib_amd.query.nearest_np, bit for bit, in the host form and in the device form - the order (d2, slot, index) is
total, so there is no tolerance to state.  Shapes are small because brute force is the checker."""

import ctypes as C
import functools

import numpy as np
import pytest

from octreelib_amd import MaxPoints, Neighbours, NotPlanar, nearest_np, synthetic
from octreelib_amd import _native as nat
from octreelib_amd._engine import Forest
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree_manager import OctreeManager
from tests.test_cpu_nearest import assert_lattice_situations, lattice_case
from tests.test_gpu_query import BAD, _counter, _DevBuf

pytestmark = pytest.mark.gpu

FIELDS = ("pose", "index", "distance2", "count")


# ---- helpers -------------------------------------------------------------------------------------------------------
def _device_form(f: Forest, Q, k, r, slots, names):
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    n = len(Q)
    xin, s_d, i_d, d_d, c_d = (_DevBuf(f.ctx, Q.nbytes), _DevBuf(f.ctx, 4 * n * k), _DevBuf(f.ctx, 8 * n * k),
                               _DevBuf(f.ctx, 8 * n * k), _DevBuf(f.ctx, 4 * n))
    try:
        xin.upload(Q)
        f.nearest_device(xin.p, n, k, r, s_d.p, i_d.p, d_d.p, c_d.p, slots)
        slot = s_d.download((n, k), np.int32)
        pose = np.asarray(list(names) + [-1], dtype=np.int32)[slot]
        return Neighbours(pose, i_d.download((n, k), np.int64), d_d.download((n, k), np.float64),
                          c_d.download(n, np.int32))
    finally:
        for b in (xin, s_d, i_d, d_d, c_d):
            b.free()


def _assert_equal(got: Neighbours, ref: Neighbours, what):
    for name in FIELDS:
        a, b = getattr(got, name), getattr(ref, name)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, a.shape)
        if not np.array_equal(a, b):
            bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
            i = int(bad[0])
            raise AssertionError(f"{what}: {name} differs in {len(bad)} of {len(a)} rows, first {i}: got "
                                 f"{[getattr(got, f)[i].tolist() for f in FIELDS]}, expected "
                                 f"{[getattr(ref, f)[i].tolist() for f in FIELDS]}")


def _check(obj, Q, clouds, k, r, what, pose_numbers=None, ref=None, octree=False):
    """Both forms of the device answer against nearest_np over `clouds` = [(pose number, cloud)] in slot order."""
    f = obj._forest
    if ref is None:
        ref = nearest_np(Q, clouds, k, max_distance=r)
    got = obj.nearest(Q, k, max_distance=r) if octree else obj.nearest(Q, k, max_distance=r, pose_numbers=pose_numbers)
    assert isinstance(got, Neighbours)
    _assert_equal(got, ref, what + " (host form)")
    if octree:
        slots, names = None, [0] * f.n_slots
    else:
        by_slot = sorted(obj._slots.items(), key=lambda kv: kv[1])
        names = [p for p, _ in by_slot]
        slots = None if pose_numbers is None else [obj._slots[p] for p in pose_numbers]
    _assert_equal(_device_form(f, Q, k, r, slots, names), ref, what + " (device form)")
    return got


def _queries(P, n, seed=0):
    """A second scan of the map: its points jittered by 1 cm, the first tenth pushed out by up to 3 m, the BAD rows."""
    rng = np.random.default_rng(seed)
    m = n - len(BAD)
    Q = P[rng.permutation(len(P))[:m]] + rng.normal(0.0, 0.01, (m, 3))
    Q[: m // 10] += rng.uniform(-3.0, 3.0, (m // 10, 3))
    return np.concatenate([Q, BAD])


def _survivors(f: Forest, slot):
    """Rows of the inserted cloud of `slot` that the ordered arrays still hold, ascending."""
    off = np.concatenate([[0], np.cumsum(f.slot_sizes)])
    f._perm = None
    perm = f.perm
    mine = perm[(perm >= off[slot]) & (perm < off[slot + 1])] - off[slot]
    return np.sort(mine)


def _ref_over_survivors(f, Q, clouds, k, r):
    """nearest_np over the points that are left, its indices mapped back to rows of the inserted clouds (the map is
    ascending, so the order (d2, slot, index) is the same in both numberings)."""
    keep = [_survivors(f, s) for s in range(len(clouds))]
    ref = nearest_np(Q, [(p, P[keep[s]]) for s, (p, P) in enumerate(clouds)], k, max_distance=r)
    names = [p for p, _ in clouds]
    for s, p in enumerate(names):
        m = ref.pose == p
        ref.index[m] = keep[s][ref.index[m]]
    return ref, keep


# ---- test 1: a planar scene, both split rules ------------------------------------------------------------------------
SETTINGS = [(1, 0.05), (3, 0.3), (8, 0.3), (8, 2.0)]


@functools.lru_cache(maxsize=None)
def _planar_case():
    P = synthetic.planar_cloud(8000, (2, 2, 2), seed=3, sigma=0.001)
    Q = _queries(P, 2000)
    clouds = [(0, P[:5000]), (1, P[5000:])]
    refs = {kr: nearest_np(Q, clouds, kr[0], max_distance=kr[1]) for kr in SETTINGS}
    for a in refs.values():
        for name in FIELDS:
            getattr(a, name).setflags(write=False)
    return clouds, Q, refs


@pytest.mark.parametrize("rule", ["count", "planar"])
def test_planar_scene(rule):
    clouds, Q, refs = _planar_case()
    g = Grid(GridConfig(voxel_edge_length=1))
    for p, P in clouds:
        g.insert_points(p, P)
    g.subdivide([MaxPoints(64)] if rule == "count" else [NotPlanar(1e-4, min_points=16)])
    assert g._forest.nodes["depth"].max() >= 2
    for (k, r), ref in refs.items():
        got = _check(g, Q, clouds, k, r, f"{rule} k={k} r={r}", ref=ref)
        none, full = float((got.count == 0).mean()), float((got.count == k).mean())
        print(f"{rule} k={k} r={r}: {none:.3f} of the queries find nothing, {full:.3f} fill all k")
        assert none > 0 and full > 0
        assert np.all(got.count[-len(BAD):] == 0)
    # float32 queries are widened on the host, exactly
    Q32 = Q[:500].astype(np.float32)
    _assert_equal(g.nearest(Q32, 3, max_distance=0.3), nearest_np(Q32.astype(np.float64), clouds, 3, max_distance=0.3),
                  "float32 queries")


# ---- test 2: ties and the inclusive radius ---------------------------------------------------------------------------
def test_lattice_ties_and_inclusive_radius():
    P0, P1, Q, k, r = lattice_case()
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P0)
    g.insert_points(1, P1)
    g.subdivide([MaxPoints(8)])
    assert g._forest.nodes["depth"].max() >= 2
    got = _check(g, Q, [(0, P0), (1, P1)], k, r, "lattice")
    assert_lattice_situations(got, k, r)


# ---- test 3: pose selection, a stale index ----------------------------------------------------------------------------
def test_pose_selection_and_stale_index():
    clouds = [(p, synthetic.planar_cloud(3000, (2, 2, 2), seed=4, stream=p, sigma=0.002)) for p in range(3)]
    g = Grid(GridConfig(voxel_edge_length=1))
    for p, P in clouds:
        g.insert_points(p, P)
    g.subdivide([MaxPoints(48)])
    Q = _queries(np.vstack([P for _, P in clouds]), 1000, seed=1)
    one = _check(g, Q, clouds[1:2], 4, 0.2, "pose 1", pose_numbers=[1])
    assert np.all(one.pose[one.pose >= 0] == 1)
    two = _check(g, Q, clouds[:2], 4, 0.2, "poses 0, 1", pose_numbers=[0, 1])     # (another selection: a new index)
    assert {0, 1} <= set(np.unique(two.pose).tolist()) and 2 not in two.pose
    _check(g, Q, clouds[1:2], 4, 0.2, "pose 1 again", pose_numbers=[1])
    _check(g, Q, clouds, 4, 0.2, "all poses")
    with pytest.raises(KeyError):
        g.nearest(Q, 1, max_distance=0.2, pose_numbers=[7])
    # a late pose: the index is stale and the next call makes it again
    late = (3, synthetic.planar_cloud(2000, (3, 2, 2), seed=4, stream=3, sigma=0.002))    # (it brings new voxels)
    g.insert_points(*late)
    allp = _check(g, Q, clouds + [late], 4, 0.2, "after a late pose")
    assert 3 in allp.pose
    _check(g, Q, [clouds[0], late], 4, 0.2, "poses 0, 3", pose_numbers=[3, 0])


# ---- test 4: after RANSAC + apply_mask, and after filter ----------------------------------------------------------------
def test_after_ransac_mask_and_filter():
    clouds = [(p, synthetic.planar_cloud(6000, (2, 2, 2), seed=6, stream=p, sigma=0.002)) for p in range(2)]
    g = Grid(GridConfig(voxel_edge_length=1))
    for p, P in clouds:
        g.insert_points(p, P)
    g.subdivide([MaxPoints(64)])
    f = g._forest
    Q = _queries(np.vstack([P for _, P in clouds]), 1000, seed=2)
    before = g.nearest(Q, 8, max_distance=0.3)
    np.random.seed(1)
    g.map_leaf_points_cuda_ransac(poses_per_batch=2, threshold=0.01, hypotheses_number=128, initial_points_number=6)
    n_left = f.n_ord
    assert 0 < n_left < 12000

    def check(what):
        ref, keep = _ref_over_survivors(f, Q, clouds, 8, 0.3)
        got = _check(g, Q, clouds, 8, 0.3, what, ref=ref)
        for s in range(2):         # no removed point is returned; the indices still name rows of the inserted clouds
            alive = np.zeros(len(clouds[s][1]), dtype=bool)
            alive[keep[s]] = True
            idx = got.index[got.pose == s]
            assert len(idx) and alive[idx].all(), what
        return got

    after = check("after RANSAC")
    assert not np.array_equal(after.index, before.index)
    g.filter([lambda pts: len(pts) >= 12])
    assert 0 < f.n_ord < n_left
    check("after filter")


# ---- test 5: geometry edges ---------------------------------------------------------------------------------------------
def test_geometry_edges():
    rng = np.random.default_rng(5)
    # a cube that is not dyadic: corners of the children are rounded sums
    c0, e0 = 0.1, 3.3
    t = Octree(OctreeConfig(), np.array([c0, c0, c0]), e0)
    P = c0 + rng.random((6000, 3)) * e0 * [1.0, 1.0, 0.3]
    P = P[np.all((P - c0 >= 0) & (P - c0 < e0), axis=1)]
    t.insert_points(P)
    t.subdivide([MaxPoints(20)])
    assert t._forest.nodes["depth"].max() >= 3
    face = rng.random((600, 3)) * e0 + c0
    for a in range(3):      # on the faces and one ulp / a little outside them
        face[100 * a: 100 * a + 25, a] = c0
        face[100 * a + 25: 100 * a + 50, a] = np.nextafter(c0, -1.0)
        face[100 * a + 50: 100 * a + 75, a] = c0 + e0
        face[100 * a + 75: 100 * a + 100, a] = c0 + e0 + 0.05
    nd = t._forest.nodes
    inner = np.nonzero(nd["first_child"] >= 0)[0]
    planes = nd["corner"][inner] + (nd["edge"][inner] / 2.0)[:, None]      # points on the splitting planes
    Qt = np.concatenate([face, planes[:300], P[:500] + rng.normal(0.0, 0.01, (500, 3)), P[:200], BAD])
    for k, r in ((8, 0.15), (2, 0.05), (8, 6.0)):
        got = _check(t, Qt, [(0, P)], k, r, f"octree k={k} r={r}", octree=True)
        assert np.all(got.pose[got.pose >= 0] == 0) and (got.count == k).any()
    # UTM magnitudes
    off = np.array([5.0e6, 4.0e5, 100.0])
    U = synthetic.planar_cloud(6000, (2, 2, 2), seed=9) + off
    gu = Grid(GridConfig(voxel_edge_length=1))
    gu.insert_points(0, U)
    gu.subdivide([MaxPoints(48)])
    Qu = np.concatenate([_queries(U, 800, seed=3), np.floor(U[:200]), np.floor(U[:100]) + [0.0, 0.5, 1.0]])
    got = _check(gu, Qu, [(0, U)], 8, 0.25, "utm")
    assert (got.count == 8).mean() > 0.5
    # one voxel of 5000 points, never subdivided: one block larger than any K, found through its root
    B = rng.random((5000, 3))
    g0 = Grid(GridConfig(voxel_edge_length=1))
    g0.insert_points(0, B)
    Q0 = np.concatenate([rng.uniform(-0.5, 1.5, (400, 3)), BAD])
    got = _check(g0, Q0, [(0, B)], 8, 0.1, "one large block")
    assert (got.count == 8).any() and (got.count == 0).any()
    _check(g0, Q0, [(0, B)], 5, 2.0, "one large block, the largest radius")
    # a manager: one cube, pose numbers that are not slots
    m = OctreeManager(Octree, OctreeConfig(), np.array([-4.0, -4.0, -4.0]), 8.0)
    Pm = {4: rng.uniform(-4.0, 4.0, (3000, 3)) * [1, 1, 0.2], 9: rng.uniform(-4.0, 4.0, (2000, 3)) * [1, 0.2, 1]}
    for p, X in Pm.items():
        m.insert_points(p, X)
    m.subdivide([MaxPoints(25)])
    Qm = np.concatenate([rng.uniform(-5.0, 5.0, (600, 3)) * [1, 1, 0.3], Pm[9][:200], BAD])
    got = _check(m, Qm, [(4, Pm[4]), (9, Pm[9])], 8, 0.5, "manager")
    assert {4, 9} <= set(np.unique(got.pose).tolist())
    only9 = _check(m, Qm, [(9, Pm[9])], 1, 0.5, "manager, pose 9", pose_numbers=[9])
    assert np.all(only9.pose[only9.pose >= 0] == 9)


# ---- test 6: refusals, n = 0, launch shape, nothing else disturbed ---------------------------------------------------------
def test_refusals_empty_input_launch_shape_and_untouched_planes():
    P = synthetic.planar_cloud(20000, (3, 3, 2), seed=3)
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P[:12000])
    g.insert_points(1, P[12000:])
    f = g._forest
    lib, h = f.lib, f.handle
    rng = np.random.default_rng(7)
    Q = np.ascontiguousarray(np.concatenate([P[rng.permutation(20000)] + rng.normal(0.0, 0.01, (20000, 3)), BAD]))
    n = len(Q)
    K = 8
    slot, index = np.empty((n, K), dtype=np.int32), np.empty((n, K), dtype=np.int64)
    d2, count = np.empty((n, K)), np.empty(n, dtype=np.int32)

    def abi(m, k, r):
        return lib.octl_forest_nearest(h, nat.ptr(Q), m, k, r, None, 0, nat.ptr(slot), nat.ptr(index), nat.ptr(d2),
                                       nat.ptr(count))

    assert abi(100, 1, 0.1) == nat.OCTL_E_STATE and b"before build" in lib.octl_last_error(f.ctx.handle)
    g.subdivide([MaxPoints(64)])
    planes = g.leaf_planes()
    adj = g.adjustment_system()
    # refusals, at the ABI and in Python
    for k in (0, -3, 9):
        assert abi(100, k, 0.1) == nat.OCTL_E_INVALID
        with pytest.raises(ValueError):
            g.nearest(Q[:10], k, max_distance=0.1)
    for r in (0.0, -0.5, float("nan"), float("inf"), 2.0000001):
        assert abi(100, 1, r) == nat.OCTL_E_INVALID
        with pytest.raises(ValueError):
            g.nearest(Q[:10], 1, max_distance=r)
    assert b"voxel edge" in lib.octl_last_error(f.ctx.handle)
    assert abi(100, 1, 2.0) == 0                     # (twice the voxel edge is allowed)
    assert abi(-1, 1, 0.1) == nat.OCTL_E_INVALID
    with pytest.raises(TypeError):
        g.nearest(Q[:10], 1)
    with pytest.raises(ValueError):
        g.nearest(np.zeros((4, 2)), 1, max_distance=0.1)
    # n = 0
    e = g.nearest(np.empty((0, 3)), 3, max_distance=0.1)
    assert e.pose.shape == e.index.shape == e.distance2.shape == (0, 3) and e.count.shape == (0,)
    assert e.pose.dtype == np.int32 and e.index.dtype == np.int64 and e.count.dtype == np.int32
    assert abi(0, 1, 0.1) == 0
    # launch and host-wait counts with the index in place: constant in n
    xin, s_d, i_d, d_d, c_d = (_DevBuf(f.ctx, Q.nbytes), _DevBuf(f.ctx, 4 * n * K), _DevBuf(f.ctx, 8 * n * K),
                               _DevBuf(f.ctx, 8 * n * K), _DevBuf(f.ctx, 4 * n))
    xin.upload(Q)
    calls = {"nearest": lambda m: abi(m, K, 0.3),
             "nearest_device": lambda m: lib.octl_forest_nearest_device(h, xin.p, m, K, 0.3, None, 0, s_d.p, i_d.p,
                                                                        d_d.p, c_d.p)}
    expect = {"nearest": (1, 1), "nearest_device": (1, 0)}
    try:
        for name, fn in calls.items():
            assert fn(n) == 0          # (warm: staging allocated, voxel codes and the index on the device)
            f.ctx.sync()
            for m in (100, n):
                a, b = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
                assert fn(m) == 0
                got = (_counter("octl_debug_launches") - a, _counter("octl_debug_host_syncs") - b)
                assert got == expect[name], (name, m, got)
            f.ctx.sync()
        assert np.array_equal(s_d.download((n, K), np.int32), slot) and np.array_equal(c_d.download(n, np.int32), count)
        assert np.array_equal(i_d.download((n, K), np.int64), index) and np.array_equal(d_d.download((n, K), np.float64), d2)
    finally:
        for b in (xin, s_d, i_d, d_d, c_d):
            b.free()
    assert (count == K).mean() > 0.5 and np.all(count[-len(BAD):] == 0)
    # another selection makes a new index: more than the one launch
    a = _counter("octl_debug_launches")
    g.nearest(Q[:100], 1, max_distance=0.3, pose_numbers=[1])
    assert _counter("octl_debug_launches") - a > 1
    # the grouping nearest shares with leaf_planes and the adjustment disturbed neither
    f._pooled = None
    planes2 = g.leaf_planes()
    assert planes2 is not planes
    for name in ("node", "count", "mean", "covariance", "eigenvalues", "eigenvectors"):
        assert getattr(planes2, name).tobytes() == getattr(planes, name).tobytes(), name
    adj2 = g.adjustment_system()
    for name in ("H", "g", "cost", "n_points", "n_blocks"):
        assert getattr(adj2, name).tobytes() == getattr(adj, name).tobytes(), name
    assert adj2.n_leaves == adj.n_leaves
    # rows moved outside their leaves: no cube bounds what it holds
    g.map_leaf_points(lambda p: p + np.array([0.0, 0.0, 0.4]), [1])
    with pytest.raises(RuntimeError, match="outside their leaves"):
        g.nearest(Q[:10], 1, max_distance=0.1)
    assert abi(100, 1, 0.1) == nat.OCTL_E_STATE
