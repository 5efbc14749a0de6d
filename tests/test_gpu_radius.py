"""The radius count and radius outlier removal on the device: octl_forest_radius_count / _radius_count_device /
octl_forest_remove_sparse and Grid / OctreeManager / Octree .radius_count / .remove_sparse.

One contract: every count EQUALS the brute force octreelib_amd.query.radius_count_np over the clouds the map reads
back, and after remove_sparse the map EQUALS a second build of the same map that got apply_host_mask with the keep
rule of octreelib_amd.query.sparse_keep_np worked out on the host - counts are integers and d2 <= r2 is decided on the
bits nearest forms, so there is no tolerance to state.  Shapes are small because brute force is the checker."""

import ctypes as C
import functools

import numpy as np
import pytest

from octreelib_amd import DeviceCloud, MaxPoints, nearest_np, radius_count_np, sparse_keep_np, synthetic
from octreelib_amd import _native as nat
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree_manager import OctreeManager
from octreelib_amd.query import sparse_counts_np
from tests.test_cpu_radius import lattice, lattice_expected
from tests.test_gpu_query import BAD, _counter, _DevBuf

pytestmark = pytest.mark.gpu

CAPS = (None, 1, 3, 7)


# ---- helpers -------------------------------------------------------------------------------------------------------
def _device_count(f, Q, r, cap, slots):
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    n = len(Q)
    xin, out = _DevBuf(f.ctx, Q.nbytes), _DevBuf(f.ctx, 4 * n)
    try:
        xin.upload(Q)
        f.radius_count_device(xin.p, n, r, out.p, cap, slots)
        return out.download(n, np.int32)
    finally:
        xin.free()
        out.free()


def _check_count(obj, Q, clouds, r, what, pose_numbers=None, octree=False):
    """Both forms of the device answer, at every cap, against radius_count_np over `clouds` (computed once)."""
    f = obj._forest
    ref = radius_count_np(Q, clouds, r)
    slots = None if octree or pose_numbers is None else [obj._slots[p] for p in pose_numbers]
    for cap in CAPS:
        want = ref if cap is None else np.minimum(ref, cap)
        kw = {} if octree else {"pose_numbers": pose_numbers}
        got = obj.radius_count(Q, r, max_count=cap, **kw)
        assert got.dtype == np.int32 and got.shape == (len(Q),), (what, cap)
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            raise AssertionError(f"{what}, max_count={cap} (host form): {len(bad)} of {len(Q)} counts differ, first "
                                 f"{int(bad[0])}: got {int(got[bad[0]])}, expected {int(want[bad[0]])}")
        assert np.array_equal(_device_count(f, Q, r, cap, slots), want), (what, cap, "device form")
    return ref


def _grid(clouds, K):
    g = Grid(GridConfig(voxel_edge_length=1))
    for p, P in clouds.items():
        g.insert_points(p, P)
    g.subdivide([MaxPoints(K)])
    return g


def _pos_slot(f):
    """The pose slot of every position of the leaf-ordered arrays (the blocks cover them exactly, in storage order)."""
    b = f.blocks
    start, size = b["start"].astype(np.int64), b["size"].astype(np.int64)
    assert np.array_equal(start, np.concatenate([[0], np.cumsum(size)[:-1]])) and size.sum() == f.n_ord
    return np.repeat(b["slot"], size)


def _sparse_counts(f, r, tested=None, among=None):
    """c(x) of sparse_keep_np for every position of the leaf-ordered arrays of `f` (-1: the position is not tested):
    the definition over the clouds the map reads back, slot by slot."""
    xyz, ps = f.xyz, _pos_slot(f)
    slots = list(range(f.n_slots))
    among = slots if among is None else sorted(among)
    tested = slots if tested is None else sorted(tested)
    clouds = [(s, xyz[ps == s]) for s in among]
    cs = sparse_counts_np(clouds, [s if s in among else (s, xyz[ps == s]) for s in tested], r)
    out = np.full(f.n_ord, -1, dtype=np.int64)
    extra = len(clouds)
    for s in tested:
        if s in among:
            out[ps == s] = cs[among.index(s)]
        else:
            out[ps == s] = cs[extra]
            extra += 1
    return out


def _assert_same_map(a, b, what, Q, r):
    """Block table, leaf-ordered points, perm and the answers of leaf_planes and nearest of two maps (b: the checker,
    which apply_host_mask has compacted)."""
    fa, fb = a._forest, b._forest
    assert fa.n_ord == fb.n_ord, what
    for k in ("node", "slot", "start", "size"):
        assert np.array_equal(fa.blocks[k], fb.blocks[k]), (what, k)
    assert fa.xyz.tobytes() == fb.xyz.tobytes() and np.array_equal(fa.perm, fb.perm), what      # (index: not renumbered)
    pa, pb = a.leaf_planes(), b.leaf_planes()
    for name in ("node", "count", "mean", "covariance", "eigenvalues", "eigenvectors"):
        assert getattr(pa, name).tobytes() == getattr(pb, name).tobytes(), (what, name)
    na, nb = a.nearest(Q, 4, max_distance=r), b.nearest(Q, 4, max_distance=r)
    for name in ("pose", "index", "distance2", "count"):
        assert getattr(na, name).tobytes() == getattr(nb, name).tobytes(), (what, name)


def _launches(fn):
    a, b = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
    out = fn()
    return out, (_counter("octl_debug_launches") - a, _counter("octl_debug_host_syncs") - b)


# ---- radius_count ------------------------------------------------------------------------------------------------------
def test_lattice_ties_on_the_radius_and_an_ulp_off():
    P = lattice()
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P[::2])
    g.insert_points(1, P[1::2])
    g.subdivide([MaxPoints(8)])
    assert g._forest.nodes["depth"].max() >= 2
    S = P[::3]
    up, down = np.nextafter(S, np.inf), np.nextafter(S, -np.inf)
    Q = np.concatenate([P, np.column_stack([up[:, 0], S[:, 1], S[:, 2]]), np.column_stack([S[:, 0], down[:, 1], S[:, 2]]),
                        np.column_stack([down[:, 0], up[:, 1], down[:, 2]])])
    ref = _check_count(g, Q, [(0, P[::2]), (1, P[1::2])], 0.125, "lattice")
    assert np.array_equal(ref[:4096], lattice_expected(P))              # 7, 6, 5, 4: d2 == r2 exactly, inclusive
    assert (ref[4096:] < np.tile(lattice_expected(S), 3)).any()          # an ulp off, a neighbour on the radius is lost
    _check_count(g, Q[::5], [(1, P[1::2])], 0.125, "lattice, pose 1", pose_numbers=[1])


def test_geometry_edges():
    rng = np.random.default_rng(5)
    # a cube that is not dyadic: corners of the children are rounded sums
    c0, e0 = 0.1, 3.3
    t = Octree(OctreeConfig(), np.array([c0, c0, c0]), e0)
    P = c0 + rng.random((4000, 3)) * e0 * [1.0, 1.0, 0.3]
    P = P[np.all((P - c0 >= 0) & (P - c0 < e0), axis=1)]
    t.insert_points(P)
    t.subdivide([MaxPoints(20)])
    assert t._forest.nodes["depth"].max() >= 3
    face = rng.random((300, 3)) * e0 + c0
    for a in range(3):      # on the faces and one ulp / a little outside them
        face[100 * a: 100 * a + 25, a] = c0
        face[100 * a + 25: 100 * a + 50, a] = np.nextafter(c0, -1.0)
        face[100 * a + 50: 100 * a + 75, a] = c0 + e0
        face[100 * a + 75: 100 * a + 100, a] = np.nextafter(c0 + e0, np.inf)
    nd = t._forest.nodes
    inner = np.nonzero(nd["first_child"] >= 0)[0]
    planes = nd["corner"][inner] + (nd["edge"][inner] / 2.0)[:, None]      # points on the splitting planes
    Qt = np.concatenate([face, planes[:200], P[:300] + rng.normal(0.0, 0.01, (300, 3)), P[:100], BAD])
    for r in (0.15, 0.6):
        ref = _check_count(t, Qt, [(0, P)], r, f"octree r={r}", octree=True)
        assert (ref > 8).any() and (ref == 0).any() and np.all(ref[-len(BAD):] == 0)
    # UTM magnitudes
    off = np.array([5.0e6, 4.0e5, 100.0])
    U = synthetic.planar_cloud(5000, (2, 2, 2), seed=9) + off
    gu = _grid({0: U}, 48)
    Qu = np.concatenate([U[rng.permutation(5000)[:500]] + rng.normal(0.0, 0.01, (500, 3)), np.floor(U[:100]),
                         np.floor(U[:100]) + [0.0, 0.5, 1.0], BAD])
    ref = _check_count(gu, Qu, [(0, U)], 0.25, "utm")
    assert (ref > 8).mean() > 0.3
    # one voxel of 5000 points, never subdivided: the long leaf loop, counts far above 8
    B = rng.random((5000, 3))
    g0 = Grid(GridConfig(voxel_edge_length=1))
    g0.insert_points(0, B)
    Q0 = np.concatenate([rng.uniform(-0.5, 1.5, (300, 3)), BAD])
    ref = _check_count(g0, Q0, [(0, B)], 0.2, "one large block")
    assert ref.max() > 100 and (ref == 0).any()
    # a manager: one cube, pose numbers that are not slots
    m = OctreeManager(Octree, OctreeConfig(), np.array([-4.0, -4.0, -4.0]), 8.0)
    Pm = {4: rng.uniform(-4.0, 4.0, (3000, 3)) * [1, 1, 0.2], 9: rng.uniform(-4.0, 4.0, (2000, 3)) * [1, 0.2, 1]}
    for p, X in Pm.items():
        m.insert_points(p, X)
    m.subdivide([MaxPoints(25)])
    Qm = np.concatenate([rng.uniform(-5.0, 5.0, (400, 3)) * [1, 1, 0.3], Pm[9][:200], BAD])
    both = _check_count(m, Qm, [(4, Pm[4]), (9, Pm[9])], 0.5, "manager")
    only9 = _check_count(m, Qm, [(9, Pm[9])], 0.5, "manager, pose 9", pose_numbers=[9])
    assert (only9 <= both).all() and (only9 < both).any() and (both > 8).any()
    with pytest.raises(KeyError):
        m.radius_count(Qm, 0.5, pose_numbers=[5])


def test_absent_points_never_count():
    clouds = {p: synthetic.planar_cloud(3000, (2, 2, 2), seed=6, stream=p, sigma=0.002) for p in range(4)}
    g = _grid(clouds, 48)
    f = g._forest
    rng = np.random.default_rng(2)
    allp = np.vstack(list(clouds.values()))
    Q = np.concatenate([allp[rng.permutation(len(allp))[:600]] + rng.normal(0.0, 0.01, (600, 3)), BAD])
    read = lambda: [(p, g.get_points(p)) for p in sorted(g._slots, key=g._slots.get)]
    full = _check_count(g, Q, read(), 0.1, "as inserted")
    np.random.seed(1)
    g.map_leaf_points_cuda_ransac(poses_per_batch=4, threshold=0.01, hypotheses_number=128, initial_points_number=6)
    n1 = f.n_ord
    assert 0 < n1 < 12000
    after = _check_count(g, Q, read(), 0.1, "after RANSAC + apply_mask")
    assert (after <= full).all() and after.sum() < full.sum()
    g.filter([lambda pts: len(pts) >= 6])
    n2 = f.n_ord
    assert 0 < n2 < n1
    _check_count(g, Q, read(), 0.1, "after filter")
    from tests._raycast import box_rays

    O, D = box_rays(rng, [0, 0, 0], [2, 2, 2], 3000, 0.5)
    assert g.carve_rays(O, D, rng.uniform(0.3, 2.5, 3000), 0.05) > 0
    _check_count(g, Q, read(), 0.1, "after carve")
    assert g.remove_poses([1]) > 0
    clouds_left = read()
    assert [p for p, _ in clouds_left] == [0, 2, 3]
    last = _check_count(g, Q, clouds_left, 0.1, "after remove_poses")
    assert 0 < last.sum() < after.sum()
    _check_count(g, Q, clouds_left[1:], 0.1, "after remove_poses, poses 3 and 2", pose_numbers=[3, 2])


def test_refusals_empty_input_launch_shape_and_nothing_else_disturbed():
    P = synthetic.planar_cloud(20000, (3, 3, 2), seed=3)
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P[:12000])
    g.insert_points(1, P[12000:])
    f = g._forest
    lib, h = f.lib, f.handle
    rng = np.random.default_rng(7)
    Q = np.ascontiguousarray(np.concatenate([P[rng.permutation(20000)] + rng.normal(0.0, 0.01, (20000, 3)), BAD]))
    n = len(Q)
    assert n == 20006
    count = np.full(n, -7, dtype=np.int32)

    def abi(m, r, cap, sel=None, n_sel=0, q=Q, out=count):
        return lib.octl_forest_radius_count(h, nat.ptr(q), m, r, cap, nat.ptr(sel), n_sel, nat.ptr(out))

    assert abi(100, 0.1, 0) == nat.OCTL_E_STATE and b"radius_count before build" in lib.octl_last_error(f.ctx.handle)
    assert lib.octl_forest_remove_sparse(h, 0.1, 1, None, 0, None, 0, None) == nat.OCTL_E_STATE
    assert b"remove_sparse before build" in lib.octl_last_error(f.ctx.handle)
    g.subdivide([MaxPoints(64)])
    # refusals, at the ABI and in Python
    for r in (0.0, -0.5, float("nan"), float("inf"), 2.0000001):
        assert abi(100, r, 0) == nat.OCTL_E_INVALID
        with pytest.raises(ValueError):
            g.radius_count(Q[:10], r)
    assert b"voxel edge" in lib.octl_last_error(f.ctx.handle)
    assert abi(100, 2.0, 1, out=np.empty(100, dtype=np.int32)) == 0      # (twice the voxel edge is allowed)
    assert abi(100, 0.1, -1) == nat.OCTL_E_INVALID and b"max_count" in lib.octl_last_error(f.ctx.handle)
    for bad in (0, -1, 2 ** 31, 1.5, True):
        with pytest.raises(ValueError):
            g.radius_count(Q[:10], 0.1, max_count=bad)
    assert abi(-1, 0.1, 0) == nat.OCTL_E_INVALID and abi(2 ** 31, 0.1, 0) == nat.OCTL_E_INVALID
    assert abi(100, 0.1, 0, q=None) == nat.OCTL_E_INVALID and abi(100, 0.1, 0, out=None) == nat.OCTL_E_INVALID
    assert abi(100, 0.1, 0, np.ones(3, dtype=np.uint8), 3) == nat.OCTL_E_INVALID
    assert np.all(count == -7)                         # nothing ran
    with pytest.raises(ValueError):
        g.radius_count(np.zeros((4, 2)), 0.1)
    with pytest.raises(KeyError):
        g.radius_count(Q[:10], 0.1, pose_numbers=[7])
    with pytest.raises(ValueError, match="float64"):
        g.radius_count(DeviceCloud(Q[:10].astype(np.float32)), 0.1)
    # n = 0 and n = 1
    e = g.radius_count(np.empty((0, 3)), 0.1)
    assert e.shape == (0,) and e.dtype == np.int32
    a = _counter("octl_debug_launches")
    assert abi(0, 0.1, 0) == 0 and lib.octl_forest_radius_count_device(h, None, 0, 0.1, 0, None, 0, None) == 0
    assert _counter("octl_debug_launches") == a        # no kernel
    clouds = [(0, P[:12000]), (1, P[12000:])]
    one = g.radius_count(Q[:1], 0.3)
    assert np.array_equal(one, radius_count_np(Q[:1], clouds, 0.3)) and one[0] > 8
    assert np.array_equal(_device_count(f, Q[:1], 0.3, None, None), one)
    # a DeviceCloud is read where it lies
    dc = DeviceCloud(Q[:500])
    assert np.array_equal(g.radius_count(dc, 0.3, max_count=5), np.minimum(radius_count_np(Q[:500], clouds, 0.3), 5))
    # what the calls below must leave alone
    planes = g.leaf_planes()
    f._pooled = None
    planes, cost_planes = _launches(g.leaf_planes)              # (the pooled table is in place: what a repeat costs)
    g.nearest(Q[:2000], 8, max_distance=0.3)                    # (warm: the staging of this size is allocated)
    near, cost_near = _launches(lambda: g.nearest(Q[:2000], 8, max_distance=0.3))
    # launch and host-wait counts with the index in place: constant in n
    xin, c_d = _DevBuf(f.ctx, Q.nbytes), _DevBuf(f.ctx, 4 * n)
    xin.upload(Q)
    calls = {"radius_count": lambda m: abi(m, 0.3, 0),
             "radius_count_device": lambda m: lib.octl_forest_radius_count_device(h, xin.p, m, 0.3, 0, None, 0, c_d.p)}
    expect = {"radius_count": (1, 1), "radius_count_device": (1, 0)}
    try:
        for name, fn in calls.items():
            assert fn(n) == 0          # (warm: staging allocated, voxel codes and the index on the device)
            f.ctx.sync()
            for m in (257, n):
                rc, got = _launches(lambda: fn(m))
                assert rc == 0 and got == expect[name], (name, m, got)
            f.ctx.sync()
        assert np.array_equal(c_d.download(n, np.int32), count)
    finally:
        xin.free()
        c_d.free()
    assert (count > 8).mean() > 0.5 and np.all(count[-len(BAD):] == 0)
    assert np.array_equal(count[:3000], radius_count_np(Q[:3000], clouds, 0.3))
    # another selection makes a new index: more than the one launch
    _, (l, _) = _launches(lambda: g.radius_count(Q[:100], 0.3, pose_numbers=[1]))
    assert l > 1
    g.radius_count(Q[:100], 0.3)                        # (back to the index of every pose, as nearest left it)
    # leaf_planes and nearest afterwards: the same bits for the same launches
    f._pooled = None
    planes2, cost2 = _launches(g.leaf_planes)
    assert planes2 is not planes and cost2 == cost_planes
    for name in ("node", "count", "mean", "covariance", "eigenvalues", "eigenvectors"):
        assert getattr(planes2, name).tobytes() == getattr(planes, name).tobytes(), name
    near2, cost2 = _launches(lambda: g.nearest(Q[:2000], 8, max_distance=0.3))
    assert cost2 == cost_near
    for name in ("pose", "index", "distance2", "count"):
        assert getattr(near2, name).tobytes() == getattr(near, name).tobytes(), name
    # the counts are the candidates of nearest wherever they fit its list
    few, near_few = g.radius_count(Q[:2000], 0.05), g.nearest(Q[:2000], 8, max_distance=0.05)
    small = few <= 8
    assert small.any() and (~small).any() and np.array_equal(np.minimum(few, 8), near_few.count)
    # rows moved outside their leaves: no cube bounds what it holds
    g.map_leaf_points(lambda p: p + np.array([0.0, 0.0, 0.4]), [1])
    with pytest.raises(RuntimeError, match="outside their leaves"):
        g.radius_count(Q[:10], 0.1)
    with pytest.raises(RuntimeError, match="outside their leaves"):
        g.remove_sparse(0.1, 2)
    assert abi(100, 0.1, 0) == nat.OCTL_E_STATE


# ---- remove_sparse -----------------------------------------------------------------------------------------------------
R = 0.125


@functools.lru_cache(maxsize=None)
def _scene():
    """Three poses, about 5 k points: a uniform background whose points have a handful of neighbours, the dyadic
    lattice {0 .. 7}/8 (3 .. 6 others at exactly the radius), blobs of 60 and of 12 points, isolated points in voxels
    of their own, duplicates far from everything, and pairs whose only neighbour lies across a voxel wall."""
    rng = np.random.default_rng(11)
    t = np.arange(8) / 8.0
    lat = np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(-1, 3) + [4.0, 0.0, 0.0]
    back = rng.uniform(0.0, 2.0, (2600, 3))
    big = np.concatenate([c + rng.normal(0.0, 0.01, (60, 3)) for c in rng.uniform(6.2, 7.8, (12, 3))])
    mid = np.concatenate([c + rng.normal(0.0, 0.01, (12, 3)) for c in rng.uniform(8.2, 9.8, (20, 3))])
    lone = rng.permutation(1000)[:60]
    lone = np.column_stack([lone // 100, (lone // 10) % 10, lone % 10]) + [12.0, 0.0, 0.0] + rng.uniform(0.1, 0.9, (60, 3))
    poses = {0: [], 1: [], 2: []}
    for X in (lat, back, big, mid, lone):
        which = rng.integers(0, 3, len(X))
        for p in poses:
            poses[p].append(X[which == p])
    wall = np.array([[3.0 - 2.0 ** -10, 5.5, 5.5], [3.0, 5.5, 5.5]])       # voxels (2, 5, 5) and (3, 5, 5)
    poses[1].append(wall)                                                  # ... both in one pose
    poses[0].append(wall[:1] + [0.0, 2.0, 0.0])                            # ... and in two poses
    poses[2].append(wall[1:] + [0.0, 2.0, 0.0])
    poses[1].append(np.array([[20.5, 12.5, 7.5], [20.5, 12.5, 7.5]]))       # duplicates far from everything
    poses[0].append(np.array([[22.5, 12.5, 7.5]]))                         # the same coordinates in two poses
    poses[2].append(np.array([[22.5, 12.5, 7.5]]))
    clouds = {p: np.ascontiguousarray(np.concatenate(v)) for p, v in poses.items()}
    for c in clouds.values():
        c.setflags(write=False)
    Q = np.concatenate([back[:150] + 0.01, lat[:100], big[:50], lone[:20], wall, BAD])
    return clouds, np.ascontiguousarray(Q)


@functools.lru_cache(maxsize=None)
def _scene_counts(tested=None, among=None):
    """c(x) over the leaf-ordered arrays of a fresh build of the scene: computed once per selection, shared."""
    clouds, _ = _scene()
    c = _sparse_counts(_grid(clouds, 16)._forest, R, tested, among)
    c.setflags(write=False)
    return c


def _rows_of(f, xyz_rows):
    return {r.tobytes() for r in np.ascontiguousarray(xyz_rows)}


@pytest.mark.parametrize("m", [1, 2, 8, 20])
def test_remove_sparse_is_apply_host_mask_of_the_keep_rule(m):
    clouds, Q = _scene()
    c = _scene_counts()
    a, b = _grid(clouds, 16), _grid(clouds, 16)
    fa, fb = a._forest, b._forest
    assert fa.nodes["depth"].max() >= 2 and fa.xyz.tobytes() == fb.xyz.tobytes()
    before = {p: a.get_points(p).copy() for p in clouds}
    n_nodes = len(fa.nodes["depth"])
    keep = c >= m
    assert 0 < keep.sum() < len(keep)
    removed = a.remove_sparse(R, m)
    assert removed == int((~keep).sum()) == sum(len(v) for v in before.values()) - fa.n_ord
    fb.apply_host_mask(keep.astype(np.uint8))
    _assert_same_map(a, b, f"remove_sparse({R}, {m})", Q, 0.3)
    # every pose's get_points: the definition's kept rows in order, bit for bit (the definition over get_points itself)
    names = sorted(clouds)
    kept = sparse_keep_np([(p, before[p]) for p in names], None, R, m)
    for p, k in zip(names, kept):
        assert a.get_points(p).tobytes() == before[p][k].tobytes(), (m, p)
        assert a.n_points(p) == int(k.sum())
    left = [(p, a.get_points(p)) for p in names]
    assert np.array_equal(a.radius_count(Q, R), radius_count_np(Q, left, R))
    ref = nearest_np(Q, left, 4, max_distance=0.3)
    got = a.nearest(Q, 4, max_distance=0.3)
    assert np.array_equal(got.count, ref.count) and np.array_equal(got.distance2, ref.distance2)
    # what the scene was made for
    have = set().union(*[_rows_of(fa, X) for _, X in left])
    row = lambda *x: np.array(x, dtype=np.float64).tobytes()
    wall = (row(3.0 - 2.0 ** -10, 5.5, 5.5), row(3.0, 5.5, 5.5), row(3.0 - 2.0 ** -10, 7.5, 5.5), row(3.0, 7.5, 5.5))
    dup = (row(20.5, 12.5, 7.5), row(22.5, 12.5, 7.5))
    for key in wall + dup:
        assert (key in have) == (m == 1), (m, key)             # one neighbour each: across the wall / the duplicate
    lat_left = sum(int(np.all((X >= [4.0, 0.0, 0.0]) & (X < [5.0, 1.0, 1.0]), axis=1).sum()) for _, X in left)
    assert lat_left == {1: 512, 2: 512, 8: 0, 20: 0}[m]          # 3 .. 6 others at exactly the radius
    lone_left = sum(int((X[:, 0] >= 12.0).sum()) for _, X in left) - (4 if m == 1 else 0)
    assert lone_left == 0                                      # isolated points go at every m
    # the scheme stays; prune afterwards drops what became empty
    assert len(fa.nodes["depth"]) == n_nodes
    res = a.prune()
    assert len(a._forest.nodes["depth"]) < n_nodes and res is not None
    for p, k in zip(names, kept):
        assert a.get_points(p).tobytes() == before[p][k].tobytes(), (m, p, "after prune")


@pytest.mark.parametrize("tested,among", [((2,), None), ((2,), (0, 1)), ((0, 2), (1, 2)), (None, (1,))])
def test_pose_numbers_and_among(tested, among):
    clouds, Q = _scene()
    a, b = _grid(clouds, 16), _grid(clouds, 16)
    fa, fb = a._forest, b._forest
    before = {p: a.get_points(p).copy() for p in clouds}
    c = _scene_counts(tested, among)                 # (pose numbers are slots in this scene)
    m = 3
    keep = (c < 0) | (c >= m)
    judged = sorted(clouds) if tested is None else list(tested)
    removed = a.remove_sparse(R, m, pose_numbers=None if tested is None else list(reversed(tested)),
                              among=None if among is None else list(among))
    assert removed == int((~keep).sum()) > 0
    fb.apply_host_mask(keep.astype(np.uint8))
    _assert_same_map(a, b, f"tested {tested}, among {among}", Q, 0.3)
    for p in clouds:
        if p in judged:
            assert a.n_points(p) < len(before[p]), p
        else:
            assert a.get_points(p).tobytes() == before[p].tobytes(), p      # untested poses keep all their bits
    # the definition over get_points, with a tested pose that is not counted given by its points
    counted = sorted(clouds) if among is None else list(among)
    kept = sparse_keep_np([(p, before[p]) for p in counted],
                          [p if p in counted else (p, before[p]) for p in judged], R, m)
    extra = len(counted)
    for p in judged:
        if p in counted:
            k = kept[counted.index(p)]
        else:
            k, extra = kept[extra], extra + 1
        assert a.get_points(p).tobytes() == before[p][k].tobytes(), p
    with pytest.raises(KeyError):
        a.remove_sparse(R, m, pose_numbers=[4])
    with pytest.raises(KeyError):
        a.remove_sparse(R, m, among=[4])


def test_a_pending_ransac_mask_goes_into_the_same_compaction():
    clouds = {p: synthetic.planar_cloud(2500, (2, 2, 2), seed=6, stream=p, sigma=0.002) for p in (0, 1, 2)}
    Q = np.ascontiguousarray(clouds[0][:300] + 0.01)
    a, b, plain = _grid(clouds, 48), _grid(clouds, 48), _grid(clouds, 48)
    masks = []
    for g in (a, b):
        f = g._forest
        np.random.seed(0)
        f.ransac_blocks(np.ascontiguousarray(f.order), np.random.random((128, 6)), 0.01)
        masks.append(f.device_mask())
    assert np.array_equal(masks[0], masks[1]) and 0 < masks[0].sum() < len(masks[0])
    fa, fb = a._forest, b._forest
    # the definition evaluated BEFORE the call: what the pending mask is about to drop still counts and is judged
    c = _sparse_counts(fb, 0.05, None, None)
    keep = c >= 4
    both = masks[1].astype(bool) & keep
    assert both.sum() < masks[1].sum() and both.sum() < keep.sum()            # each of the two removes something
    assert ((~masks[1].astype(bool)) & keep).any()
    for g in (a, plain):
        g.radius_count(Q[:1], 0.05)                  # (the index of every pose is in place)
    before = fa.n_ord
    removed, cost = _launches(lambda: a.remove_sparse(0.05, 4))
    _, cost_plain = _launches(lambda: plain.remove_sparse(0.05, 4))
    assert cost == cost_plain, (cost, cost_plain)    # one compaction applies both
    fb.apply_host_mask(both.astype(np.uint8))
    assert removed == before - fb.n_ord
    _assert_same_map(a, b, "remove_sparse with a pending RANSAC mask", Q, 0.3)
    assert plain._forest.n_ord == int(keep.sum())


def test_octree_manager_and_octree():
    rng = np.random.default_rng(3)
    blobs = np.concatenate([c + rng.normal(0.0, 0.02, (40, 3)) for c in rng.uniform(-3.0, 3.0, (30, 3)) * [0.5, 1, 1] - [1.6, 0, 0]])
    lone = rng.uniform(-3.9, 3.9, (120, 3))
    # ... and an octant that holds nothing else: 30 points half a metre apart, so that it is split and then empty
    cell = rng.permutation(64)[:30]
    far = np.column_stack([cell // 16, (cell // 4) % 4, cell % 4]) * 0.5 + 2.1 + rng.uniform(-0.05, 0.05, (30, 3))
    X = np.concatenate([blobs, lone, far])[rng.permutation(1350)]
    Q = np.concatenate([X[:200] + 0.01, BAD])
    # a manager: one cube, pose numbers that are not slots
    Pm = {4: X[:700], 9: X[700:]}
    pair = []
    for _ in range(2):
        m = OctreeManager(Octree, OctreeConfig(), np.array([-4.0, -4.0, -4.0]), 8.0)
        for p, Y in Pm.items():
            m.insert_points(p, Y)
        m.subdivide([MaxPoints(25)])
        pair.append(m)
    a, b = pair
    before = {p: a.get_points(p).copy() for p in Pm}
    n_nodes = len(a._forest.nodes["depth"])
    c = _sparse_counts(b._forest, 0.3, [a._slots[9]], None)
    keep = (c < 0) | (c >= 5)
    assert a.remove_sparse(0.3, 5, pose_numbers=[9]) == int((~keep).sum()) > 0
    b._forest.apply_host_mask(keep.astype(np.uint8))
    _assert_same_map(a, b, "manager", Q, 0.5)
    k4, k9 = sparse_keep_np([(4, before[4]), (9, before[9])], [9], 0.3, 5)
    assert k4.all() and a.get_points(4).tobytes() == before[4].tobytes()
    assert a.get_points(9).tobytes() == before[9][k9].tobytes() and 0 < k9.sum() < len(k9)
    left = [(4, a.get_points(4)), (9, a.get_points(9))]
    assert np.array_equal(a.radius_count(Q, 0.3), radius_count_np(Q, left, 0.3))
    assert len(a._forest.nodes["depth"]) == n_nodes
    # an octree: no pose arguments
    pair = []
    for _ in range(2):
        t = Octree(OctreeConfig(), np.array([-4.0, -4.0, -4.0]), 8.0)
        t.insert_points(X)
        t.subdivide([MaxPoints(25)])
        pair.append(t)
    a, b = pair
    before = a.get_points().copy()
    n_nodes = len(a._forest.nodes["depth"])
    c = _sparse_counts(b._forest, 0.3)
    assert a.remove_sparse(0.3, 10) == int((c < 10).sum()) > 0
    b._forest.apply_host_mask((c >= 10).astype(np.uint8))
    _assert_same_map(a, b, "octree", Q, 0.5)
    k, = sparse_keep_np([(0, before)], None, 0.3, 10)
    assert a.get_points().tobytes() == before[k].tobytes() and 0 < k.sum() < len(k)
    assert np.array_equal(a.radius_count(Q, 0.3, max_count=9), radius_count_np(Q, [(0, before[k])], 0.3, max_count=9))
    assert len(a._forest.nodes["depth"]) == n_nodes
    a.prune()
    assert len(a._forest.nodes["depth"]) < n_nodes and a.get_points().tobytes() == before[k].tobytes()


def test_launch_shape_does_not_depend_on_the_size_of_the_map():
    costs = {}
    for n in (2000, 20000):
        P = synthetic.planar_cloud(n, (2, 2, 2), seed=4, sigma=0.002)
        g = _grid({0: P[: n // 2], 1: P[n // 2:]}, 48)
        f = g._forest
        f.apply_host_mask(np.ones(f.n_ord, dtype=np.uint8))      # (warm: the buffers of the compaction exist)
        g.radius_count(P[:1], 0.05)                              # (... and the index of every pose is in place)
        f.ctx.sync()
        removed, costs[n] = _launches(lambda: g.remove_sparse(0.05, 4))
        assert 0 < removed < n
        g.radius_count(P[:1], 0.05, pose_numbers=[0])
        _, costs[n, "sel"] = _launches(lambda: g.remove_sparse(0.05, 4, pose_numbers=[1], among=[0]))
    print("remove_sparse (launches, host waits):", costs)
    assert costs[2000] == costs[20000] and costs[2000, "sel"] == costs[20000, "sel"], costs


def test_every_refusal_leaves_the_map_as_it_was():
    clouds = {p: synthetic.planar_cloud(2000, (2, 2, 2), seed=6, stream=p, sigma=0.002) for p in (0, 1)}
    g = _grid(clouds, 48)
    f = g._forest
    lib, h = f.lib, f.handle
    np.random.seed(0)
    f.ransac_blocks(np.ascontiguousarray(f.order), np.random.random((128, 6)), 0.01)      # a mask is pending
    pts = {p: g.get_points(p).copy() for p in clouds}
    mask = f.device_mask()
    assert 0 < mask.sum() < len(mask)
    n_alive = C.c_int64(-5)
    two, three = np.ones(2, dtype=np.uint8), np.ones(3, dtype=np.uint8)

    def abi(r, m, sel=None, n_sel=0, among=None, n_among=0):
        return lib.octl_forest_remove_sparse(h, r, m, nat.ptr(sel), n_sel, nat.ptr(among), n_among, C.byref(n_alive))

    a = _counter("octl_debug_launches")
    for r in (0.0, -0.5, float("nan"), float("inf"), 2.0000001):
        assert abi(r, 2) == nat.OCTL_E_INVALID, r
    for m in (0, -1, -2 ** 31):
        assert abi(0.1, m) == nat.OCTL_E_INVALID and b"min_neighbours" in lib.octl_last_error(f.ctx.handle)
    assert abi(0.1, 2, three, 3) == nat.OCTL_E_INVALID and abi(0.1, 2, two, 2, three, 3) == nat.OCTL_E_INVALID
    assert abi(0.1, 2, None, 0, three, 3) == nat.OCTL_E_INVALID
    assert _counter("octl_debug_launches") == a and n_alive.value == -5          # nothing ran
    for bad in ((0.0, 2), (float("nan"), 2), (2.5, 2), (0.1, 0), (0.1, -1), (0.1, 1.5), (0.1, True), (0.1, 2 ** 31),
                (0.1, None)):
        with pytest.raises(ValueError):
            g.remove_sparse(*bad)
    with pytest.raises(TypeError):
        g.remove_sparse(0.1)
    with pytest.raises(KeyError):
        g.remove_sparse(0.1, 2, pose_numbers=[3])
    assert np.array_equal(f.device_mask(), mask)
    for p in clouds:
        assert g.get_points(p).tobytes() == pts[p].tobytes()
    # ... and the call that is not refused applies both
    before = f.n_ord
    c = _sparse_counts(f, 0.1)
    removed = g.remove_sparse(0.1, 2)
    assert removed == before - int((mask.astype(bool) & (c >= 2)).sum()) > before - int(mask.sum())
