"""Multi-pose plane adjustment on the device: octl_forest_adjustment_system / octl_forest_adjustment_tables
(csrc/adjust.hip) and their Python surface (Grid / OctreeManager: adjustment_system, adjust).

Contracts (eps = 2^-53):
 * at identity transforms the leaf table is the bits of leaf_planes(pose_numbers);
 * block moments: within the bound of DESIGN.md 4.6 of the np.longdouble sums over the block's points;
 * sums: the used set and the counts are those of adjustment_system_np(np.longdouble) on the downloaded block moments,
   and every one of the 28 entries of a pose is within (D + 32) eps sum |term| of the longdouble sum of the block terms
   formed from those moments and the device's own plane bits - D = tree_depth(blocks of the pose), |term| product by
   product (adjustment_system_np(magnitude=True)), 32 = the roundings of forming a term;
 * the bits of a pose's row are a function of the call and of that pose's and its leaves' blocks alone."""

import ctypes as C

import numpy as np
import pytest

from octreelib_amd import MaxPoints, synthetic
from octreelib_amd import _native as nat
from octreelib_amd.adjustment import adjust_np, adjustment_system_np, block_moments_np, tree_depth
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree_manager import OctreeManager
from octreelib_amd.registration import se3_exp
from tests.test_cpu_adjustment import (ROOM_MAX_VARIANCE, ROOM_ORIGIN, assert_recovers, random_rigid, room_scene,
                                       sums28, voxel_blocks)
from tests.test_gpu_query import _counter

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
LD = np.longdouble
K_TERM = 32
MAX_EDGE = 2.0      # the largest leaf of the scenes with a variance gate


def _grid(clouds, first_pose=0, edge=1):
    g = Grid(GridConfig(voxel_edge_length=edge))
    for p, P in enumerate(clouds):
        g.insert_points(first_pose + p, P)
    return g


def _check_system(s, T, c, what, **gates):
    """s: an AdjustmentSystem with its tables.  Used set and counts exact, sums within the bound; returns the worst
    error / bound ratio."""
    S = len(s.pose_numbers)
    own = adjustment_system_np(s.blocks, T, c, dtype=LD, leaves=True, **gates)
    mv = gates.get("max_variance")
    if mv is not None and len(own.leaves):       # (no leaf near the gate: the used set is not a matter of rounding)
        assert np.all(np.abs(own.leaves.lambda0 - mv) > 1e-9 * MAX_EDGE ** 2), what
    assert np.array_equal(s.leaves.node, own.leaves.node) and np.array_equal(s.leaves.count, own.leaves.count), what
    assert np.array_equal(s.leaves.used, own.leaves.used), what
    assert s.n_leaves == own.n_leaves == (len(s.leaves), int(s.leaves.used.sum())), what
    assert np.array_equal(s.n_points, own.n_points) and np.array_equal(s.n_blocks, own.n_blocks), what
    ref = adjustment_system_np(s.blocks, T, c, dtype=LD, planes=s.leaves)
    mag = adjustment_system_np(s.blocks, T, c, dtype=LD, planes=s.leaves, magnitude=True)
    worst = 0.0
    for k in range(S):
        D = tree_depth(int((s.blocks.pose == k).sum()))
        bound = (D + K_TERM) * LD(EPS) * sums28(mag, k)
        err = np.abs(sums28(s, k).astype(LD) - sums28(ref, k))
        assert np.all(err <= bound), (what, k, np.nonzero(err > bound)[0], float((err / bound).max()))
        if s.n_blocks[k]:
            worst = max(worst, float((err / np.maximum(bound, np.finfo(LD).tiny)).max()))
        else:
            assert not np.any(sums28(s, k)) and s.n_points[k] == 0, what
        assert np.array_equal(s.H[k], s.H[k].T)
    print(f"{what}: S = {S}, blocks {len(s.blocks)}, leaves {s.n_leaves}, worst sum error / bound = {worst:.4f}")
    return worst


@pytest.fixture(scope="module")
def room():
    clouds, truth = room_scene()
    return _grid(clouds), clouds, truth


def _small_transforms(n, seed=7, angle=0.003, shift=0.004):
    rng = np.random.default_rng(seed)
    return np.stack([random_rigid(rng, angle, shift, ROOM_ORIGIN) for _ in range(n)])


# ---- the leaf table and the block moments -------------------------------------------------------------------------------
def test_identity_is_the_pooled_table():
    P = synthetic.planar_cloud(30000, (4, 4, 2), seed=3, sigma=0.001)
    g = _grid([P[:12000], P[12000:20000] + 0.001, P[20000:] - 0.002], first_pose=2)
    g.subdivide([MaxPoints(64)])
    for sel in (None, [2, 4], [3]):
        s = g.adjustment_system(pose_numbers=sel, min_poses=1, leaves=True)
        planes = g.leaf_planes(sel)
        assert len(planes) > 100 and s.n_leaves[0] == len(planes)
        assert np.array_equal(s.leaves.node, planes.node) and np.array_equal(s.leaves.count, planes.count)
        assert s.leaves.mean.tobytes() == np.ascontiguousarray(planes.mean).tobytes()
        assert s.leaves.lambda0.tobytes() == np.ascontiguousarray(planes.eigenvalues[:, 0]).tobytes()
        assert s.leaves.normal.tobytes() == np.ascontiguousarray(planes.normal).tobytes()
        assert np.array_equal(s.leaves.used, planes.count >= 8)


def test_block_moments():
    rng = np.random.default_rng(11)
    sizes = {(0, 0, 0): 5000, (1, 0, 0): 1, (2, 0, 0): 63, (3, 0, 0): 64, (4, 0, 0): 65, (5, 0, 0): 4097}
    cloud = lambda scale: np.concatenate([np.array(v) + rng.random((max(1, int(n * scale)), 3)) * [1, 1, 0.05]
                                          for v, n in sizes.items()])
    clouds = [cloud(1.0), cloud(0.01)]
    g = _grid(clouds, first_pose=5)          # (never subdivided: the voxel of 5000 points is one block of one pose)
    s = g.adjustment_system(leaves=True)
    bm = s.blocks
    assert bm.pose_numbers == [5, 6] and len(bm) == 12 and sorted(bm.count[bm.pose == 0].tolist()) == sorted(sizes.values())
    assert np.all(np.diff(bm.node.astype(np.int64) * 2 + bm.pose) > 0)          # ((node, pose) order)
    seen = 0
    for k, pose in enumerate(bm.pose_numbers):
        for leaf in g.get_leaf_points(pose):
            i = int(np.nonzero((bm.node == leaf.node) & (bm.pose == k))[0][0])
            x = leaf.get_points().astype(LD)
            a = (np.asarray(leaf.corner_min, dtype=np.float64) + np.float64(leaf.edge_length) / 2.0)
            assert np.array_equal(a, bm.anchor[i])
            d = x - a.astype(LD)
            n = len(x)
            R = float(np.abs(d).max())
            gamma = (-(-n // 64) + -(-n // 4096) + 1 + 16) * EPS
            assert bm.count[i] == n
            assert np.all(np.abs(bm.s[i].astype(LD) - d.sum(axis=0)) <= 2 * gamma * R * n)
            M = np.array([(d[:, u] * d[:, v]).sum() for u, v in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])
            assert np.all(np.abs(bm.M[i].astype(LD) - M) <= 4 * gamma * R * R * n)
            seen += 1
    assert seen == len(bm)


# ---- the sums -----------------------------------------------------------------------------------------------------------
def test_system_on_the_room(room):
    g, clouds, _ = room
    worst = 0.0
    for T, what in ((None, "identity"), (_small_transforms(4), "small"),
                    (_small_transforms(4, 8, np.deg2rad(30.0), 0.5), "30 degrees")):
        for gates in (dict(max_variance=ROOM_MAX_VARIANCE), dict(min_points=200, min_poses=4)):
            mv = gates.get("max_variance")
            if what == "30 degrees" and mv is not None:
                gates = dict(max_variance=0.5)       # (poses this far apart pool into thick leaves)
            s = g.adjustment_system(T, origin=ROOM_ORIGIN, leaves=True, **gates)
            assert s.n_leaves[1] > 20 and np.all(s.n_points > 1000)
            worst = max(worst, _check_system(s, T, ROOM_ORIGIN, f"room {what} {gates}", **gates))
    # the default origin: the centre of the box of the top-level voxels
    assert np.array_equal(g.adjustment_system().origin, [3.5, 3.0, 2.0])
    print(f"worst error / bound on the room: {worst:.4f}")


def _counts_scene():
    """Poses whose selected-block counts are the given ones: leaves of 8 points seen by two poses."""
    counts = [4097, 0, 1, 255, 256, 257, 1023, 1024, 1025, 4097]
    rng = np.random.default_rng(13)
    vox = np.array([v for v in np.ndindex(17, 17, 15)][:4097], dtype=np.float64)
    clouds = []
    for n in counts:
        v = np.repeat(vox[:n], 4, axis=0)
        clouds.append(v + np.column_stack([rng.uniform(0.1, 0.9, (len(v), 2)), 0.5 + rng.normal(0, 1e-3, len(v))]))
    # ... and a pose alone in its voxels: no block of it lies in a used leaf
    far = np.repeat(np.array([[30.0, 0.0, 0.0], [31.0, 0.0, 0.0]]), 10, axis=0)
    clouds.append(far + rng.uniform(0.1, 0.9, far.shape) * [1, 1, 0.01])
    return counts + [2], clouds


@pytest.fixture(scope="module")
def counted():
    counts, clouds = _counts_scene()
    return _grid(clouds), counts, clouds


def test_shapes(counted):
    g, counts, clouds = counted
    S = len(counts)
    T = _small_transforms(S, 9, 0.002, 0.003)
    c = np.array([8.0, 8.0, 7.0])
    s = g.adjustment_system(T, origin=c, leaves=True)
    assert [int((s.blocks.pose == k).sum()) for k in range(S)] == counts
    _check_system(s, T, c, "all counts")
    assert s.n_blocks.tolist()[:-1] == counts[:-1] and s.n_points.tolist()[:-1] == [4 * n for n in counts[:-1]]
    assert s.n_blocks[-1] == 0 and s.n_points[-1] == 0 and not s.H[-1].any() and s.cost[-1] == 0    # (alone)
    assert s.n_blocks[1] == 0 and not s.H[1].any()                                                    # (no block at all)
    # S = 1: nothing is used under min_poses = 2; with min_poses = 1 the pose is scored against its own planes
    one = g.adjustment_system(T[9:10], pose_numbers=[9], origin=c, leaves=True)
    assert one.n_leaves == (4097, 0) and not one.H.any() and one.n_points.tolist() == [0]
    _check_system(one, T[9:10], c, "one pose")
    own = g.adjustment_system(T[9:10], pose_numbers=[9], origin=c, min_points=4, min_poses=1, leaves=True)
    assert own.n_leaves == (4097, 4097) and own.n_blocks.tolist() == [4097]
    _check_system(own, T[9:10], c, "one pose, min_poses 1", min_points=4, min_poses=1)
    # a subset, in whatever order it is named
    sub = g.adjustment_system(T[[4, 7, 9]], pose_numbers=[9, 4, 7], origin=c, leaves=True)
    assert sub.pose_numbers == [4, 7, 9]
    _check_system(sub, T[[4, 7, 9]], c, "subset")
    # no selected block at all: nothing runs
    none = g.adjustment_system(pose_numbers=[1], origin=c)
    assert none.n_leaves == (0, 0) and not none.H.any() and none.H.shape == (1, 6, 6)
    a = _counter("octl_debug_launches")
    g.adjustment_system(pose_numbers=[1], origin=c)
    assert _counter("octl_debug_launches") == a
    with pytest.raises(KeyError):
        g.adjustment_system(pose_numbers=[0, 77])


def test_scheme_from_another_subset():
    rng = np.random.default_rng(5)
    clouds = [rng.uniform(-5.0, 5.0, (15000, 3)) * [1, 1, 0.002] + [0, 0, 0.5] for _ in range(3)]
    g = _grid(clouds, first_pose=3, edge=2)
    g.subdivide([MaxPoints(30)], pose_numbers=[3])
    T = np.stack([se3_exp([0.001 * k, -0.002, 0.003, 0.01, 0.0, 0.002 * k], [0.0, 0.0, 0.5]) for k in range(2)])
    s = g.adjustment_system(T, pose_numbers=[4, 5], origin=[0.0, 0.0, 0.5], leaves=True)
    assert s.pose_numbers == [4, 5] and s.n_leaves[1] > 200 and g._forest.nodes["depth"].max() >= 2
    _check_system(s, T, np.array([0.0, 0.0, 0.5]), "subset scheme")
    # a manager: one cube
    m = OctreeManager(Octree, OctreeConfig(), np.array([-6.0, -6.0, -6.0]), 12.0)
    for p, P in zip((4, 9), clouds):
        m.insert_points(p, P)
    m.subdivide([MaxPoints(25)])
    sm = m.adjustment_system(T, leaves=True)
    assert np.array_equal(sm.origin, [0.0, 0.0, 0.0]) and sm.pose_numbers == [4, 9] and sm.n_leaves[1] > 200
    _check_system(sm, T, np.zeros(3), "manager")


def test_reproducible_and_independent_of_other_poses(counted):
    g, counts, clouds = counted
    T = _small_transforms(3, 10, 0.002, 0.003)
    c = np.array([8.0, 8.0, 7.0])
    a = g.adjustment_system(T, pose_numbers=[0, 5, 8], origin=c)
    b = g.adjustment_system(T, pose_numbers=[0, 5, 8], origin=c)
    g.adjustment_system(pose_numbers=[2, 3], origin=c)                     # (another selection in between)
    d = g.adjustment_system(T, pose_numbers=[0, 5, 8], origin=c)
    for k in range(3):
        assert sums28(a, k).tobytes() == sums28(b, k).tobytes() == sums28(d, k).tobytes()
    # an unrelated pose added to the forest, not to the selection
    h = _grid([clouds[0], clouds[5], clouds[8]])
    e = h.adjustment_system(T, origin=c)
    h.insert_points(9, clouds[3] + 0.01)
    f = h.adjustment_system(T, pose_numbers=[0, 1, 2], origin=c)
    for k in range(3):
        assert sums28(e, k).tobytes() == sums28(f, k).tobytes()
    assert np.array_equal(e.n_points, f.n_points)


def test_rigid_motion_of_everything(room):
    g, _, _ = room
    rng = np.random.default_rng(2)
    T = _small_transforms(4)
    a = g.adjustment_system(T, origin=ROOM_ORIGIN, max_variance=ROOM_MAX_VARIANCE)
    for angle in (np.deg2rad(30.0), np.deg2rad(-47.0)):
        G = random_rigid(rng, angle, 2.0, ROOM_ORIGIN)
        b = g.adjustment_system(np.stack([G @ t for t in T]), origin=G[:3, :3] @ ROOM_ORIGIN + G[:3, 3],
                                max_variance=ROOM_MAX_VARIANCE)
        assert a.n_leaves == b.n_leaves and np.array_equal(a.n_points, b.n_points)
        Dm = np.zeros((6, 6))
        Dm[:3, :3] = Dm[3:, 3:] = G[:3, :3]
        for k in range(4):
            # (the cost is what cancellation leaves of sums of size n edge^2: relative to those)
            assert abs(a.cost[k] - b.cost[k]) <= 1e-11 * a.n_points[k]
            Hk = Dm @ a.H[k] @ Dm.T
            assert np.abs(Hk - b.H[k]).max() <= 1e-11 * np.abs(Hk).max()
            assert np.abs(Dm @ a.g[k] - b.g[k]).max() <= 1e-11 * np.abs(Hk).max()


# ---- state ---------------------------------------------------------------------------------------------------------------
def _same_as_fresh(g, poses, what, **gates):
    fresh = _grid([g.get_points(p) for p in poses])
    T = _small_transforms(len(poses), 12)
    a = g.adjustment_system(T, origin=ROOM_ORIGIN, leaves=True, **gates)
    b = fresh.adjustment_system(T, origin=ROOM_ORIGIN, leaves=True, **gates)
    assert a.n_leaves == b.n_leaves and np.array_equal(a.n_points, b.n_points), what
    assert np.array_equal(a.blocks.count, b.blocks.count) and np.array_equal(a.leaves.used, b.leaves.used), what
    for k in range(len(poses)):
        assert np.allclose(sums28(a, k), sums28(b, k), rtol=1e-9, atol=1e-12 * np.abs(b.H[k]).max()), what
    return a


def test_staleness():
    clouds, _ = room_scene(n=3000, seed=6)
    g = _grid(clouds[:3])
    f = g._forest
    gates = dict(max_variance=ROOM_MAX_VARIANCE)
    before = _same_as_fresh(g, [0, 1, 2], "start", **gates)
    # apply_host_mask: every third point leaves
    keep = np.ones(f.n_ord, dtype=np.uint8)
    keep[::3] = 0
    f.apply_host_mask(keep)
    masked = _same_as_fresh(g, [0, 1, 2], "apply_host_mask", **gates)
    assert masked.n_points.sum() < before.n_points.sum()
    # filter_count: the thin leaves of every pose are emptied
    f.filter_count([0, 1, 2], 15, 1 << 30)
    filtered = _same_as_fresh(g, [0, 1, 2], "filter_count", **gates)
    assert len(filtered.blocks) < len(masked.blocks)
    # RANSAC + apply_mask
    np.random.seed(0)
    g.map_leaf_points_cuda_ransac()
    _same_as_fresh(g, [0, 1, 2], "apply_mask", **gates)
    # a late pose
    g.insert_points(3, clouds[3])
    late = _same_as_fresh(g, [0, 1, 2, 3], "late pose", **gates)
    assert late.H.shape == (4, 6, 6) and late.n_points[3] > 100
    # a rebuild
    g.subdivide([MaxPoints(20)])
    rebuilt = g.adjustment_system(origin=ROOM_ORIGIN, leaves=True, **gates)
    assert rebuilt.n_leaves[0] > late.n_leaves[0]
    _check_system(rebuilt, None, ROOM_ORIGIN, "rebuilt", **gates)


def test_state_and_errors():
    clouds, _ = room_scene(n=3000, seed=6)
    g = Grid(GridConfig(voxel_edge_length=1))
    f = g._forest
    lib, h = f.lib, f.handle
    T = np.ascontiguousarray(np.tile(np.eye(4)[:3].reshape(12), (2, 1)))
    c = np.ascontiguousarray(ROOM_ORIGIN)
    sums, counts, nl = np.empty((2, 28)), np.empty((2, 2), dtype=np.int64), np.empty(2, dtype=np.int64)
    n1, n2 = C.c_int64(0), C.c_int64(0)

    def abi(sel=None, n_sel=0, T=T, origin=c, out=sums):
        return lib.octl_forest_adjustment_system(h, nat.ptr(sel), n_sel, nat.ptr(T), nat.ptr(origin), 8, 2, -1.0,
                                                 nat.ptr(out), nat.ptr(counts), nat.ptr(nl))

    def tables():
        return lib.octl_forest_adjustment_tables(h, 0, None, None, None, None, None, None, C.byref(n1), 0, None, None,
                                                 None, C.byref(n2))

    assert abi() == nat.OCTL_E_STATE and b"before build" in lib.octl_last_error(f.ctx.handle)
    assert tables() == nat.OCTL_E_STATE
    for p in range(2):
        g.insert_points(p, clouds[p])
    f.ensure_built()
    assert tables() == nat.OCTL_E_STATE and b"no octl_forest_adjustment_system call" in lib.octl_last_error(f.ctx.handle)
    assert abi() == 0 and nl[0] > 50 and nl[1] > 20 and counts[0, 0] > 1000
    good = sums.copy()
    assert tables() == 0 and n1.value == nl[0] and n2.value > nl[0]
    bad_T = T.copy()
    bad_T[1, 5] = np.nan
    assert abi(T=bad_T) == nat.OCTL_E_INVALID and b"selected pose 1" in lib.octl_last_error(f.ctx.handle)
    assert abi(origin=np.array([0.0, np.inf, 0.0])) == nat.OCTL_E_INVALID
    assert abi(sel=np.ones(3, dtype=np.uint8), n_sel=3) == nat.OCTL_E_INVALID
    assert abi(out=None) == nat.OCTL_E_INVALID
    assert lib.octl_forest_adjustment_system(h, None, 0, None, nat.ptr(c), 8, 2, -1.0, nat.ptr(sums), nat.ptr(counts),
                                             nat.ptr(nl)) == nat.OCTL_E_INVALID
    assert abi() == 0 and sums.tobytes() == good.tobytes()
    for bad in (np.full((2, 4, 4), np.nan), np.stack([np.eye(4)] * 3), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            g.adjustment_system(bad)
    with pytest.raises(ValueError):
        g.adjustment_system(origin=[0.0, np.nan, 1.0])
    # a change of the contents drops the tables of the last call
    g.insert_points(2, clouds[2])
    f.ensure_built()
    assert tables() == nat.OCTL_E_STATE
    assert g.adjustment_system().H.shape == (3, 6, 6) and tables() == 0


def test_allocation_failures_of_a_first_call():
    """The convention of tests/test_gpu_failures.py: every growth of a device buffer that a first adjustment_system
    call makes fails once; the call raises MemoryError with the library's message and, asked again, answers what an
    undisturbed grid answers."""
    clouds, _ = room_scene(n=3000, seed=6)
    T = _small_transforms(4, 12)

    def arm(nth):
        seen = C.c_int64(0)
        nat.get_context().check(nat.load().octl_debug_fail_alloc(int(nth), C.byref(seen)))
        return seen.value

    def fresh():
        g = _grid(clouds)
        g._forest.ensure_built()
        return g

    want = fresh().adjustment_system(T, origin=ROOM_ORIGIN, max_variance=ROOM_MAX_VARIANCE)
    hits, nth = 0, 1
    while True:
        g = fresh()
        arm(nth)
        raised = False
        try:
            g.adjustment_system(T, origin=ROOM_ORIGIN, max_variance=ROOM_MAX_VARIANCE)
        except MemoryError as e:
            raised = True
            assert "injected by octl_debug_fail_alloc" in str(e)
        finally:
            arm(0)
        if not raised:
            break
        hits += 1
        assert g.n_points(0) == len(clouds[0])
        got = g.adjustment_system(T, origin=ROOM_ORIGIN, max_variance=ROOM_MAX_VARIANCE)
        for k in range(4):
            assert sums28(got, k).tobytes() == sums28(want, k).tobytes()
        assert np.array_equal(got.n_points, want.n_points)
        nth += 1
        assert nth < 20
    assert hits >= 3, hits          # (the sort scratch, the tables, the buffer of a call)


def test_launch_shape(room, counted):
    per_size = []
    for g, sel in ((room[0], None), (counted[0], [0, 8, 9])):
        S = 4 if sel is None else 3
        T = _small_transforms(S)
        g.adjustment_system(T, pose_numbers=sel, origin=ROOM_ORIGIN)          # (prepared, buffers grown)
        a, b = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
        g.adjustment_system(T, pose_numbers=sel, origin=ROOM_ORIGIN)
        per_size.append((_counter("octl_debug_launches") - a, _counter("octl_debug_host_syncs") - b))
    assert per_size[0] == per_size[1] == (3, 1), per_size
    # one adjust iteration = the difference between a run of two and a run of one
    g = room[0]
    runs = {}
    for iters in (1, 2):
        a, b = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
        res = g.adjust(origin=ROOM_ORIGIN, max_variance=ROOM_MAX_VARIANCE, max_iterations=iters, tolerance=0.0)
        assert res.iterations == iters and res.reason == "max_iterations"
        runs[iters] = (_counter("octl_debug_launches") - a, _counter("octl_debug_host_syncs") - b)
    assert tuple(x - y for x, y in zip(runs[2], runs[1])) == (3, 1), runs


# ---- adjust --------------------------------------------------------------------------------------------------------------
def test_adjust_recovers_the_poses_on_the_device(room):
    g, clouds, truth = room
    res = g.adjust(origin=ROOM_ORIGIN, max_variance=ROOM_MAX_VARIANCE)
    assert_recovers(res, truth)
    assert res.pose_numbers == [0, 1, 2, 3] and np.array_equal(res.transforms[0], np.eye(4))
    bm = block_moments_np(voxel_blocks(clouds), [0, 1, 2, 3], ROOM_ORIGIN)
    host = adjust_np(lambda T: adjustment_system_np(bm, T, max_variance=ROOM_MAX_VARIANCE), 4)
    diff = float(np.abs(res.transforms - host.transforms).max())
    print(f"device against adjust_np: {res.iterations} / {host.iterations} iterations, largest difference {diff:.3g}")
    assert diff <= 1e-6
    # held poses stay, the others still move
    held = g.adjust(origin=ROOM_ORIGIN, max_variance=ROOM_MAX_VARIANCE, fixed=[0, 2], max_iterations=5)
    assert np.array_equal(held.transforms[2], np.eye(4)) and not np.array_equal(held.transforms[1], np.eye(4))
    # the same through a manager: one cube, subdivided
    m = OctreeManager(Octree, OctreeConfig(), np.zeros(3), 8.0)
    for p, P in enumerate(clouds):
        m.insert_points(p, P)
    m.subdivide([MaxPoints(1000)])
    assert_recovers(m.adjust(origin=ROOM_ORIGIN, max_variance=ROOM_MAX_VARIANCE), truth)


def test_plugged_grid_equals_the_host_map():
    from octreelib_amd.octree.octree_base import OctreeConfigBase
    from tests.test_cpu_query import HostManager, HostOctree

    clouds, truth = room_scene(n=3000, seed=4)
    g = Grid(GridConfig(octree_manager_type=HostManager, octree_type=HostOctree, octree_config=OctreeConfigBase(),
                        voxel_edge_length=1))
    for p, P in enumerate(clouds):
        g.insert_points(p, P)
    assert g._plug is not None
    s = g.adjustment_system(origin=ROOM_ORIGIN, max_variance=ROOM_MAX_VARIANCE)
    hm = g._host_map().adjustment_system(origin=ROOM_ORIGIN, max_variance=ROOM_MAX_VARIANCE)
    for k in range(4):
        assert sums28(s, k).tobytes() == sums28(hm, k).tobytes()
    dev = _grid(clouds).adjustment_system(origin=ROOM_ORIGIN, max_variance=ROOM_MAX_VARIANCE)
    assert np.array_equal(dev.n_points, s.n_points) and dev.n_leaves == s.n_leaves
    for k in range(4):
        assert np.allclose(sums28(dev, k), sums28(s, k), rtol=1e-9, atol=1e-12 * np.abs(s.H[k]).max())
    res = g.adjust(origin=ROOM_ORIGIN, max_variance=ROOM_MAX_VARIANCE)
    assert_recovers(res, truth)
    assert np.array_equal(res.transforms, g._host_map().adjust(origin=ROOM_ORIGIN,
                                                                 max_variance=ROOM_MAX_VARIANCE).transforms)
