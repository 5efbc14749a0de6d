"""The cell count and voxel-grid thinning on the device: octl_forest_cell_count / _cell_count_device /
octl_forest_thin and the module-level cell_count / thin over Grid, OctreeManager and Octree.

One contract: every count EQUALS octreelib_amd.thinning.cell_count_np over the clouds the map reads back, and after
thin the map EQUALS a second build of the same map that got apply_host_mask with the keep rule of
octreelib_amd.thinning.thin_keep_np worked out on the host - counts are integers and cell membership is decided on the
exact sign of a remainder, so there is no tolerance to state.  Shapes are the smallest that reach the cases: cell walls
that rounding moved, cells larger than a voxel's leaves and smaller than the deepest one, cells across voxel walls."""

import ctypes as C
import functools

import numpy as np
import pytest

from octreelib_amd import DeviceCloud, MaxPoints, cell_count, cell_count_np, synthetic, thin, thin_keep_np
from octreelib_amd import _native as nat
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree_manager import OctreeManager
from tests._cell import CAPS, CELL, lattice01, ulp_neighbours
from tests.test_gpu_query import BAD, _counter, _DevBuf
from tests.test_gpu_radius import _assert_same_map, _grid, _launches, _pos_slot

pytestmark = pytest.mark.gpu


# ---- helpers -------------------------------------------------------------------------------------------------------
def _device_count(f, Q, cell, cap, slots):
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    n = len(Q)
    xin, out = _DevBuf(f.ctx, Q.nbytes), _DevBuf(f.ctx, 4 * n)
    try:
        xin.upload(Q)
        f.cell_count_device(xin.p, n, cell, out.p, cap, slots)
        return out.download(n, np.int32)
    finally:
        xin.free()
        out.free()


def _check_count(obj, Q, clouds, cell, what, pose_numbers=None, octree=False, caps=CAPS):
    """Both forms of the device answer, at every cap, against cell_count_np over `clouds` (computed once)."""
    f = obj._forest
    ref = cell_count_np(Q, clouds, cell)
    slots = None if octree or pose_numbers is None else [obj._slots[p] for p in pose_numbers]
    for cap in caps:
        want = ref if cap is None else np.minimum(ref, cap)
        kw = {} if octree else {"pose_numbers": pose_numbers}
        got = cell_count(obj, Q, cell, max_count=cap, **kw)
        assert got.dtype == np.int32 and got.shape == (len(Q),), (what, cap)
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            raise AssertionError(f"{what}, cell={cell}, max_count={cap} (host form): {len(bad)} of {len(Q)} counts "
                                 f"differ, first {int(bad[0])} at {Q[bad[0]].tolist()}: got {int(got[bad[0]])}, "
                                 f"expected {int(want[bad[0]])}")
        assert np.array_equal(_device_count(f, Q, cell, cap, slots), want), (what, cell, cap, "device form")
    return ref


def _thin_keep(f, cell, m, tested=None, among=None):
    """keep of thin_keep_np for every position of the leaf-ordered arrays of `f` (True where the position is not
    tested): the definition over the clouds the map reads back - every slot's rows in insertion order (perm)."""
    xyz, ps, perm = f.xyz, _pos_slot(f), f.perm
    slots = list(range(f.n_slots))
    among = slots if among is None else sorted(among)
    tested = slots if tested is None else sorted(tested)

    def rows(s):
        pos = np.nonzero(ps == s)[0]
        return pos[np.argsort(perm[pos], kind="stable")]

    counted = [(s, xyz[rows(s)]) for s in among]
    tt = [s if s in among else (s, xyz[rows(s)], sum(1 for a in among if a < s)) for s in tested]
    keep = thin_keep_np(counted, tt, cell, m)
    out = np.ones(f.n_ord, dtype=bool)
    extra = len(counted)
    for s in tested:
        if s in among:
            out[rows(s)] = keep[among.index(s)]
        else:
            out[rows(s)] = keep[extra]
            extra += 1
    return out


def _same_rows(A, B):
    """The same rows, bit for bit, in any order: get_points lists a pose leaf by leaf, the definition in the order of
    the cloud as inserted."""
    A, B = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
    return A.shape == B.shape and A[np.lexsort(A.T)].tobytes() == B[np.lexsort(B.T)].tobytes()


def _lattice_grid():
    P, _ = lattice01()
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P[::2])
    g.insert_points(1, P[1::2])
    g.subdivide([MaxPoints(8)])
    assert g._forest.nodes["depth"].max() >= 2
    return g, P


def _sparse_cloud():
    """Occupied unit voxels with gaps, negative indices too, some points on leaf and voxel walls."""
    rng = np.random.default_rng(2)
    vox = np.argwhere(rng.random((5, 5, 3)) < 0.45) - [2, 2, 1]
    P = np.concatenate([v + rng.random((60, 3)) for v in vox])
    P[:300:3] = np.floor(P[:300:3] * 8) / 8
    Q = np.concatenate([P[::2] + rng.normal(0.0, 0.02, (len(P[::2]), 3)), P[:200], rng.uniform(-3.0, 4.0, (400, 3)),
                        np.floor(P[:100]), np.floor(P[:100]) + [0.0, 0.5, 1.0], BAD])
    return P, Q


# ---- cell_count ----------------------------------------------------------------------------------------------------
def test_lattice_walls_that_rounding_moved():
    g, P = _lattice_grid()
    up, down = ulp_neighbours(P)
    Q = np.concatenate([P, up[::3], down[::3], np.column_stack([up[::5, 0], P[::5, 1], down[::5, 2]]), BAD,
                        np.empty((0, 3))])
    clouds = [(0, P[::2]), (1, P[1::2])]
    ref = _check_count(g, Q, clouds, CELL, "lattice")
    assert ref.max() > 1 and (ref[:len(P)] >= 1).all() and np.all(ref[-len(BAD):] == 0)
    _check_count(g, Q[::5], clouds[1:], CELL, "lattice, pose 1", pose_numbers=[1])
    e = cell_count(g, np.empty((0, 3)), CELL)
    assert e.shape == (0,) and e.dtype == np.int32


def test_geometry_cells_of_every_size():
    rng = np.random.default_rng(5)
    # a grid whose voxel edge is 1 with missing voxels
    P, Q = _sparse_cloud()
    g = _grid({0: P[::2], 1: P[1::2]}, 10)
    assert g._forest.nodes["depth"].max() >= 2
    smallest = float(g._forest.nodes["edge"].min())
    clouds = [(0, P[::2]), (1, P[1::2])]
    for cell in (1.0, 0.7, CELL, smallest / 4.0):       # the voxel edge, across voxel walls, below the deepest leaf
        ref = _check_count(g, Q, clouds, cell, "sparse grid", caps=(None, 3))
        assert ref.sum() > 0 and (ref == 0).any() and np.all(ref[-len(BAD):] == 0)
    assert _check_count(g, Q[::3], clouds, 1.0, "sparse grid, every cap").max() >= 60
    only0 = _check_count(g, Q[::3], clouds[:1], 0.7, "sparse grid, pose 0", pose_numbers=[0], caps=(None, 1))
    assert 0 < only0.sum() < cell_count_np(Q[::3], clouds, 0.7).sum()
    # a cube that is not dyadic: corners of the children are rounded sums
    c0, e0 = 0.1, 3.3
    t = Octree(OctreeConfig(), np.array([c0, c0, c0]), e0)
    X = c0 + rng.random((4000, 3)) * e0 * [1.0, 1.0, 0.3]
    X = X[np.all((X - c0 >= 0) & (X - c0 < e0), axis=1)]
    t.insert_points(X)
    t.subdivide([MaxPoints(20)])
    nd = t._forest.nodes
    assert nd["depth"].max() >= 3
    inner = np.nonzero(nd["first_child"] >= 0)[0]
    split = nd["corner"][inner] + (nd["edge"][inner] / 2.0)[:, None]
    Qt = np.concatenate([X[:600] + rng.normal(0.0, 0.01, (600, 3)), X[:200], split[:200],
                         np.nextafter(split[:100], -9.0), rng.uniform(-0.5, 4.0, (300, 3)), BAD])
    for cell in (1.0, 0.7, CELL, 0.01):
        ref = _check_count(t, Qt, [(0, X)], cell, "octree", octree=True, caps=(None, 7))
        assert ref.sum() > 0 and (ref == 0).any()
    _check_count(t, Qt[::3], [(0, X)], 0.3, "octree, every cap", octree=True)
    # a manager: one cube, pose numbers that are not slots
    m = OctreeManager(Octree, OctreeConfig(), np.array([-4.0, -4.0, -4.0]), 8.0)
    Pm = {4: rng.uniform(-4.0, 4.0, (3000, 3)) * [1, 1, 0.2], 9: rng.uniform(-4.0, 4.0, (2000, 3)) * [1, 0.2, 1]}
    for p, Y in Pm.items():
        m.insert_points(p, Y)
    m.subdivide([MaxPoints(25)])
    Qm = np.concatenate([rng.uniform(-5.0, 5.0, (400, 3)) * [1, 1, 0.3], Pm[9][:200], BAD])
    both = _check_count(m, Qm, [(4, Pm[4]), (9, Pm[9])], 0.5, "manager")
    only9 = _check_count(m, Qm, [(9, Pm[9])], 0.5, "manager, pose 9", pose_numbers=[9])
    assert (only9 <= both).all() and (only9 < both).any() and (both > 3).any()


# ---- thin ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene():
    """Three poses, about 4 k points over a few voxels: uniform background (a few points per cell of 0.25), the 0.1
    lattice, duplicates inside a pose and across poses, and pairs either side of a voxel wall in one cell of 0.7."""
    rng = np.random.default_rng(11)
    lat, _ = lattice01(-4, 4)
    back = rng.uniform(-1.0, 2.0, (3000, 3))
    poses = {0: [], 1: [], 2: []}
    for X in (lat + [3.0, 0.0, 0.0], back):
        which = rng.integers(0, 3, len(X))
        for p in poses:
            poses[p].append(X[which == p])
    wall = np.array([[1.4 - 2.0 ** -10, 5.5, 5.5], [1.4 + 2.0 ** -10, 5.5, 5.5], [2.0 - 2.0 ** -10, 7.5, 5.5],
                     [2.0, 7.5, 5.5]])                                    # cell walls of 0.7 at 1.4 and 2.1; a voxel wall at 2
    poses[1].append(wall)
    poses[0].append(np.array([[20.5, 12.5, 7.5]]))                        # the same coordinates in two poses ...
    poses[2].append(np.array([[20.5, 12.5, 7.5], [20.5, 12.5, 7.5]]))      # ... and twice in one
    poses[2].append(back[:40])                                            # duplicates of stored points of any pose
    clouds = {p: np.ascontiguousarray(np.concatenate(v)) for p, v in poses.items()}
    for c in clouds.values():
        c.setflags(write=False)
    Q = np.concatenate([back[:300] + 0.01, lat[:100] + [3.0, 0.0, 0.0], wall, BAD])
    return clouds, np.ascontiguousarray(Q)


@pytest.mark.parametrize("cell,m", [(0.25, 1), (0.25, 2), (0.25, 5), (0.7, 1), (CELL, 1)])
def test_thin_is_apply_host_mask_of_the_keep_rule(cell, m):
    clouds, Q = _scene()
    a, b = _grid(clouds, 16), _grid(clouds, 16)
    fa, fb = a._forest, b._forest
    assert fa.nodes["depth"].max() >= 2 and fa.xyz.tobytes() == fb.xyz.tobytes()
    before = {p: a.get_points(p).copy() for p in clouds}
    n_nodes = len(fa.nodes["depth"])
    keep = _thin_keep(fb, cell, m)
    assert 0 < keep.sum() < len(keep)
    removed = thin(a, cell, m)
    assert removed == int((~keep).sum()) == sum(len(v) for v in before.values()) - fa.n_ord
    fb.apply_host_mask(keep.astype(np.uint8))
    _assert_same_map(a, b, f"thin({cell}, {m})", Q, 0.3)
    # every pose's get_points: the rows the definition keeps of the clouds as they were inserted, bit for bit
    names = sorted(clouds)
    kept = thin_keep_np([(p, clouds[p]) for p in names], None, cell, m)
    for p, k in zip(names, kept):
        assert _same_rows(a.get_points(p), clouds[p][k]), (cell, m, p)
        assert a.n_points(p) == int(k.sum())
    left = [(p, a.get_points(p)) for p in names]
    after = cell_count(a, Q, cell)
    assert np.array_equal(after, cell_count_np(Q, left, cell)) and after.max() <= m
    # what was occupied stays occupied, nothing holds more than m, and a second round removes nothing
    was = cell_count_np(Q, [(p, before[p]) for p in names], cell)
    assert np.array_equal(after, np.minimum(was, m))
    if m == 1:
        assert thin(a, cell) == 0
        # duplicates: the smallest id stays - pose 0's row of the pair of poses, none of pose 2's copies
        dup = np.array([20.5, 12.5, 7.5])
        assert [int((X == dup).all(axis=1).sum()) for _, X in left] == [1, 0, 0]
    else:
        assert thin(a, cell, m) == 0
    # the scheme stays; prune afterwards drops what became empty, and the count is still its definition
    assert len(fa.nodes["depth"]) == n_nodes
    a.prune()
    assert np.array_equal(cell_count(a, Q, cell), after)
    for p, k in zip(names, kept):
        assert _same_rows(a.get_points(p), clouds[p][k]), (cell, m, p, "after prune")


@pytest.mark.parametrize("tested,among", [((2,), None), ((2,), (0, 1)), ((0, 2), (1, 2)), (None, (1,))])
def test_pose_numbers_and_among(tested, among):
    clouds, Q = _scene()
    a, b = _grid(clouds, 16), _grid(clouds, 16)
    fa, fb = a._forest, b._forest
    before = {p: a.get_points(p).copy() for p in clouds}
    cell, m = 0.25, 2
    keep = _thin_keep(fb, cell, m, tested, among)          # (pose numbers are slots in this scene)
    judged = sorted(clouds) if tested is None else list(tested)
    removed = thin(a, cell, m, pose_numbers=None if tested is None else list(reversed(tested)),
                   among=None if among is None else list(among))
    assert removed == int((~keep).sum()) > 0
    fb.apply_host_mask(keep.astype(np.uint8))
    _assert_same_map(a, b, f"tested {tested}, among {among}", Q, 0.3)
    counted = sorted(clouds) if among is None else list(among)
    for p in clouds:
        if p not in judged or (p not in counted and p < min(counted)):
            assert a.get_points(p).tobytes() == before[p].tobytes(), p      # untested, or nothing comes before it
    # the definition over the clouds as inserted, a tested pose that is not counted given by its points and its place
    kept = thin_keep_np([(p, clouds[p]) for p in counted],
                        [p if p in counted else (p, clouds[p], sum(1 for q in counted if q < p)) for p in judged], cell, m)
    extra = len(counted)
    for p in judged:
        if p in counted:
            k = kept[counted.index(p)]
        else:
            k, extra = kept[extra], extra + 1
        assert _same_rows(a.get_points(p), clouds[p][k]), p
    with pytest.raises(KeyError):
        thin(a, cell, m, pose_numbers=[4])
    with pytest.raises(KeyError):
        thin(a, cell, m, among=[4])


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
    # the definition evaluated BEFORE the call: what the pending mask is about to drop still occupies cells and is judged
    keep = _thin_keep(fb, 0.05, 2)
    both = masks[1].astype(bool) & keep
    assert both.sum() < masks[1].sum() and both.sum() < keep.sum()            # each of the two removes something
    assert ((~masks[1].astype(bool)) & keep).any()
    for g in (a, plain):
        cell_count(g, Q[:1], 0.05)                   # (the index of every pose is in place)
    before = fa.n_ord
    removed, cost = _launches(lambda: thin(a, 0.05, 2))
    _, cost_plain = _launches(lambda: thin(plain, 0.05, 2))
    assert cost == cost_plain, (cost, cost_plain)    # one compaction applies both
    fb.apply_host_mask(both.astype(np.uint8))
    assert removed == before - fb.n_ord
    _assert_same_map(a, b, "thin with a pending RANSAC mask", Q, 0.3)
    assert plain._forest.n_ord == int(keep.sum())


def test_octree_manager_octree_and_compacted_slots():
    rng = np.random.default_rng(3)
    X = rng.uniform(-3.9, 3.9, (3000, 3)) * [1.0, 1.0, 0.3]
    X[2000:2100] = X[:100]
    Q = np.concatenate([X[:200] + 0.01, BAD])
    # a manager: one cube, pose numbers that are not slots; remove_poses then thin works on the compacted slots
    Pm = {4: X[:1000], 6: X[1000:1500], 9: X[1500:]}
    pair = []
    for _ in range(2):
        m = OctreeManager(Octree, OctreeConfig(), np.array([-4.0, -4.0, -4.0]), 8.0)
        for p, Y in Pm.items():
            m.insert_points(p, Y)
        m.subdivide([MaxPoints(25)])
        assert m.remove_poses([6]) > 0
        pair.append(m)
    a, b = pair
    before = {p: a.get_points(p).copy() for p in (4, 9)}
    n_nodes = len(a._forest.nodes["depth"])
    keep = _thin_keep(b._forest, 0.5, 3, [a._slots[9]], None)
    assert thin(a, 0.5, 3, pose_numbers=[9]) == int((~keep).sum()) > 0
    b._forest.apply_host_mask(keep.astype(np.uint8))
    _assert_same_map(a, b, "manager", Q, 0.5)
    k4, k9 = thin_keep_np([(4, Pm[4]), (9, Pm[9])], [9], 0.5, 3)
    assert k4.all() and a.get_points(4).tobytes() == before[4].tobytes()
    assert _same_rows(a.get_points(9), Pm[9][k9]) and 0 < k9.sum() < len(k9)
    left = [(4, a.get_points(4)), (9, a.get_points(9))]
    assert np.array_equal(cell_count(a, Q, 0.5), cell_count_np(Q, left, 0.5))
    assert len(a._forest.nodes["depth"]) == n_nodes
    # an octree: no pose arguments
    pair = []
    for _ in range(2):
        t = Octree(OctreeConfig(), np.array([-4.0, -4.0, -4.0]), 8.0)
        t.insert_points(X)
        t.subdivide([MaxPoints(25)])
        pair.append(t)
    a, b = pair
    keep = _thin_keep(b._forest, 0.5, 2)
    assert thin(a, 0.5, 2) == int((~keep).sum()) > 0
    b._forest.apply_host_mask(keep.astype(np.uint8))
    _assert_same_map(a, b, "octree", Q, 0.5)
    k, = thin_keep_np([(0, X)], None, 0.5, 2)
    assert _same_rows(a.get_points(), X[k]) and 0 < k.sum() < len(k)
    assert np.array_equal(cell_count(a, Q, 0.5, max_count=9), cell_count_np(Q, [(0, X[k])], 0.5, max_count=9))
    assert thin(a, 0.5, 2) == 0
    a.prune()
    assert _same_rows(a.get_points(), X[k])
    assert np.array_equal(cell_count(a, Q, 0.5), cell_count_np(Q, [(0, X[k])], 0.5))
    with pytest.raises(ValueError, match="single pose"):
        thin(a, 0.5, pose_numbers=[0])
    with pytest.raises(ValueError, match="single pose"):
        thin(a, 0.5, among=[0])
    with pytest.raises(ValueError, match="single pose"):
        cell_count(a, Q, 0.5, pose_numbers=[0])
    with pytest.raises(ValueError, match="reach"):
        cell_count(a, Q, 4.0 * 2.0 ** -50)
    assert _same_rows(a.get_points(), X[k])


# ---- launches, refusals ----------------------------------------------------------------------------------------------
def test_launch_shape_is_that_of_the_radius_counterparts_and_does_not_depend_on_the_size_of_the_map():
    costs = {}
    for n in (2000, 20000):
        P = synthetic.planar_cloud(n, (2, 2, 2), seed=4, sigma=0.002)
        pair = [_grid({0: P[: n // 2], 1: P[n // 2:]}, 48) for _ in range(2)]
        for g in pair:
            f = g._forest
            f.apply_host_mask(np.ones(f.n_ord, dtype=np.uint8))      # (warm: the buffers of the compaction exist)
            cell_count(g, P[:1], 0.05)                               # (... and the index of every pose is in place)
            f.ctx.sync()
        g, twin = pair
        dc = DeviceCloud(P[:500])
        cell_count(g, dc, 0.05)
        g.radius_count(dc, 0.05)
        got, costs[n, "count"] = _launches(lambda: cell_count(g, dc, 0.05, max_count=3))
        _, costs[n, "radius_count"] = _launches(lambda: g.radius_count(dc, 0.05, max_count=3))
        assert np.array_equal(got, np.minimum(cell_count_np(P[:500], [(0, g.get_points(0)), (1, g.get_points(1))], 0.05), 3))
        assert costs[n, "count"][0] == 1 and costs[n, "count"] == costs[n, "radius_count"]      # one launch
        removed, costs[n] = _launches(lambda: thin(g, 0.05))
        _, costs[n, "sparse"] = _launches(lambda: twin.remove_sparse(0.05, 4))
        assert 0 < removed < n and costs[n] == costs[n, "sparse"], costs
        for h in pair:
            h.radius_count(P[:1], 0.05, pose_numbers=[0])
        _, costs[n, "sel"] = _launches(lambda: thin(g, 0.05, pose_numbers=[1], among=[0]))
        _, costs[n, "sparse sel"] = _launches(lambda: twin.remove_sparse(0.05, 4, pose_numbers=[1], among=[0]))
        assert costs[n, "sel"] == costs[n, "sparse sel"], costs
    print("thin (launches, host waits):", costs)
    for key in (None, "count", "sel"):
        assert costs[2000 if key is None else (2000, key)] == costs[20000 if key is None else (20000, key)], costs


def test_every_refusal_leaves_the_map_as_it_was():
    clouds = {p: synthetic.planar_cloud(2000, (2, 2, 2), seed=6, stream=p, sigma=0.002) for p in (0, 1)}
    g = Grid(GridConfig(voxel_edge_length=1))
    for p, P in clouds.items():
        g.insert_points(p, P)
    f = g._forest
    lib, h = f.lib, f.handle
    Q = np.ascontiguousarray(np.concatenate([clouds[0][:100], BAD]))
    count = np.full(len(Q), -7, dtype=np.int32)
    n_alive = C.c_int64(-5)
    two, three = np.ones(2, dtype=np.uint8), np.ones(3, dtype=np.uint8)

    def abi_count(m, cell, cap, sel=None, n_sel=0, q=Q, out=count):
        return lib.octl_forest_cell_count(h, nat.ptr(q), m, cell, cap, nat.ptr(sel), n_sel, nat.ptr(out))

    def abi_thin(cell, m, sel=None, n_sel=0, among=None, n_among=0):
        return lib.octl_forest_thin(h, cell, m, nat.ptr(sel), n_sel, nat.ptr(among), n_among, C.byref(n_alive))

    # before subdivide: the library's refusal, as for radius_count
    assert abi_count(100, 0.1, 0) == nat.OCTL_E_STATE and b"cell_count before build" in lib.octl_last_error(f.ctx.handle)
    assert abi_thin(0.1, 1) == nat.OCTL_E_STATE and b"thin before build" in lib.octl_last_error(f.ctx.handle)
    g.subdivide([MaxPoints(48)])
    np.random.seed(0)
    f.ransac_blocks(np.ascontiguousarray(f.order), np.random.random((128, 6)), 0.01)      # a mask is pending
    pts = {p: g.get_points(p).copy() for p in clouds}
    mask = f.device_mask()
    assert 0 < mask.sum() < len(mask)
    a = _counter("octl_debug_launches")
    for cell in (0.0, -0.5, float("nan"), float("inf"), 1.0000001, 2.0 ** -21):
        assert abi_count(100, cell, 0) == nat.OCTL_E_INVALID, cell
        assert abi_thin(cell, 1) == nat.OCTL_E_INVALID, cell
    assert b"voxel edge" in lib.octl_last_error(f.ctx.handle)
    assert abi_count(100, 0.1, -1) == nat.OCTL_E_INVALID and b"max_count" in lib.octl_last_error(f.ctx.handle)
    for m in (0, -1, -2 ** 31):
        assert abi_thin(0.1, m) == nat.OCTL_E_INVALID and b"max_per_cell" in lib.octl_last_error(f.ctx.handle)
    assert abi_count(-1, 0.1, 0) == nat.OCTL_E_INVALID and abi_count(2 ** 31, 0.1, 0) == nat.OCTL_E_INVALID
    assert abi_count(100, 0.1, 0, q=None) == nat.OCTL_E_INVALID and abi_count(100, 0.1, 0, out=None) == nat.OCTL_E_INVALID
    assert abi_count(100, 0.1, 0, three, 3) == nat.OCTL_E_INVALID
    assert abi_thin(0.1, 2, three, 3) == nat.OCTL_E_INVALID and abi_thin(0.1, 2, two, 2, three, 3) == nat.OCTL_E_INVALID
    assert abi_thin(0.1, 2, None, 0, three, 3) == nat.OCTL_E_INVALID
    assert abi_count(0, 0.1, 0) == 0 and lib.octl_forest_cell_count_device(h, None, 0, 0.1, 0, None, 0, None) == 0
    assert _counter("octl_debug_launches") == a and n_alive.value == -5 and np.all(count == -7)      # nothing ran
    for bad in (0.0, float("nan"), "x", None, 1.5, 2.0 ** -21):
        with pytest.raises(ValueError):
            cell_count(g, Q, bad)
        with pytest.raises(ValueError):
            thin(g, bad)
    for bad in (0, -1, 2 ** 31, 1.5, True):
        with pytest.raises(ValueError):
            cell_count(g, Q, 0.1, max_count=bad)
        with pytest.raises(ValueError):
            thin(g, 0.1, bad)
    with pytest.raises(ValueError):
        thin(g, 0.1, None)
    with pytest.raises(ValueError):
        cell_count(g, np.zeros((4, 2)), 0.1)
    with pytest.raises(ValueError, match="float64"):
        cell_count(g, DeviceCloud(Q[:10].astype(np.float32)), 0.1)
    with pytest.raises(KeyError):
        cell_count(g, Q, 0.1, pose_numbers=[3])
    with pytest.raises(KeyError):
        thin(g, 0.1, pose_numbers=[3])
    with pytest.raises(KeyError):
        thin(g, 0.1, among=[3])
    for other in (None, f, np.zeros((3, 3))):
        with pytest.raises(TypeError):
            cell_count(other, Q, 0.1)
        with pytest.raises(TypeError):
            thin(other, 0.1)
    assert np.array_equal(f.device_mask(), mask)
    for p in clouds:
        assert g.get_points(p).tobytes() == pts[p].tobytes()
    # the edges of the allowed range run: the voxel edge itself and 2^-20 of it
    assert abi_count(len(Q), 1.0, 0) == 0 and count[:100].min() >= 1 and np.all(count[-len(BAD):] == 0)
    assert abi_count(len(Q), 2.0 ** -20, 1) == 0 and count.max() <= 1
    assert np.array_equal(f.device_mask(), mask)          # a count leaves the pending mask alone
    # ... and the call that is not refused applies both
    before = f.n_ord
    keep = _thin_keep(f, 0.1, 2)
    removed = thin(g, 0.1, 2)
    assert removed == before - int((mask.astype(bool) & keep).sum()) > before - int(mask.sum())
    # rows moved outside their leaves: no cube bounds what it holds
    g.map_leaf_points(lambda p: p + np.array([0.0, 0.0, 0.4]), [1])
    with pytest.raises(RuntimeError, match="outside their leaves"):
        cell_count(g, Q[:10], 0.1)
    with pytest.raises(RuntimeError, match="outside their leaves"):
        thin(g, 0.1)
    assert abi_count(100, 0.1, 0) == nat.OCTL_E_STATE
