"""Let go of poses: octl_forest_remove_poses and Grid / OctreeManager .remove_poses.

Two oracles, both on bits (np.array_equal / tobytes: there is no tolerance to state).  INVARIANCE: everything a remaining
pose reads back, and every map query restricted to the remaining poses, is snapshotted before the removal and compared
with the same call over "every pose" afterwards.  TWIN: a second map that never had the removed pose must agree in the
node table, the block table, perm, the ordered points and per-pose get_points - also after both went on (a new pose, a
fresh subdivide, RANSAC, a pose write-back), which is what reads the squeezed store and the refolded voxel box.

The scene: voxel edge 2, synthetic.planar_cloud over 3 x 3 x 2 voxels, MaxPoints(32), a fixed hypothesis table; poses of
1001, 778, 1535 and 2048 rows (the odd ones move every later pose by an odd shift: 24 bytes mod 16 = 8, the source of the
store pass is then 8 bytes off its destination's 16-byte units) plus late poses of 1 row and of 0 rows.  The store kernel
takes 2048 rows per workgroup (store.hip: RT_ROWS_PER_WG; the CPU test pins the constant): pose boundaries fall inside
workgroups and the store spans three of them."""

import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from octreelib_amd import MaxPoints, synthetic
from octreelib_amd import _native as nat
from octreelib_amd.feed import DeviceCloud
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree_manager import OctreeManager
from octreelib_amd.registration import se3_exp
from tests._util import assert_same_leaves, canon, set_option

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# store.hip: RT_ROWS_PER_WG = 256 threads x RT_UNITS 16-byte units x 2 doubles / 3 per row (the one place it is kept)
ROWS_PER_WG = 256 * int(re.search(r"constexpr int RT_UNITS = (\d+);", open(os.path.join(
    ROOT, "octreelib_amd", "csrc", "store.hip")).read()).group(1)) * 2 // 3
assert ROWS_PER_WG == 2048      # (what the pose sizes below were chosen against: the store spans three workgroups)
SHAPE_BUILT = (4, 2)             # launches, host waits of one call on a built forest ...
SHAPE_STORE_ONLY = (2, 1)        # ... and on a forest without tables (the store pass, the count of its flags)
EDGE = 2
DIMS = (3, 3, 2)
SIZES = [1001, 778, 1535, 2048]
COUNT = [MaxPoints(32)]
TABLE = np.random.default_rng(4).random((128, 6))
THRESHOLD = 0.02


# ---- helpers (the small ones are those of tests/test_gpu_transform_poses.py) ----------------------------------------
def _grid():
    return Grid(GridConfig(voxel_edge_length=EDGE))


def _cloud(n, seed=31, stream=0):
    return np.ascontiguousarray(EDGE * synthetic.planar_cloud(n, DIMS, seed=seed, stream=stream, sigma=0.002))


def _rigid(axis, angle, t):
    w = np.asarray(axis, dtype=np.float64)
    return se3_exp(np.concatenate([w / np.linalg.norm(w) * angle, np.asarray(t, dtype=np.float64)]))


def _same_bits(a, b, what):
    if dataclasses.is_dataclass(a):
        assert type(a) is type(b), what
        for fld in dataclasses.fields(a):
            _same_bits(getattr(a, fld.name), getattr(b, fld.name), f"{what}.{fld.name}")
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), what
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


def _assert_same_grid(A, B, poses, what):
    for p in poses:
        for count in ("n_points", "n_leaves", "n_nodes"):
            assert getattr(A, count)(p) == getattr(B, count)(p), (what, count, p)
        for non_empty in (True, False):
            la, lb = A.get_leaf_points(p, non_empty), B.get_leaf_points(p, non_empty)
            assert_same_leaves(_table(la), _table(lb))
            _same_bits(_leaf_points(la), _leaf_points(lb), f"{what}: leaf points of pose {p}")
        _same_bits(A.get_points(p), B.get_points(p), f"{what}: get_points({p})")


def _assert_twin(A, B, poses, what, epoch=True):
    """The twin comparison: the tables of the two forests bit for bit, then everything a pose reads back."""
    fa, fb = A._forest, B._forest
    fa._invalidate()
    fb._invalidate()
    assert A._slots == B._slots, what
    assert fa.store_size() == fb.store_size(), what
    for k in ("voxel", "depth", "parent", "first_child", "corner", "edge") + (("epoch",) if epoch else ()):
        _same_bits(fa.nodes[k], fb.nodes[k], f"{what}: nodes.{k}")
    _same_bits(fa.voxels, fb.voxels, f"{what}: voxels")
    for k in ("node", "slot", "start", "size"):
        _same_bits(fa.blocks[k], fb.blocks[k], f"{what}: blocks.{k}")
    _same_bits(fa.perm, fb.perm, f"{what}: perm")
    _same_bits(fa.xyz, fb.xyz, f"{what}: ordered points")
    _assert_same_grid(A, B, poses, what)


def _counter(name):
    c = C.c_uint64(0)
    nat.get_context().check(getattr(nat.load(), name)(C.byref(c)))
    return c.value


def _deltas(fn):
    a = (_counter("octl_debug_launches"), _counter("octl_debug_host_syncs"))
    fn()
    return _counter("octl_debug_launches") - a[0], _counter("octl_debug_host_syncs") - a[1]


def _split(P, sizes):
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [(p, P[off[p]:off[p + 1]]) for p in range(len(sizes))]


def _try(fn):
    """The answer, or the kind of refusal: both must be the same before and after."""
    try:
        return ("answer", fn())
    except Exception as e:   # noqa: BLE001 (whatever the call raises for this selection is part of its answer)
        return ("raises", type(e).__name__)


def _fit(g):
    g.map_leaf_points_cuda_ransac(poses_per_batch=2, threshold=THRESHOLD, hypotheses=TABLE)


def _scene(scheme=None, fit=True):
    """The issue's scene: four poses, the scheme (from `scheme`, None: all), the two late poses, RANSAC + apply_mask +
    a count filter."""
    clouds = _split(_cloud(sum(SIZES)), SIZES)
    g = _grid()
    for p, X in clouds:
        g.insert_points(p, X)
    g.subdivide(COUNT, pose_numbers=scheme)
    late = _cloud(1, stream=7)
    g.insert_points(4, late)
    g.insert_points(5, np.empty((0, 3)))
    if fit:
        _fit(g)
        g.filter([lambda pts: len(pts) >= 5])
    return g, clouds + [(4, late), (5, np.empty((0, 3)))]


QUERIES = _cloud(700, stream=3) + 0.01
RAY_O = _cloud(300, stream=4) + np.array([-7.0, 0.1, 0.05])
RAY_D = np.tile(np.array([[1.0, 0.02, 0.01], [1.0, -0.05, 0.03], [0.9, 0.3, -0.1]]), (100, 1))


def _pose_rows(g, p):
    """The rows of pose p in storage order, numbered within the pose (perm minus the pose's offset)."""
    f = g._forest
    s = g._slots[p]
    off = np.concatenate([[0], np.cumsum(f.slot_sizes)]).astype(np.int64)
    perm = f.perm
    return perm[(perm >= off[s]) & (perm < off[s + 1])] - off[s]


def _snapshot(g, poses, sel):
    """Everything the poses read back, and every map query over the selection `sel` (None: every pose)."""
    g._forest._invalidate()
    out = []
    for p in poses:
        out += [g.get_points(p), _pose_rows(g, p), [g.n_points(p), g.n_leaves(p), g.n_nodes(p)],
                _try(lambda: g.leaf_statistics(p))]
        for non_empty in (True, False):
            lv = g.get_leaf_points(p, non_empty)
            out += [np.array([v.corner_min for v in lv], dtype=np.float64).reshape(-1, 3),
                    np.array([v.edge_length for v in lv], dtype=np.float64), [v.n_points for v in lv], _leaf_points(lv)]
    out += [
        _try(lambda: g.leaf_planes(sel)),
        _try(lambda: g.point_to_plane(QUERIES, sel, 8, 1e-2)),
        _try(lambda: g.nearest(QUERIES, 4, max_distance=0.3, pose_numbers=sel)),
        _try(lambda: g.raycast(RAY_O, RAY_D, 12.0, pose_numbers=sel)),
        _try(lambda: g.raycast(RAY_O, RAY_D, 12.0, pose_numbers=sel, surface="plane", max_variance=1e-2)),
        _try(lambda: g.plane_segments(sel, max_variance=1e-2)),
        _try(lambda: g.registration_system(QUERIES, None, sel, max_variance=1e-2)),
        _try(lambda: g.adjustment_system(None, sel, max_variance=1e-2)),
        g.node_cubes(), g.locate(QUERIES),
    ]
    return out


# ---- invariance --------------------------------------------------------------------------------------------------
CASES = {
    "first": ([0], None),
    "middle": ([2], None),
    "last-full-pose": ([3], None),            # everything behind it is the two late poses
    "two-non-adjacent": ([1, 3], None),
    "zero-rows": ([5], None),                 # (also the last slot)
    "one-row": ([4], None),
    "the-only-scheme-pose": ([1], [1]),
    "every-pose": ([0, 1, 2, 3, 4, 5], None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_invariance(name):
    removed, scheme = CASES[name]
    g, clouds = _scene(scheme)
    f = g._forest
    stay = [p for p, _ in clouds if p not in removed]
    sizes = dict((p, len(X)) for p, X in clouds)
    alive = {p: g.n_points(p) for p, _ in clouds}
    print(f"{name}: alive rows per pose {alive}")
    assert 0 < sum(alive.values()) < sum(SIZES) and alive[3] > 0      # (RANSAC and the filter removed some, not all)
    before = _snapshot(g, stay, stay)
    if stay:    # a refusal is an answer only for the empty selection: here every query must have answered
        assert [kind for kind, _ in before[-10:-2]] == ["answer"] * 8, [a for a in before[-10:-2] if a[0] != "answer"]
        assert all(before[i + 3][0] == "answer" for i in range(0, 12 * len(stay), 12) if alive[stay[i // 12]] > 0)
    left = g.remove_poses(removed)
    assert left == sum(alive[p] for p in removed)
    assert sorted(g._slots) == stay and sorted(g._slots.values()) == list(range(len(stay)))
    assert f.store_size() == (sum(sizes[p] for p in stay), sum(alive[p] for p in stay), len(stay))
    _same_bits(_snapshot(g, stay, None), before, name)
    # the numbers are free again: a late pose under one of them inherits the scheme
    fresh = _cloud(333, stream=9)
    g.insert_points(removed[0], fresh)
    assert g.n_points(removed[0]) == len(fresh)
    same = lambda a, b: sorted(r.tobytes() for r in a) == sorted(r.tobytes() for r in np.ascontiguousarray(b))
    assert same(g.get_points(removed[0]), fresh)
    for p, i in zip(stay, range(0, len(before), 12)):
        _same_bits(g.get_points(p), before[i], f"{name}: get_points({p}) behind a new pose")
    if name == "every-pose":     # a fresh subdivide on what is now a one-pose map
        g.subdivide(COUNT)
        assert g.n_points(removed[0]) == len(fresh) and same(g.get_points(removed[0]), fresh)
        assert f.store_size() == (len(fresh), len(fresh), 1)


def test_octree_manager():
    make = lambda: OctreeManager(Octree, OctreeConfig(), np.array([-4.0, -4.0, -4.0]), 8.0)
    rng = np.random.default_rng(6)
    mc = [(4, rng.uniform(-3.5, 3.5, (1501, 3)) * [1, 1, 0.2]), (9, rng.uniform(-3.5, 3.5, (777, 3)) * [1, 0.2, 1]),
          (2, rng.uniform(-3.5, 3.5, (1000, 3)) * [0.2, 1, 1])]
    A, B = make(), make()
    for p, X in mc:
        A.insert_points(p, X)
        if p != 4:
            B.insert_points(p, X)
    for M in (A, B):
        M.subdivide([MaxPoints(25)], pose_numbers=[9, 2])
        M.filter([lambda pts: len(pts) >= 3])
    n4 = A.n_points(4)
    assert A.remove_poses([4]) == n4 > 0
    assert A._forest.store_size()[0] == 1777 and A._slots == B._slots
    for p in (9, 2):
        _same_bits(A.get_points(p), B.get_points(p), f"manager: get_points({p})")
        assert (A.n_points(p), A.n_leaves(p), A.n_nodes(p)) == (B.n_points(p), B.n_leaves(p), B.n_nodes(p))
    _same_bits(A._forest.perm, B._forest.perm, "manager: perm")
    _same_bits(A.leaf_planes(), B.leaf_planes(), "manager: leaf_planes")
    with pytest.raises(KeyError):
        A.remove_poses([4])


# ---- the twin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused-compaction", "separate-scan"])
def test_twin(fused):
    if not fused:       # apply_mask's other form (large maps): the reservations in front of it differ
        set_option("NO_FUSED_TABLES", 1)
    clouds = _split(_cloud(sum(SIZES)), SIZES)
    for p, X in clouds:    # every pose has points in every voxel: both maps create their voxels in the same order
        q = np.floor_divide(X, EDGE).astype(np.int64)
        assert len(np.unique(q, axis=0)) == int(np.prod(DIMS)), p
    A, B = _grid(), _grid()
    for p, X in clouds:
        A.insert_points(p, X)
        if p != 0:
            B.insert_points(p, X)
    for g in (A, B):
        g.subdivide(COUNT, pose_numbers=[1, 2, 3])
        g.filter([lambda pts: len(pts) >= 6])       # (dead rows that keep their place; per (leaf, pose): pose 0 apart)
    assert 0 < sum(B.n_points(p) for p in (1, 2, 3)) < sum(SIZES[1:])
    n0 = A.n_points(0)
    assert A.remove_poses([0]) == n0 > 0
    _assert_twin(A, B, [1, 2, 3], "after the removal")
    # both go on: the number is taken again, a FRESH subdivide reads the squeezed store and the refolded box
    again = _cloud(1203, stream=5)
    T = _rigid((0, 0, 1), 0.2, (3.0, -2.0, 1.0))
    for g in (A, B):
        g.insert_points(0, again)
        g.subdivide(COUNT)
        _fit(g)
    _assert_twin(A, B, [1, 2, 3, 0], "after a new pose, a fresh subdivide and RANSAC")
    for g in (A, B):
        g.transform_poses([T], pose_numbers=[2])
        g.subdivide(COUNT)
    _assert_twin(A, B, [1, 2, 3, 0], "after a pose write-back and another subdivide")


def test_the_refolded_box_is_the_remaining_poses_box():
    """A pose far away leaves: the next fresh build forms its key geometry from the box of what stayed, and every
    remaining pose reads back what it reads from a map that never saw the far pose."""
    near = _split(_cloud(3000), [1001, 1999])
    far = _cloud(901, stream=2) + np.array([4000.0, -2000.0, 600.0])
    A, B = _grid(), _grid()
    A.insert_points(7, far)
    for p, X in near:
        A.insert_points(p, X)
        B.insert_points(p, X)
    A.subdivide(COUNT)
    assert A.remove_poses([7]) == len(far)
    A.subdivide(COUNT)
    B.subdivide(COUNT)
    # (the far pose's voxels stay, empty: the scheme never forgets a voxel)
    assert set(map(tuple, B._forest.voxels)) < set(map(tuple, A._forest.voxels))
    _assert_same_grid(A, B, [0, 1], "after the far pose left")
    _same_bits(A._forest.perm, B._forest.perm, "perm")


# ---- a window that travels ---------------------------------------------------------------------------------------
def test_window():
    """Twelve scans through a window of three, nine removals one behind the other.  The last map against a map that
    only ever saw the last three scans, whole, in the same scheme (Forest.adopt_scheme) and with the same rows dead: the
    masks of W's nine fits cannot be had by fitting the twin (a RANSAC batch samples by the running sum of ITS block
    sizes, cuda_ransac.py:64-66,103-107 - those of a window of four), so the twin takes them as ONE mask over its ordered
    points.  Its second and third scan come in late and one by one, as the window's did (a late pose's blocks are stored
    behind the others: storage order is history).  Then the twin comparison holds as everywhere else - node table, block table,
    perm, ordered points, every per-pose read, in order - with one exception by construction: the epoch column
    (adopt_scheme stamps the twin's own counter)."""
    scans = [_cloud(300, seed=41, stream=i) for i in range(12)]
    W = _grid()
    for p in range(3):
        W.insert_points(p, scans[p])
    # the scheme from the first scan alone: a scan has about 17 points per voxel, and RANSAC skips blocks of fewer
    # than six - three scans' worth would split every voxel into leaves no scan fills
    W.subdivide(COUNT, pose_numbers=[0])
    f = W._forest
    # scan k goes in under the number k % 4 - the number the scan that left one step earlier gave back (the RANSAC of
    # the reference takes the pose numbers to be 0 .. n - 1, grid.py:149-157)
    for k in range(3, 12):
        W.insert_points(k % 4, scans[k])
        _fit(W)
        stay = [j % 4 for j in range(k - 2, k + 1)]
        kept = {p: W.get_points(p) for p in stay}
        gone = W.n_points((k - 3) % 4)
        assert W.remove_poses([(k - 3) % 4]) == gone
        n_store, n_alive, n_poses = f.store_size()
        assert (n_store, n_poses) == (900, 3) and n_alive == sum(len(kept[p]) for p in stay)
        assert f.slot_sizes == [300, 300, 300] and sorted(W._slots) == sorted(stay)
        assert [W._slots[p] for p in stay] == [0, 1, 2]
        for p in stay:
            _same_bits(W.get_points(p), kept[p], f"step {k}: get_points({p})")
    last = [9 % 4, 10 % 4, 11 % 4]
    T = _grid()
    ft = T._forest
    for p in last:       # the first scan, the scheme, then the other two LATE, as every scan of the window came in: the
        assert 0 < W.n_points(p) < 300      # block table is in storage order, and a late pose's blocks go behind
        T.insert_points(p, scans[p + 8])
        ft.ensure_built()                   # (placed before the next one comes, as in the window)
        if p == last[0]:
            _same_bits(ft.voxels, f.voxels, "voxels")
            ft.adopt_scheme(f)
    f._invalidate()
    ft.apply_host_mask(np.isin(ft.perm, f.perm).astype(np.uint8))    # (both stores: the three scans, row for row)
    _assert_twin(W, T, last, "the window against a map of its last three scans", epoch=False)


# ---- a forest without tables: the store pass alone -----------------------------------------------------------------
def test_before_any_build_and_straight_after_transform_poses():
    clouds = _split(_cloud(sum(SIZES)), SIZES)
    A, B = _grid(), _grid()
    for p, X in clouds:
        A.insert_points(p, X)
        if p != 1:
            B.insert_points(p, X)
    A._forest.ctx.sync()
    assert _deltas(lambda: A._forest.remove_slots([A._slots[1]])) == SHAPE_STORE_ONLY
    A._slots = {0: 0, 2: 1, 3: 2}
    assert A._forest.store_size() == (sum(SIZES) - SIZES[1], sum(SIZES) - SIZES[1], 3)
    for g in (A, B):
        g.subdivide(COUNT)
    _assert_twin(A, B, [0, 2, 3], "removed before any build")
    # ... and on the store transform_poses leaves: dead rows in place, no scheme
    T = _rigid((0, 1, 0), 0.1, (2.0, 1.0, 0.5))
    A, B = _grid(), _grid()
    for p, X in clouds:
        A.insert_points(p, X)
        if p != 0:
            B.insert_points(p, X)
    for g in (A, B):
        g.subdivide(COUNT, pose_numbers=[1, 2, 3])
        g.filter([lambda pts: len(pts) >= 6])
        g.transform_poses([T], pose_numbers=[2])
    n0 = A._forest.store_size()[1] - B._forest.store_size()[1]
    assert A.remove_poses([0]) == n0 > 0
    assert not A._forest.has_scheme and A._forest.store_size() == B._forest.store_size()
    for g in (A, B):
        g.subdivide(COUNT)
    _assert_twin(A, B, [1, 2, 3], "removed straight after transform_poses")


# ---- a store read in place from the caller's buffer ---------------------------------------------------------------------
def test_borrowed_store_is_never_written():
    P = _cloud(3001, stream=6)
    back = np.empty_like(P)

    def unchanged(f, dc):
        f.ctx.check(f.lib.octl_dev_download(f.ctx.handle, nat.ptr(back), dc.ptr, back.nbytes))
        _same_bits(back, P, "the caller's buffer")

    # the borrowed pose itself leaves (a store is read in place only while it is that one pose)
    dc = DeviceCloud(P)
    A = _grid()
    A.insert_points(0, dc)
    f = A._forest
    A.subdivide(COUNT)
    A.filter([lambda pts: len(pts) >= 12])
    assert f.reads_in_place(dc) and 0 < A.n_points(0) < len(P)
    assert A.remove_poses([0]) > 0
    assert not f.reads_in_place(dc) and f.store_size() == (0, 0, 0)
    unchanged(f, dc)
    X = _cloud(1501, stream=8)
    A.insert_points(0, X)           # lands in the forest's own block
    A.subdivide(COUNT)
    assert A.n_points(0) == len(X)
    unchanged(f, dc)
    f.close()
    # a later pose leaves: the store became the forest's own when it grew; the removal reads and writes only that
    B, R = _grid(), _grid()
    B.insert_points(0, dc)
    B.insert_points(1, X)
    R.insert_points(0, P)
    for g in (B, R):
        g.subdivide(COUNT, pose_numbers=[0])
    assert not B._forest.reads_in_place(dc)
    assert B.remove_poses([1]) == len(X)
    unchanged(B._forest, dc)
    _assert_same_grid(B, R, [0], "after the later pose left")
    _same_bits(B._forest.perm, R._forest.perm, "perm")
    B._forest.close()
    dc.release()


# ---- a pending RANSAC mask, and a compaction whose counts are still on their way -------------------------------------
def test_pending_mask_and_asynchronous_apply_mask():
    def fitted_not_applied():
        g = _grid()
        for p, X in _split(_cloud(sum(SIZES)), SIZES):
            g.insert_points(p, X)
        g.subdivide(COUNT)
        g._forest.ransac_all(2, TABLE, THRESHOLD)
        return g

    pending, asynchronous, settled = fitted_not_applied(), fitted_not_applied(), fitted_not_applied()
    mask = pending._forest.device_mask()
    assert 0 < int(mask.sum()) < len(mask)
    asynchronous._forest.apply_device_mask()
    assert asynchronous._forest._n_ord_pending
    settled._forest.apply_device_mask()
    assert 0 < settled._forest.n_ord < sum(SIZES) and not settled._forest._n_ord_pending
    want = settled.n_points(1)
    assert settled.remove_poses([1]) == want
    assert asynchronous.remove_poses([1]) == want
    assert pending.remove_poses([1]) == sum(SIZES[1:2])     # (its rows were all still alive when it left)
    _assert_twin(asynchronous, settled, [0, 2, 3], "behind an asynchronous apply_mask")
    _assert_twin(pending, settled, [0, 2, 3], "a pending mask goes into the same compaction")


# ---- failure is atomic -------------------------------------------------------------------------------------------
def _arm(nth):
    seen = C.c_int64(0)
    nat.get_context().check(nat.load().octl_debug_fail_alloc(int(nth), C.byref(seen)))
    return seen.value


def _state(g):
    f = g._forest
    f._invalidate()
    near = g.nearest(QUERIES, 4, max_distance=0.3)
    return (f.perm.copy(), f.xyz.copy(), f.blocks["node"].copy(), f.blocks["slot"].copy(), f.blocks["start"].copy(),
            f.device_mask(), list(f.store_size()), [g.get_points(p) for p in sorted(g._slots)], near.pose, near.index,
            near.distance2)


def test_failure_is_atomic():
    """octl_debug_fail_alloc swept over every growth the call makes, each on a map of its own whose buffers have
    never been asked for (a pending RANSAC mask: the compaction's targets do not exist yet)."""
    def fresh():
        g = _grid()
        for p, X in _split(_cloud(sum(SIZES)), SIZES):
            g.insert_points(p, X)
        g.subdivide(COUNT)
        g._forest.ransac_all(2, TABLE, THRESHOLD)
        return g

    ref = fresh()
    ref.remove_poses([1])
    hits = 0
    for nth in range(1, 40):
        g = fresh()
        f = g._forest
        before = _state(g)
        mirror = (dict(g._slots), list(f.slot_sizes), f.n_slots, f.n_ord)
        _arm(nth)
        raised = False
        try:
            g.remove_poses([1])
        except MemoryError as e:
            raised = True
            assert "injected by octl_debug_fail_alloc" in str(e)
        finally:
            _arm(0)
        if raised:
            hits += 1
            assert (dict(g._slots), list(f.slot_sizes), f.n_slots, f.n_ord) == mirror
            _same_bits(_state(g), before, f"after growth {nth} failed")
            g.remove_poses([1])              # disarmed: goes through
        _assert_twin(g, ref, [0, 2, 3], f"growth {nth}")
        f.close()
        if not raised:
            break
    assert not raised and hits >= 3, hits


# ---- launches and host waits -------------------------------------------------------------------------------------
def test_launch_shape_does_not_depend_on_the_size():
    seen = []
    for n in (100, 20006):
        P = _cloud(n, seed=15)
        g = _grid()
        for p in range(5):
            g.insert_points(p, P[p * n // 5:(p + 1) * n // 5])
        g.subdivide(COUNT)
        f = g._forest
        g.remove_poses([4])                  # (the first call on a map may grow buffers)
        assert g.n_points(0) > 0
        f._resolve_membership()
        f.ctx.sync()
        seen.append(_deltas(lambda: g.remove_poses([1])))
        seen.append(_deltas(lambda: g.remove_poses([0])))
        assert f.store_size()[2] == 2 and f.n_ord > 0
    assert seen == [SHAPE_BUILT] * 4, seen


# ---- no-ops and refusals -------------------------------------------------------------------------------------------
def test_no_ops_and_refusals():
    g, clouds = _scene()
    f = g._forest
    f._resolve_membership()
    perm, stamp = f.perm.copy(), f.store_size()
    assert _deltas(lambda: g.remove_poses([])) == (0, 0)
    none = np.zeros(6, dtype=np.uint8)
    new_slot = np.full(6, -7, dtype=np.int32)
    removed = C.c_int64(-1)
    call = lambda sel, n: f.lib.octl_forest_remove_poses(f.handle, nat.ptr(sel), n, nat.ptr(new_slot), C.byref(removed))
    assert _deltas(lambda: f.ctx.check(call(none, 6))) == (0, 0)
    assert new_slot.tolist() == list(range(6)) and removed.value == 0
    assert _deltas(f.ensure_built) == (0, 0) and f.store_size() == stamp
    f._invalidate()
    _same_bits(f.perm, perm, "perm after an empty selection")
    assert call(none, 5) == nat.OCTL_E_INVALID and call(np.ones(7, dtype=np.uint8), 7) == nat.OCTL_E_INVALID
    assert f.lib.octl_forest_remove_poses(None, None, 0, None, None) == nat.OCTL_E_INVALID
    with pytest.raises(KeyError):
        g.remove_poses([0, 17])
    assert f.store_size() == stamp and sorted(g._slots) == list(range(6))
    # built, and grown since: the raw entry refuses; the method brings the map up to date first
    g.insert_points(6, _cloud(200, stream=11))
    one = np.zeros(7, dtype=np.uint8)
    one[2] = 1
    assert f.lib.octl_forest_remove_poses(f.handle, nat.ptr(one), 7, None, None) == nat.OCTL_E_STATE
    assert f.store_size()[2] == 7
    n2 = g.n_points(2)
    assert g.remove_poses([2]) == n2 and g.n_points(6) == 200 and f.store_size()[2] == 6
    # built WITHOUT a scheme (a read before any subdivide) and grown since: the same refusal, the same way out
    h = _grid()
    h.insert_points(0, _cloud(500, stream=12))
    h.insert_points(1, _cloud(401, stream=13))
    kept = h.get_points(1)                      # (builds the top-level voxels: no scheme)
    fh = h._forest
    assert not fh.has_scheme and fh.info is not None
    h.insert_points(2, _cloud(300, stream=14))
    assert fh._dirty
    first = np.array([1, 0, 0], dtype=np.uint8)
    assert fh.lib.octl_forest_remove_poses(fh.handle, nat.ptr(first), 3, None, None) == nat.OCTL_E_STATE
    assert h.remove_poses([0]) == 500 and fh.store_size() == (701, 701, 2) and h._slots == {1: 0, 2: 1}
    _same_bits(h.get_points(1), kept, "scheme-less map: get_points(1)")
    assert h.n_points(2) == 300
    # a pose twice in the list is one pose
    n0 = g.n_points(0)
    assert g.remove_poses([0, 0]) == n0 and f.store_size()[2] == 5
