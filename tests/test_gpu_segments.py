"""Plane segments on the device: octl_forest_plane_segments and Grid / OctreeManager / Octree .plane_segments.

The contract has no tolerance for neighbour, label, root and n_leaves: they EQUAL octreelib_amd.query.plane_segments_np
evaluated on the device's own leaf_planes() bits and node table, because the definition makes every decision on
identical bits.  The merged table stays within the bound of tests/test_cpu_segments.py: table_error_over_bound
(gamma = (ceil(m / 64) + 32) eps against a np.longdouble merge of the same rows; one-leaf segments bit-equal).

Worst error / bound of the merged table over the cases of this file, measured on an MI355X: 0.21."""

import ctypes as C
import math

import numpy as np
import pytest

from octreelib_amd import MaxPoints, NotPlanar, PlaneSegments, plane_segments_np
from octreelib_amd import _native as nat
from octreelib_amd._engine import Forest
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree_manager import OctreeManager
from tests.test_cpu_segments import (DEFAULTS, across_zero, assert_adjacency_across_zero, assert_structure,
                                     face_adjacency, floor_and_wall, gate_values, probe_pairs, table_error_over_bound)
from tests.test_gpu_query import _counter

pytestmark = pytest.mark.gpu

EXACT = ("neighbour", "label")
EXACT_TABLE = ("root", "n_leaves", "count")
# launches and host waits of octl_forest_plane_segments (size query), asserted by test_launch_shape; DESIGN.md 4.12
# has the breakdown.  Both contain the sort's passes: 3 launches per 8 bits of the segment count (one pass here), and
# in a first call the pooled table's own (two passes here).
FIRST_CALL = (22, 2)
ON_POOLED_TABLE = (10, 1)


# ---- helpers -------------------------------------------------------------------------------------------------------
def _spec(obj, pose_numbers=None, octree=False, **args) -> PlaneSegments:
    f = obj._forest
    planes = obj.leaf_planes() if octree else obj.leaf_planes(pose_numbers)
    return plane_segments_np(planes, f.nodes, f.voxels, f.mode, f._cube[1], **{**DEFAULTS, **args})


def _assert_equal(got: PlaneSegments, ref: PlaneSegments, what):
    assert isinstance(got, PlaneSegments)
    for name in ("node", "count", "mean", "covariance", "eigenvalues", "eigenvectors"):
        assert getattr(got.planes, name).tobytes() == getattr(ref.planes, name).tobytes(), (what, name)
    for owner, names in ((lambda x: x, EXACT), (lambda x: x.segments, EXACT_TABLE)):
        for name in names:
            a, b = getattr(owner(got), name), getattr(owner(ref), name)
            assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, a.shape, b.dtype, b.shape)
            if not np.array_equal(a, b):
                bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
                raise AssertionError(f"{what}: {name} differs in {len(bad)} of {len(a)} rows, first {bad[0]}: got "
                                     f"{a[bad[0]].tolist()}, expected {b[bad[0]].tolist()}")


def _check(obj, what, pose_numbers=None, octree=False, **args):
    """The device answer against the definition on the device's own plane bits and node table; the merged table
    within its bound.  Returns (answer, worst error / bound of the table)."""
    ref = _spec(obj, pose_numbers, octree, **args)
    got = obj.plane_segments(**args) if octree else obj.plane_segments(pose_numbers, **args)
    _assert_equal(got, ref, what)
    worst = table_error_over_bound(got)
    t = got.segments
    print(f"{what}: {len(got.label)} rows, {len(t.count)} segments, largest {t.n_leaves.max() if len(t.count) else 0} "
          f"leaves, table error / bound {worst:.3g}")
    assert worst <= 1.0
    return got, worst


def _grid(clouds, rule=None, L=1):
    g = Grid(GridConfig(voxel_edge_length=L))
    for p, P in enumerate(clouds):
        g.insert_points(p, P)
    if rule is not None:
        g.subdivide([rule])
    return g


def _plane_patch(lo, hi, z, n, rng, axis=2, sigma=0.0):
    """n points of the plane coordinate[axis] = z over the box lo .. hi of the other two axes."""
    P = np.empty((n, 3))
    others = [a for a in range(3) if a != axis]
    for k, a in enumerate(others):
        P[:, a] = rng.uniform(lo[k], hi[k], n)
    P[:, axis] = z + (rng.normal(0.0, sigma, n) if sigma else 0.0)
    return P


def _flat_voxels(cells, per=12, seed=0):
    """`per` points of the plane z = 0.5 (N(0, 2 mm)) inside every listed (x, y) voxel of edge 1."""
    rng = np.random.default_rng(seed)
    cells = np.asarray(cells, dtype=np.float64)
    xy = np.repeat(cells, per, axis=0) + rng.uniform(0.05, 0.95, (len(cells) * per, 2))
    return np.column_stack([xy, 0.5 + rng.normal(0.0, 0.002, len(xy))])


# ---- 1. the CPU scene, three ways ------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", ["grid", "manager", "planar"])
def test_floor_and_wall(way):
    P = floor_and_wall()
    if way == "grid":
        obj, sel = _grid([P], MaxPoints(64)), None
    elif way == "planar":
        obj, sel = _grid([P], NotPlanar(1e-4, min_points=16)), None
    else:
        obj, sel = OctreeManager(Octree, OctreeConfig(), np.array([0.0, 0.0, 0.0]), 8.0), [0, 2]
        for p, part in enumerate(np.array_split(P[np.random.default_rng(3).permutation(len(P))], 3)):
            obj.insert_points(p, part)
        obj.subdivide([MaxPoints(64)])
    got, _ = _check(obj, way, sel)
    assert_structure(got)
    nd = obj._forest.nodes
    ids = got.planes.node
    assert len(np.unique(nd["edge"][ids])) >= (3 if way != "planar" else 2)
    assert probe_pairs(got) == face_adjacency(nd["corner"][ids], nd["edge"][ids])
    t = got.segments
    big = np.argsort(-t.n_leaves, kind="stable")[:3]
    print(way, "largest segments:", t.n_leaves[big], t.normal[big].round(3).tolist())
    if way == "grid":
        assert np.sum(t.n_leaves > 50) >= 2
        assert sorted(int(np.argmax(np.abs(t.normal[s]))) for s in big) == [0, 2, 2]
    for axis in (0, 2):        # the wall and the floor are found, whatever the tree
        assert any(abs(t.normal[s, axis]) >= math.cos(0.1) and t.n_leaves[s] >= 4 for s in range(len(t.count)))
    if way == "manager":
        assert got.planes.count.sum() < len(P)
        _check(obj, "manager, all poses", None)
    # other gates on the same map
    for args in (dict(max_variance=1e-5), dict(max_angle=0.02, max_offset=0.004), dict(min_points=30),
                 dict(min_points=10 ** 6)):
        other, _ = _check(obj, f"{way} {args}", sel, **args)
        assert np.array_equal(other.neighbour, got.neighbour)
        assert way == "planar" or not np.array_equal(other.label, got.label)
    assert len(other.segments.count) == 0 and np.all(other.label == -1)


# ---- 2. across coordinate 0, and a hole in the grid ----------------------------------------------------------------------
def test_across_zero_and_missing_voxel():
    P = across_zero()
    hole = np.all((P >= 0.0) & (P < 1.0), axis=1)     # the voxel (0, 0, 0): the planes z = 0.3 and x = 0.4 cross it
    assert 50 < hole.sum() < len(P)
    g = _grid([P[~hole]], MaxPoints(64))
    got, _ = _check(g, "across zero")
    assert_structure(got)
    f = g._forest
    nd = f.nodes
    _, _, corner, edge = assert_adjacency_across_zero(got, nd, f.voxels, 1.0)
    for a in range(3):
        assert any(np.any(corner[got.label == s, a] < 0) and np.any(corner[got.label == s, a] >= 0)
                   for s in range(len(got.segments.count))), a
    # the subnormal probe finds the unsplit voxel (-1, 1, 1)
    at0 = np.nonzero(corner[:, 0] == 0.0)[0]
    behind = got.neighbour[at0, 0]
    assert np.any(behind >= 0) and np.all(nd["edge"][behind[behind >= 0]] == 1.0)
    # the hole: leaves that look into it see -1
    assert g.locate(np.array([[0.5, 0.5, 0.3]]))[0] == -1
    inside = (corner[:, 1] >= 0) & (corner[:, 1] < 1) & (corner[:, 2] >= 0) & (corner[:, 2] < 1)
    left = np.nonzero((corner[:, 0] + edge == 0.0) & inside)[0]      # (their + probe is the coordinate 0 itself)
    right = np.nonzero((corner[:, 0] == 1.0) & inside)[0]
    assert len(left) and len(right)
    assert np.all(got.neighbour[left, 1] == -1) and np.all(got.neighbour[right, 0] == -1)


# ---- 3. a cube that is not dyadic ---------------------------------------------------------------------------------------
def test_non_dyadic_octree():
    rng = np.random.default_rng(5)
    c0, e0 = 0.1, 3.3
    t = Octree(OctreeConfig(), np.array([c0, c0, c0]), e0)
    P = np.concatenate([c0 + rng.random((3000, 3)) * e0 * [1.0, 1.0, 0.3],
                        _plane_patch((c0, c0), (c0 + e0, c0 + e0), 2.2, 5000, rng, sigma=0.002),
                        _plane_patch((c0, c0), (c0 + e0, c0 + 2.0), 1.7, 3000, rng, axis=0, sigma=0.002)])
    P = P[np.all((P - c0 >= 0) & (P - c0 < e0), axis=1)]
    t.insert_points(P)
    t.subdivide([MaxPoints(40)])
    assert t._forest.nodes["depth"].max() >= 3
    got, _ = _check(t, "octree", octree=True)
    assert_structure(got)
    assert got.segments.n_leaves.max() > 20
    _check(t, "octree, strict", octree=True, max_angle=0.03, max_offset=0.01, min_points=12)


# ---- 4. the union-find under contention ---------------------------------------------------------------------------------
def test_union_find_under_contention():
    # one flat plane over 32 x 32 unsplit voxels: 1024 rows, one component, every union ends in row 0
    cells = [(x, y) for x in range(32) for y in range(32)]
    got, _ = _check(_grid([_flat_voxels(cells)]), "32 x 32 plane")
    assert len(got.label) == 1024 and np.all(got.label == 0) and got.segments.n_leaves.tolist() == [1024]
    # a strip of 256 voxels: a chain of diameter 255
    got, _ = _check(_grid([_flat_voxels([(x, 0) for x in range(256)], seed=1)]), "1 x 256 strip")
    assert len(got.label) == 256 and np.all(got.label == 0) and got.segments.n_leaves.tolist() == [256]
    assert np.array_equal(got.neighbour[:, 0] >= 0, np.arange(256) > 0)
    # a comb: 32 teeth of 8 voxels that join only through the spine
    comb = [(x, 0) for x in range(64)] + [(x, y) for x in range(0, 64, 2) for y in range(1, 9)]
    g = _grid([_flat_voxels(comb, seed=2)])
    got, _ = _check(g, "comb")
    assert len(got.label) == 320 and got.segments.n_leaves.tolist() == [320]
    # ... and without the spine (its voxels hold 12 points, the teeth get 20) every tooth is a segment of its own
    teeth = [(x, y) for x in range(0, 64, 2) for y in range(1, 9)]
    g = _grid([np.concatenate([_flat_voxels(comb, seed=2), _flat_voxels(teeth, per=8, seed=3)])])
    got, _ = _check(g, "comb, spine not eligible", min_points=16)
    assert got.segments.n_leaves.tolist() == [8] * 32 and np.sum(got.label < 0) == 64


# ---- 5. the gates' edges -------------------------------------------------------------------------------------------------
def _margins(ps, **args):
    """Smallest distance of a candidate edge's gate values from their thresholds."""
    a = {**DEFAULTS, **args}
    vals = gate_values(ps, probe_pairs(ps))
    cos_min = math.cos(a["max_angle"])
    return min(min(abs(c - cos_min), abs(oi - a["max_offset"]), abs(oj - a["max_offset"])) for c, oi, oj in vals.values())


def test_gate_edges():
    rng = np.random.default_rng(8)
    mo = 0.05
    for delta, segments in ((1.1 * mo, 2), (0.9 * mo, 1)):
        # two parallel exact planes in adjacent voxels, their offset 10 % above / below max_offset
        P = np.concatenate([_plane_patch((0.1, 0.1), (0.9, 0.9), 0.5, 40, rng),
                            _plane_patch((1.1, 0.1), (1.9, 0.9), 0.5 + delta, 40, rng)])
        got, _ = _check(_grid([P]), f"parallel planes {delta:.3f} apart", max_offset=mo)
        assert _margins(got, max_offset=mo) > 1e-9
        assert len(got.segments.count) == segments, got.segments.n_leaves
    # perpendicular planes that meet in the voxel edge x = 1, z = 0: never merged, whatever the offset allowed
    P = np.concatenate([_plane_patch((0.0, 0.1), (1.0, 0.9), 0.002, 60, rng, sigma=0.0005),
                        _plane_patch((0.1, 0.0), (0.9, 1.0), 1.002, 60, rng, axis=0, sigma=0.0005)])
    g = _grid([P])
    for args in (dict(max_offset=1.0), dict(max_offset=1.0, max_angle=1.5)):
        got, _ = _check(g, f"perpendicular planes {args}", **args)
        assert _margins(got, **args) > 1e-9
        assert len(got.label) == 2 and got.neighbour[0, 1] == got.planes.node[1] and len(got.segments.count) == 2
    got, _ = _check(g, "perpendicular planes, max_angle = pi / 2", max_offset=1.0, max_angle=math.pi / 2)
    assert len(got.segments.count) == 1
    # max_angle = 0: cos_min is 1.0, only normals whose rounded dot product reaches 1 are joined
    flat = _flat_voxels([(x, y) for x in range(6) for y in range(6)], seed=4)
    got, _ = _check(_grid([flat]), "max_angle = 0, noisy", max_angle=0.0)
    assert len(got.segments.count) > 18
    exact = np.concatenate([_plane_patch((x + 0.1, 0.1), (x + 0.9, 0.9), 0.5, 30, rng) for x in range(4)])
    got, _ = _check(_grid([exact]), "max_angle = 0, exact planes", max_angle=0.0)
    assert np.all(np.abs(got.planes.normal[:, 2]) == 1.0) and got.segments.n_leaves.tolist() == [4]


# ---- 6. cache and stamps ---------------------------------------------------------------------------------------------------
def _abi(f: Forest, cap=(0, 0), outs=None, sel=None, min_points=8, max_variance=-1.0, cos_min=math.cos(0.1),
         max_offset=0.05):
    nr, ns = C.c_int64(-1), C.c_int64(-1)
    ptrs = [nat.ptr(a) for a in outs] if outs else [None] * 9
    rc = f.lib.octl_forest_plane_segments(f.handle, nat.ptr(sel), 0 if sel is None else len(sel), min_points,
                                          max_variance, cos_min, max_offset, cap[0], cap[1], *ptrs, C.byref(nr),
                                          C.byref(ns))
    return rc, nr.value, ns.value


def _abi_tables(f: Forest, **args):
    rc, R, S = _abi(f, **args)
    assert rc == 0
    outs = [np.empty((R, 6), np.int32), np.empty(R, np.int32), np.empty(S, np.int32), np.empty(S, np.int32),
            np.empty(S, np.int64), np.empty((S, 3)), np.empty((S, 6)), np.empty((S, 3)), np.empty((S, 3, 3))]
    assert _abi(f, (R, S), outs, **args) == (0, R, S)
    return outs


def _delta(fn):
    a, b = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
    out = fn()
    return out, (_counter("octl_debug_launches") - a, _counter("octl_debug_host_syncs") - b)


def test_cache_and_stamps():
    P = floor_and_wall()
    g = _grid([P[:9000], P[9000:14000]], MaxPoints(64))
    first, _ = _check(g, "first")
    again, d = _delta(lambda: g.plane_segments())
    assert d[0] == 0, d                                    # (nothing launched: the tables are downloaded again)
    _assert_equal(again, first, "again")
    assert again.segments.mean.tobytes() == first.segments.mean.tobytes()
    other, d = _delta(lambda: g.plane_segments(max_angle=0.05))
    assert d[0] > 0 and not np.array_equal(other.label, first.label)
    _, d = _delta(lambda: g.plane_segments([1]))           # another selection: pooled table and segments again
    assert d[0] > 0
    _check(g, "pose 1", [1])
    _check(g, "all poses again")
    # apply_mask
    np.random.seed(1)
    g.map_leaf_points_cuda_ransac(poses_per_batch=2, threshold=0.01, hypotheses_number=128, initial_points_number=6)
    masked, _ = _check(g, "after RANSAC and apply_mask")
    assert masked.planes.count.sum() < first.planes.count.sum()
    # a late pose
    g.insert_points(2, P[14000:])
    late, _ = _check(g, "after a late pose")
    assert late.planes.count.sum() > masked.planes.count.sum()
    # filter
    g.filter([lambda pts: len(pts) >= 12])
    filtered, _ = _check(g, "after filter")
    assert len(filtered.label) < len(late.label)
    # clear, at the ABI: refused until the forest is built again, then what a fresh forest answers
    f = Forest(0, np.zeros(3), 1.0)
    ref = Forest(0, np.zeros(3), 1.0)
    try:
        f.add_pose(P[:6000])
        f.build(64)
        before = _abi_tables(f)
        f.ctx.check(f.lib.octl_forest_clear(f.handle))
        assert _abi(f)[0] == nat.OCTL_E_STATE
        slot, info = C.c_int32(0), nat.BuildInfo()
        Q = np.ascontiguousarray(P[6000:12000])
        f.ctx.check(f.lib.octl_forest_add_pose(f.handle, nat.ptr(Q), len(Q), C.byref(slot)))
        f.ctx.check(f.lib.octl_forest_build(f.handle, 64, None, 0, 0, 0, C.byref(info)))
        after = _abi_tables(f)
        ref.add_pose(Q)
        ref.build(64)
        want = _abi_tables(ref)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(after, want))
        assert after[1].tobytes() != before[1].tobytes()
        spec = plane_segments_np(ref.leaf_planes(), ref.nodes, ref.voxels, 0, 1.0)
        assert np.array_equal(want[0], spec.neighbour) and np.array_equal(want[1], spec.label)
        assert np.array_equal(want[2], spec.segments.root) and np.array_equal(want[3], spec.segments.n_leaves)
    finally:
        f.close()
        ref.close()


# ---- 7. refusals at the ABI, launch shape -------------------------------------------------------------------------------------
def test_refusals():
    g = _grid([floor_and_wall()[::8]])
    f = g._forest
    assert _abi(f)[0] == nat.OCTL_E_STATE and b"before build" in f.lib.octl_last_error(f.ctx.handle)
    g.subdivide([MaxPoints(64)])
    g.locate(np.zeros((1, 3)))                       # (warm: the voxel codes are on the device)
    launches = _counter("octl_debug_launches")
    for bad in (dict(min_points=0), dict(min_points=-1), dict(cos_min=-0.1), dict(cos_min=1.0000001),
                dict(cos_min=float("nan")), dict(max_offset=-1e-9), dict(max_offset=float("inf")),
                dict(max_offset=float("nan")), dict(max_variance=float("nan")), dict(sel=np.ones(3, np.uint8))):
        assert _abi(f, **bad)[0] == nat.OCTL_E_INVALID, bad
    assert _counter("octl_debug_launches") == launches               # (refused before anything runs)
    for bad in (dict(max_angle=-0.1), dict(max_angle=1.6), dict(max_offset=-1.0), dict(max_offset=float("nan")),
                dict(min_points=0)):
        with pytest.raises(ValueError):
            g.plane_segments(**bad)
    with pytest.raises(KeyError):
        g.plane_segments([5])
    assert _abi(f, cos_min=1.0, max_offset=0.0)[0] == 0 and _abi(f, cos_min=0.0)[0] == 0


def test_launch_shape():
    """Launches and host waits of a first call (no pooled table yet) and of a call on an existing pooled table, at two
    map sizes that differ 10x.  Both scenes have fewer than 256 segments and fewer than 2^13 nodes, so the two radix
    sorts run the same number of passes (the count is a function of those bit widths, never of the device)."""
    P = floor_and_wall()
    per_size = []
    for cloud in (P[::10], P):
        g = _grid([cloud], MaxPoints(64))
        f = g._forest
        f.ensure_built()
        f.locate(cloud[:10])                           # (warm: the voxel codes are on the device)
        f.ctx.sync()
        (rc, R, S), first = _delta(lambda: _abi(f))
        assert rc == 0 and 0 < S < 256 and R > S
        (rc, R2, S2), other = _delta(lambda: _abi(f, cos_min=math.cos(0.2)))
        assert rc == 0 and R2 == R and 0 < S2 < 256
        _, fill = _delta(lambda: _abi_tables(f, cos_min=math.cos(0.2)))
        assert fill == (0, 1), fill                    # (size query and fill: no launch, the download's wait)
        per_size.append((first, other))
        print(len(cloud), R, S, first, other)
    assert per_size[0] == per_size[1], per_size
    assert per_size[0] == (FIRST_CALL, ON_POOLED_TABLE), per_size


# ---- 8. the other queries are untouched ------------------------------------------------------------------------------------
def test_other_queries_untouched():
    P = floor_and_wall()
    clouds = [P[:6000], P[6000:12000], P[12000:]]
    Q = P[::7] + 0.003

    def run(with_segments):
        g = _grid(clouds, MaxPoints(64))
        g._forest.ensure_built()
        g.locate(Q[:1])         # (the voxel codes go to the device with the first query, whichever it is)
        out, counts = [], []
        for step in (lambda: g.leaf_planes(), lambda: g.nearest(Q, 4, max_distance=0.2),
                     lambda: g.adjustment_system(), lambda: g.point_to_plane(Q)):
            res, d = _delta(step)
            out.append(res)
            counts.append(d)
            if with_segments:
                assert len(g.plane_segments().segments.count) > 3
                assert len(g.plane_segments(max_angle=0.05, min_points=12).segments.count) > 3
        return out, counts

    (pl0, nn0, adj0, pp0), c0 = run(False)
    (pl1, nn1, adj1, pp1), c1 = run(True)
    assert c0 == c1, (c0, c1)
    for name in ("node", "count", "mean", "covariance", "eigenvalues", "eigenvectors"):
        assert getattr(pl0, name).tobytes() == getattr(pl1, name).tobytes(), name
    for name in ("pose", "index", "distance2", "count"):
        assert getattr(nn0, name).tobytes() == getattr(nn1, name).tobytes(), name
    for name in ("H", "g", "cost", "n_points", "n_blocks"):
        assert getattr(adj0, name).tobytes() == getattr(adj1, name).tobytes(), name
    for name in ("node", "row", "distance"):
        assert getattr(pp0, name).tobytes() == getattr(pp1, name).tobytes(), name


# ---- allocation failures of a first call ---------------------------------------------------------------------------------------
def test_allocation_failures_of_a_first_call():
    """Every growth of a device buffer that a first plane_segments call makes fails once (octl_debug_fail_alloc, the
    convention of tests/test_gpu_failures.py): the call raises MemoryError and, asked again, answers as undisturbed."""
    P = floor_and_wall()[::4]

    def arm(nth):
        seen = C.c_int64(0)
        nat.get_context().check(nat.load().octl_debug_fail_alloc(int(nth), C.byref(seen)))

    def fresh():
        g = _grid([P], MaxPoints(64))
        g._forest.ensure_built()
        return g

    want = fresh().plane_segments()
    hits, nth = 0, 1
    while True:
        g = fresh()
        arm(nth)
        raised = False
        try:
            g.plane_segments()
        except MemoryError as e:
            raised = True
            assert "injected by octl_debug_fail_alloc" in str(e)
        finally:
            arm(0)
        if not raised:
            break
        hits += 1
        got = g.plane_segments()
        _assert_equal(got, want, f"after a failed growth {nth}")
        assert got.segments.covariance.tobytes() == want.segments.covariance.tobytes()
        nth += 1
        assert nth < 30
    print(f"{hits} growths failed once")
    assert hits >= 1, hits
