"""prune() on the device (octl_forest_prune) against its definition octreelib_amd.query.prune_np: the
tables after equal the definition applied to the tables before, column for column and bit for bit; what a pose reads
back and what the map queries answer do not change except for node ids, which go through PruneResult.node_map; the
map goes on working (RANSAC, late poses, subdivide, carve, remove_poses, prune again); launches and host waits do not
depend on the size; an allocation failure changes nothing; refusals.

The scenes: three or four poses of 300 - 2000 points over a 3 x 3 x 2 block of 1 m voxels, MaxPoints(8): depth >= 3.
Holes are made the ways users make them: remove_poses of a pose that alone populated two voxels and some sub-leaves,
carve, RANSAC + apply_mask and a count filter."""

import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from octreelib_amd import MaxPoints, PruneResult, RayEvidence, plane_segments_np, prune_np, synthetic
from octreelib_amd import _native as nat
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree_manager import OctreeManager
from octreelib_amd.query import evidence_inputs
from oracle import octree_np as onp
from tests._evidence import assert_evidence_equal, evidence_of_nodes
from tests._util import assert_same_leaves, canon, canon_from_list
from tests.test_gpu_remove_poses import _arm, _deltas, _leaf_points, _same_bits, _table, _try

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_scan = open(os.path.join(ROOT, "octreelib_amd", "csrc", "scan.hip")).read()
SCAN_TILE = (int(re.search(r"constexpr int SCAN_THREADS = (\d+);", _scan).group(1))
             * int(re.search(r"constexpr int SCAN_IPT = (\d+);", _scan).group(1)))
assert SCAN_TILE == 2048
# (launches, host waits) of the raw entry without downloads - one fill, mark, flags, scan | the wait |
# node pass, block pass - and of a call that finds nothing to do (it ends behind the wait)
SHAPE_WORKING = (6, 1)
SHAPE_NOOP = (4, 1)
DIMS = (3, 3, 2)
K = 8
COUNT = [MaxPoints(K)]
TABLE = np.random.default_rng(9).random((128, 6))
THRESHOLD = 0.02
NODE_COLS = ("voxel", "depth", "parent", "first_child", "corner", "edge", "epoch")
BLOCK_COLS = ("node", "slot", "start", "size")


# ---- scenes --------------------------------------------------------------------------------------------------------
def _grid():
    return Grid(GridConfig(voxel_edge_length=1))


def _clouds(n=3300, seed=5):
    """Poses 0, 1: the scene without the voxels (2, 2, *); pose 2: those two voxels alone, and a tight cluster in a
    corner of voxel (0, 0, 0) where the planes of poses 0 and 1 do not pass."""
    base = synthetic.planar_cloud(n, DIMS, seed=seed)
    lonely = (np.floor(base[:, 0]) == 2) & (np.floor(base[:, 1]) == 2)
    rest = base[~lonely]
    a = len(rest) * 11 // 20
    cluster = 0.93 + 0.06 * np.random.default_rng(seed + 1).random((40, 3))
    return [rest[:a], rest[a:], np.ascontiguousarray(np.vstack([base[lonely], cluster]))]


RAYS_O = np.tile(np.array([[-0.5, 0.31, 0.27], [-0.5, 1.43, 0.77], [-0.5, 2.19, 1.35], [1.21, -0.5, 0.55]]), (60, 1))
_rng = np.random.default_rng(2)
RAYS_D = np.where(np.arange(240)[:, None] % 4 == 3, [0.02, 1.0, 0.01], [1.0, 0.03, 0.02]) + 0.05 * _rng.normal(size=(240, 3))
RAYS_R = _rng.uniform(1.0, 3.4, 240)
QUERIES = synthetic.planar_cloud(600, DIMS, seed=5, stream=3) + 0.004
ORIGIN = np.array([1.5, 1.5, 1.0])    # (adjustment_system's default origin is the centre of the voxels that exist)


def _holes(g, how):
    if "remove" in how:
        g.remove_poses([2])
    if "carve" in how:
        g.carve(g.ray_evidence(RAYS_O, RAYS_D, RAYS_R, 0.05), 1, 0)
    if "ransac" in how:
        g.map_leaf_points_cuda_ransac(poses_per_batch=2, threshold=THRESHOLD, hypotheses=TABLE)
        g.filter([lambda pts: len(pts) >= 4])


def _scene(how=("remove", "carve", "ransac"), clouds=None):
    g = _grid()
    for p, X in enumerate(_clouds() if clouds is None else clouds):
        g.insert_points(p, X)
    g.subdivide(COUNT)
    _holes(g, how)
    return g


def _tables(f):
    f._invalidate()
    return ({k: f.nodes[k].copy() for k in NODE_COLS}, f.voxels.copy(), {k: f.blocks[k].copy() for k in BLOCK_COLS},
            f.perm.copy(), f.xyz.copy())


def _flat(tables):
    """The tables of _tables as one list of arrays (what _same_bits compares)."""
    nodes, voxels, blocks, perm, xyz = tables
    return [nodes[k] for k in NODE_COLS] + [voxels] + [blocks[k] for k in BLOCK_COLS] + [perm, xyz]


def _prune_and_check(obj, what, expect_change=True):
    """prune() against prune_np of the tables downloaded before; returns (PruneResult, tables before, tables after)."""
    f = obj._forest
    before = _tables(f)
    nodes, voxels, blocks, perm, xyz = before
    res = obj.prune()
    assert isinstance(res, PruneResult), what
    want = prune_np(nodes, blocks, f.mode)
    after = _tables(f)
    for k in NODE_COLS:
        _same_bits(after[0][k], want.nodes[k], f"{what}: nodes.{k}")
    _same_bits(after[1], voxels[want.voxel_keep], f"{what}: voxels")
    for k in BLOCK_COLS:
        _same_bits(after[2][k], want.blocks[k], f"{what}: blocks.{k}")
    _same_bits(after[3], perm, f"{what}: perm")
    _same_bits(after[4], xyz, f"{what}: ordered points")
    _same_bits(res.node_map, want.node_map, f"{what}: node_map")
    _same_bits(res.old_node, want.old_node, f"{what}: old_node")
    N, N2, V, V2 = len(nodes["edge"]), len(want.old_node), len(voxels), int(np.count_nonzero(want.voxel_keep))
    assert (res.n_nodes, res.n_voxels, res.nodes_dropped, res.voxels_dropped, res.collapsed) == \
        (N2, V2, N - N2, V - V2, want.collapsed), what
    assert f.n_scheme_nodes() == N2 and len(f.internal_per_voxel()) == V2, what
    assert int(f.internal_per_voxel().sum()) == int(np.count_nonzero(want.nodes["first_child"] >= 0)), what
    if expect_change:
        assert N2 < N, what
    return res, before, after


# ---- 1. the tables equal the definition -----------------------------------------------------------------------------
def test_tables_equal_the_definition():
    g = _scene()
    assert g._forest.nodes["depth"].max() >= 3
    res, before, _ = _prune_and_check(g, "the scene")
    assert res.voxels_dropped >= 2 and res.collapsed > 0
    # the all-empty grid: no voxel, no node - and a map that takes a pose again
    g.remove_poses([0, 1])
    res, _, after = _prune_and_check(g, "the empty grid")
    assert res.n_nodes == 0 and res.n_voxels == 0 and len(after[1]) == 0
    late = synthetic.planar_cloud(300, DIMS, seed=5, stream=8)
    g.insert_points(7, late)
    assert sorted(map(tuple, g.get_points(7).tolist())) == sorted(map(tuple, late.tolist()))
    g.subdivide(COUNT)
    assert g.n_points(7) == 300 and g._forest.nodes["depth"].max() >= 1


def test_tables_roots_across_workgroups():
    """7 x 7 x 6 = 294 voxels with a point or two each, half of them emptied: the roots span two workgroups."""
    V = 7 * 7 * 6
    lin = np.arange(V)
    q = np.stack([lin // 42, (lin // 6) % 7, lin % 6], axis=1)
    rng = np.random.default_rng(4)
    one = q + 0.1 + 0.8 * rng.random((V, 3))                       # one point in every voxel ...
    two = q[::3] + 0.1 + 0.8 * rng.random((len(q[::3]), 3))        # ... a second one in every third
    g = _grid()
    g.insert_points(0, np.vstack([one[::2], two[::2]]))
    g.insert_points(1, np.vstack([one[1::2], two[1::2]]))
    g.subdivide([MaxPoints(1)])
    assert len(g._forest.voxels) == V
    g.remove_poses([1])
    res, _, _ = _prune_and_check(g, "294 voxels")
    assert res.voxels_dropped > 100 and res.n_voxels > 100


def test_tables_more_nodes_than_a_scan_tile_and_a_deep_cluster():
    rng = np.random.default_rng(6)
    big = synthetic.planar_cloud(12000, DIMS, seed=5, stream=2)
    cluster = np.array([1.3, 1.6, 0.7]) + 0.015 * rng.random((300, 3))       # depth >= 6 under MaxPoints(8)
    g = _grid()
    g.insert_points(0, big[:6000])
    g.insert_points(1, np.vstack([big[6000:], cluster]))
    g.insert_points(2, _clouds()[2])
    g.subdivide(COUNT)
    f = g._forest
    assert f.n_scheme_nodes() > 2 * SCAN_TILE and f.nodes["depth"].max() >= 6
    g.remove_poses([1])
    g.carve(g.ray_evidence(RAYS_O, RAYS_D, RAYS_R, 0.05), 1, 0)
    res, _, after = _prune_and_check(g, "large table")
    assert res.n_nodes > SCAN_TILE and res.collapsed > 0


def test_tables_two_epochs_and_late_voxels():
    """subdivide, a late pose elsewhere, subdivide again: two level ranges per depth, more than one epoch."""
    c = _clouds()
    g = _grid()
    g.insert_points(0, c[0])
    g.insert_points(1, c[1])
    g.subdivide([MaxPoints(24)], pose_numbers=[0])
    far = synthetic.planar_cloud(900, (5, 3, 2), seed=8, box=((3, 0, 0), (5, 3, 2)))
    g.insert_points(2, np.vstack([far, c[2]]))
    assert g.n_points(2) == len(far) + len(c[2])
    g.subdivide(COUNT)
    f = g._forest
    assert len(np.unique(f.nodes["epoch"][f.nodes["first_child"] >= 0])) >= 2
    g.remove_poses([2])
    g.map_leaf_points_cuda_ransac(poses_per_batch=2, threshold=THRESHOLD, hypotheses=TABLE)
    res, _, _ = _prune_and_check(g, "two epochs")
    assert res.voxels_dropped >= 8


def test_tables_single_cube_all_empty_and_not():
    c = np.vstack(_clouds()) / 3.0
    m = OctreeManager(Octree, OctreeConfig(), np.array([0.0, 0.0, 0.0]), 1.0)
    m.insert_points(0, c[:1500])
    m.insert_points(1, c[1500:])
    m.subdivide(COUNT)
    m.remove_poses([1])
    res, _, _ = _prune_and_check(m, "manager")
    assert res.n_voxels == 1 and res.voxels_dropped == 0
    m.remove_poses([0])
    res, _, after = _prune_and_check(m, "empty manager")
    assert res.n_nodes == 1 and res.collapsed == 1 and after[0]["first_child"][0] == -1 and after[0]["epoch"][0] == 0
    o = Octree(OctreeConfig(), np.array([0.0, 0.0, 0.0]), 1.0)
    o.insert_points(c[:800])
    o.subdivide(COUNT)
    o.filter([lambda pts: len(pts) >= 6])
    _prune_and_check(o, "octree")


# ---- 2. reads are invariant -----------------------------------------------------------------------------------------
def _leaf_keys(nodes):
    return {(nodes["corner"][i].tobytes(), nodes["edge"][i].tobytes()) for i in np.nonzero(nodes["first_child"] < 0)[0]}


def _reads_equal(P, T, poses, what):
    """P: the pruned map, T: its untouched twin (the same operations, no prune)."""
    fp = P._forest
    fp._invalidate()
    T._forest._invalidate()
    new = fp.nodes
    leaves_p, leaves_t = _leaf_keys(new), _leaf_keys(T._forest.nodes)
    key = lambda v: (np.asarray(v.corner_min, dtype=np.float64).tobytes(), np.float64(v.edge_length).tobytes())
    for p in poses:
        for count in ("n_points", "n_leaves"):
            assert getattr(P, count)(p) == getattr(T, count)(p), (what, count, p)
        _same_bits(P.get_points(p), T.get_points(p), f"{what}: get_points({p})")
        la, lb = P.get_leaf_points(p), T.get_leaf_points(p)
        assert_same_leaves(_table(la), _table(lb))
        _same_bits(_leaf_points(la), _leaf_points(lb), f"{what}: leaf points of pose {p}")
        _same_bits(_try(lambda: P.leaf_statistics(p)), _try(lambda: T.leaf_statistics(p)), f"{what}: leaf_statistics({p})")
        fa, fb = P.get_leaf_points(p, False), T.get_leaf_points(p, False)
        # the twin's listing with the vanished empty leaves deleted; a node that collapsed - internal in the twin -
        # lists as the one empty leaf it is now
        kept = [(key(v), v.n_points) for v in fb if key(v) in leaves_p]
        assert all(v.n_points == 0 for v in fb if key(v) not in leaves_p), (what, p)
        got = [(key(v), v.n_points) for v in fa if key(v) in leaves_t]
        assert all(v.n_points == 0 for v in fa if key(v) not in leaves_t), (what, p)
        assert got == kept, (what, p)
        _same_bits(_leaf_points(fa), _leaf_points(fb), f"{what}: all leaf points of pose {p}")
        in_pose = np.isin(new["voxel"], fp.slot_voxel_ranks(P._slots[p]))
        assert P.n_nodes(p) == int(in_pose.sum()) == len(fa) + int((in_pose & (new["first_child"] >= 0)).sum()), (what, p)


def test_reads_are_invariant():
    P, T = _scene(), _scene()
    res = P.prune()
    assert res.nodes_dropped > 0 and res.collapsed > 0
    _reads_equal(P, T, [0, 1], "scene")


# ---- 3. queries are invariant through the map -------------------------------------------------------------------------
def _mapped(node, node_map):
    return np.where(node >= 0, node_map[np.maximum(node, 0)], -1).astype(np.int32)


def _through(x, node_map):
    """The answer x with every node id it names sent through the map."""
    x = dataclasses.replace(x, node=_mapped(x.node, node_map))
    return dataclasses.replace(x, planes=_through(x.planes, node_map)) if hasattr(x, "planes") else x


# the queries and rays of _queries: this module's scene (a map of another extent passes its own)
SCENE = {"queries": QUERIES, "origins": RAYS_O, "directions": RAYS_D, "ranges": RAYS_R, "margin": 0.05, "max_range": 6.0,
         "radius": 0.3, "max_variance": 1e-2, "origin": ORIGIN}


def _queries(g, scene=SCENE):
    """Every map query as ("answer", x), or ("raises", kind) where the map refuses it (both must agree).  g: a Grid,
    an OctreeManager or an Octree (which takes no pose selection and has no adjustment: that one refuses, both times)."""
    sel = () if isinstance(g, Octree) else (None,)
    Q, O, D, R, mv = (scene[k] for k in ("queries", "origins", "directions", "ranges", "max_variance"))
    return {
        "locate": _try(lambda: g.locate(Q)),
        "planes": _try(lambda: g.leaf_planes()),
        "p2p": _try(lambda: g.point_to_plane(Q, *sel, 8, mv)),
        "ray_cube": _try(lambda: g.raycast(O, D, scene["max_range"])),
        "ray_plane": _try(lambda: g.raycast(O, D, scene["max_range"], surface="plane", max_variance=mv)),
        "nearest": _try(lambda: g.nearest(Q, 4, max_distance=scene["radius"])),
        "registration": _try(lambda: g.registration_system(Q, None, *sel, max_variance=mv)),
        "adjustment": _try(lambda: g.adjustment_system(None, None, origin=scene["origin"], max_variance=mv)),
        "segments": _try(lambda: g.plane_segments(*sel, max_variance=mv)),
        "evidence": _try(lambda: g.ray_evidence(O, D, R, scene["margin"])),
    }


def _queries_equal(a, b, res, nodes_before, g, what, scene=SCENE):
    """a: before (or the unpruned twin), b: after, on the map g; scene: what _queries was given."""
    m = res.node_map
    for name in a:
        assert a[name][0] == b[name][0] and (a[name][0] == "answer" or a[name][1] == b[name][1]), (what, name, a[name])
    for name in ("locate", "planes", "evidence"):
        assert a[name][0] == "answer", (what, name, a[name])
    refused = {name for name in a if a[name][0] != "answer"}
    a, b = ({k: v[1] for k, v in d.items()} for d in (a, b))
    _same_bits(b["locate"], _mapped(a["locate"], m), f"{what}: locate")
    for name in {"planes", "p2p", "ray_cube", "ray_plane"} - refused:
        _same_bits(b[name], _through(a[name], m), f"{what}: {name}")
    for name in {"nearest", "adjustment"} - refused:
        _same_bits(b[name], a[name], f"{what}: {name}")
    if "registration" not in refused:
        for fld in ("H", "g", "cost", "n_used", "origin"):
            _same_bits(getattr(b["registration"], fld), getattr(a["registration"], fld), f"{what}: registration.{fld}")
        # (n_located counts the scan points that fall into any leaf: those in a dropped voxel no longer do)
        assert b["registration"].n_located <= a["registration"].n_located, what
    f = g._forest
    if "segments" not in refused:
        _same_bits(b["segments"].label, a["segments"].label, f"{what}: segments.label")
        table = a["segments"].segments
        table = dataclasses.replace(table, root=_mapped(table.root, m))        # (a segment's root leaf is a node id)
        _same_bits(b["segments"].segments, table, f"{what}: segments.segments")
        spec = plane_segments_np(b["planes"], f.nodes, f.voxels, f.mode, f._cube[1], max_variance=scene["max_variance"])
        _same_bits(b["segments"].neighbour, spec.neighbour, f"{what}: segments.neighbour")
    inp = evidence_inputs(scene["origins"], scene["directions"], scene["ranges"], scene["margin"])
    assert_evidence_equal(b["evidence"], evidence_of_nodes(f.nodes, *inp), f"{what}: ray_evidence")
    carried = a["evidence"].remapped(res)
    same = (nodes_before["first_child"][res.old_node] >= 0) == (f.nodes["first_child"] >= 0)      # (not collapsed)
    assert np.array_equal(b["evidence"].through[same], carried.through[same]), what
    assert np.array_equal(b["evidence"].hits[same], carried.hits[same]), what
    assert not carried.through[~same].any() and not carried.hits[~same].any(), what


def test_queries_are_invariant_through_the_map():
    g = _scene()
    f = g._forest
    nodes_before = {k: v.copy() for k, v in f.nodes.items()}
    before = _queries(g)
    assert all(v[0] == "answer" for v in before.values()), before
    assert (before["locate"][1] >= 0).sum() > 100 and (before["ray_cube"][1].node >= 0).sum() > 20
    res = g.prune()
    assert res.collapsed > 0 and res.voxels_dropped >= 2
    _queries_equal(before, _queries(g), res, nodes_before, g, "scene")
    again = g.prune()
    assert len(again.node_map) == res.n_nodes < len(before["evidence"][1])
    with pytest.raises(ValueError, match="evidence over"):
        before["evidence"][1].remapped(again)


# ---- 4. the map goes on working ---------------------------------------------------------------------------------------
def _oracle_leaves(g, poses, Kc):
    """The NumPy oracle of a fresh subdivide over the points the map holds now: canon leaf table per pose."""
    og = onp.OGrid(1)
    clouds = {p: g.get_points(p) for p in poses}
    for p in poses:
        og.insert_points(p, clouds[p])
    og.subdivide(Kc)
    return {p: canon_from_list(og.leaf_table(p)) for p in poses}, clouds


def _leaves_by_index(g, p, cloud):
    index = {row.tobytes(): i for i, row in enumerate(cloud)}
    lv = g.get_leaf_points(p)
    return canon([np.asarray(v.corner_min, dtype=np.float64) for v in lv], [v.edge_length for v in lv],
                 [v.n_points for v in lv], np.array([index[r.tobytes()] for v in lv for r in v.get_points()], dtype=np.int64))


def test_the_map_goes_on_working():
    P, T = _scene(("remove", "carve")), _scene(("remove", "carve"))
    fp = P._forest
    res = P.prune()
    assert res.voxels_dropped >= 2 and res.collapsed > 0
    # a second prune straight after the first: nothing to do, no table written (the pooled planes stay valid)
    P.leaf_planes()
    size_query = lambda: fp.ctx.check(fp.lib.octl_forest_pooled_leaf_stats(fp.handle, None, 0, 0, None, None, None, None,
                                                                           None, None, C.byref(C.c_int64(0))))
    assert _deltas(size_query)[0] == 0
    again = P.prune()
    assert (again.nodes_dropped, again.voxels_dropped, again.collapsed) == (0, 0, 0)
    assert np.array_equal(again.node_map, np.arange(res.n_nodes)) and np.array_equal(again.old_node, again.node_map)
    assert _deltas(size_query)[0] == 0, "a prune that finds nothing moved the content stamp"
    # RANSAC on the pruned map: the twin's masks and planes (level ranges, reference order)
    for g in (P, T):
        g._forest.ensure_built()
    order_p, order_t = fp.order.copy(), T._forest.order.copy()
    out_p = fp.ransac_blocks(order_p, TABLE, THRESHOLD, details=True)
    out_t = T._forest.ransac_blocks(order_t, TABLE, THRESHOLD, details=True)
    _same_bits(out_p, out_t, "ransac planes / counts / indices")
    _same_bits(fp.device_mask(), T._forest.device_mask(), "ransac mask")
    _same_bits(fp.blocks["start"][order_p], T._forest.blocks["start"][order_t], "reference order")
    for g in (P, T):
        g.map_leaf_points_cuda_ransac(poses_per_batch=2, threshold=THRESHOLD, hypotheses=TABLE)
    _reads_equal(P, T, [0, 1], "after RANSAC")
    # a late pose partly in kept voxels, partly in the dropped ones
    late = synthetic.planar_cloud(700, DIMS, seed=5, stream=9, box=((1, 1, 0), (3, 3, 2)))
    assert ((np.floor(late[:, 0]) == 2) & (np.floor(late[:, 1]) == 2)).sum() > 50
    for g in (P, T):
        g.insert_points(5, late)
        assert g.n_points(5) == 700
    vp, vt = set(map(tuple, fp.voxels.tolist())), set(map(tuple, T._forest.voxels.tolist()))
    assert len(vt) == 18 and vp <= vt and {(2, 2, 0), (2, 2, 1)} <= vp     # (the dropped voxels are back)
    for g in (P, T):
        g.subdivide(COUNT)
    want, clouds = _oracle_leaves(T, [0, 1, 5], K)
    for p in (0, 1, 5):
        _same_bits(np.sort(P.get_points(p), axis=0), np.sort(T.get_points(p), axis=0), f"points of pose {p}")
        a, b = _leaves_by_index(P, p, clouds[p]), _leaves_by_index(T, p, clouds[p])
        assert_same_leaves(a, b, ordered=False)
        assert_same_leaves(a, want[p], ordered=False)
    # carve with remapped-plus-fresh evidence, remove_poses, prune again
    g2 = _scene(("remove",))
    ev0 = g2.ray_evidence(RAYS_O, RAYS_D, RAYS_R, 0.05)
    r2 = g2.prune()
    ev = ev0.remapped(r2) + g2.ray_evidence(RAYS_O[::2], RAYS_D[::2], RAYS_R[::2], 0.05)
    assert isinstance(ev, RayEvidence) and len(ev) == r2.n_nodes
    assert g2.carve(ev, 2, 0) > 0
    with pytest.raises(ValueError, match="evidence over"):
        g2.carve(ev0, 2, 0)
    g2.remove_poses([1])
    r3, _, _ = _prune_and_check(g2, "pruned, carved, a pose removed, pruned again")
    assert r3.nodes_dropped > 0 and g2.n_points(0) > 0


# ---- 5. shape of the call ---------------------------------------------------------------------------------------------
def _raw(f):
    pi = nat.PruneInfo()
    code = f.lib.octl_forest_prune(f.handle, 0, None, None, C.byref(pi))
    return code, pi


def test_launch_shape_does_not_depend_on_the_size():
    seen, noop = [], []
    for n in (3300, 20000):
        g = _scene(("remove", "carve"), _clouds(n))
        f = g._forest
        f.ensure_built()
        f._resolve_membership()
        assert len(f.voxels) == 18                         # (also: the voxel keys are where the call wants them)
        warm = _scene(("remove",), _clouds(n))             # (the first call on a context may grow its scan buffers)
        warm.prune()
        f.ctx.sync()
        seen.append(_deltas(lambda: f.ctx.check(_raw(f)[0])))
        noop.append(_deltas(lambda: f.ctx.check(_raw(f)[0])))
        f._invalidate()
        assert g.n_points(0) > 0 and len(f.voxels) <= 16
    assert seen == [SHAPE_WORKING] * 2, seen
    assert noop == [SHAPE_NOOP] * 2, noop
    assert SHAPE_NOOP[0] <= SHAPE_WORKING[0] - 2 and SHAPE_NOOP[1] == 1


# ---- 6. atomic on failure -----------------------------------------------------------------------------------------------
def _state(g):
    f = g._forest
    tabs = _flat(_tables(f))
    return [tabs, f.device_mask(), [g.get_points(p) for p in sorted(g._slots)],
            [[v.n_points for v in g.get_leaf_points(p, False)] for p in sorted(g._slots)], g.locate(QUERIES)]


def test_failure_is_atomic():
    """octl_debug_fail_alloc swept over every growth the call makes, each on a map of its own whose prune buffers have
    never been asked for.  After a failure the map reads as before, and the retried call equals the definition."""
    hits, raised = 0, True
    for nth in range(1, 30):
        g = _scene(("remove", "carve"))
        f = g._forest
        f.ensure_built()
        before = _state(g)
        _arm(nth)
        raised = False
        try:
            g.prune()
        except MemoryError as e:
            raised = True
            assert "injected by octl_debug_fail_alloc" in str(e)
        finally:
            _arm(0)
        if raised:
            hits += 1
            _same_bits(_state(g), before, f"after growth {nth} failed")
            res, _, _ = _prune_and_check(g, f"retried after growth {nth}")
            assert res.voxels_dropped >= 2
        f.close()
        if not raised:
            break
    assert not raised and hits >= 2, hits


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    g = _scene(("remove",))
    f = g._forest
    N = f.n_scheme_nodes()
    # an unplaced late pose: the raw entry refuses, the method brings the map up to date first
    g.insert_points(6, synthetic.planar_cloud(200, DIMS, seed=5, stream=11))
    code, _ = _raw(f)
    assert code == nat.OCTL_E_STATE
    res = g.prune()
    assert res.nodes_dropped > 0 and g.n_points(6) == 200
    # cap_nodes too small, before anything changes
    g2 = _scene(("remove",))
    f2 = g2._forest
    f2.ensure_built()
    tabs = _tables(f2)
    small = np.empty(N - 1, dtype=np.int32)
    pi = nat.PruneInfo()
    assert f2.lib.octl_forest_prune(f2.handle, N - 1, nat.ptr(small), None, C.byref(pi)) == nat.OCTL_E_INVALID
    assert f2.lib.octl_forest_prune(f2.handle, N - 1, None, nat.ptr(small), C.byref(pi)) == nat.OCTL_E_INVALID
    assert f2.lib.octl_forest_prune(None, 0, None, None, None) == nat.OCTL_E_INVALID
    _same_bits(_flat(_tables(f2)), _flat(tabs), "after the refusals")
    # plug types
    from tests.test_cpu_registration import _plug_grid
    with pytest.raises(ValueError, match="plug types"):
        _plug_grid({0: _clouds()[0][:50]}).prune()
    # an unbuilt map: zeros, no launch
    h = _grid()
    h.insert_points(0, _clouds()[0])
    fh = h._forest
    shape = _deltas(lambda: fh.ctx.check(_raw(fh)[0]))
    assert shape == (0, 0)
    r = h.prune()
    assert (r.n_nodes, r.n_voxels, r.nodes_dropped, r.voxels_dropped, r.collapsed) == (0, 0, 0, 0, 0)
    assert len(r.node_map) == 0 and len(r.old_node) == 0 and fh.info is None
    assert h.n_points(0) == len(_clouds()[0])
