"""CPU-only checks of the map queries (octreelib_amd/query.py): locate_np against trees built by the oracle,
pooled_leaf_statistics_np / point_to_plane_np against exact arithmetic, the plug path (the caller's own octree
types) end to end on the host, and the five new C entries in the header and _native.py's signature table."""

import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from octreelib_amd import MaxPoints
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.internal.voxel import Voxel
from octreelib_amd.octree.octree_base import OctreeBase, OctreeConfigBase
from octreelib_amd.octree_manager import OctreeManager
from octreelib_amd.query import (HostMap, LeafPlanes, locate_np, node_table_from_leaves, point_to_plane_np,
                                 pooled_leaf_statistics_np)
from oracle.octree_np import OGrid, OTree, tree_leaf_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
_UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))

ENTRIES = {
    "octl_forest_pooled_leaf_stats":
        "int octl_forest_pooled_leaf_stats(octl_forest* f, const uint8_t* slot_sel, int32_t n_sel, int64_t cap, "
        "int32_t* node, int64_t* count, double* mean, double* cov6, double* eigval, double* eigvec, "
        "int64_t* n_leaves)",
    "octl_forest_locate": "int octl_forest_locate(octl_forest* f, const double* xyz, int64_t n, int32_t* node)",
    "octl_forest_locate_device":
        "int octl_forest_locate_device(octl_forest* f, const double* xyz_dev, int64_t n, int32_t* node_dev)",
    "octl_forest_point_to_plane":
        "int octl_forest_point_to_plane(octl_forest* f, const double* xyz, int64_t n, int32_t min_points, "
        "double max_variance, int32_t* node, int32_t* row, double* distance)",
    "octl_forest_point_to_plane_device":
        "int octl_forest_point_to_plane_device(octl_forest* f, const double* xyz_dev, int64_t n, int32_t min_points, "
        "double max_variance, int32_t* node_dev, int32_t* row_dev, double* distance_dev)",
}


class _Leaf:
    def __init__(self, corner, edge, points):
        self.corner_min, self.edge_length, self._p = corner, edge, points

    def get_points(self):
        return self._p


def _grid_map(og: OGrid, L):
    """HostMap over an oracle grid: roots in voxel order, every pose's leaves (empty ones too)."""
    roots = [(np.array(k, dtype=np.float64), float(L)) for k in sorted(og.managers)]
    leaves = {p: [_Leaf(c, e, og.pose_points[p][i]) for c, e, i in og.leaf_table(p, False)] for p in og.pose_voxels}
    return HostMap(0, float(L), roots, leaves)


def _depths(nodes):
    fc = nodes["first_child"]
    d = np.zeros(len(fc), dtype=int)
    for i in np.nonzero(fc >= 0)[0]:      # (children are numbered behind their parents)
        d[fc[i]:fc[i] + 8] = d[i] + 1
    return d


# ---- locate_np against the oracle ------------------------------------------------------------------------------------
def test_locate_grid_multi_pose_every_stored_point():
    rng = np.random.default_rng(1)
    A = rng.uniform(-3.0, 3.0, (5000, 3))          # negative coordinates included
    B = rng.uniform(-1.0, 4.0, (3000, 3))
    og = OGrid(2)
    og.insert_points(0, A)
    og.insert_points(1, B)
    og.subdivide(5, [0])                           # scheme from a pose subset
    hm = _grid_map(og, 2)
    seen = 0
    for p in (0, 1):
        for v in hm._leaves[p]:
            pts = v.get_points()
            if len(pts):
                assert np.all(hm.locate(pts) == hm._id(v))
                seen += len(pts)
    assert seen == len(A) + len(B)
    assert _depths(hm.nodes).max() >= 3


def test_locate_single_cube():
    rng = np.random.default_rng(2)
    P = rng.uniform(-1.0, 1.0, (3000, 3)) * [1.0, 1.0, 0.05]
    t = OTree(np.array([-1.0, -1.0, -1.0]), 2.0)
    t.insert_points(P)
    t.subdivide(25)
    table = tree_leaf_table(t, False)
    nodes, ids = node_table_from_leaves([(np.array([-1.0, -1.0, -1.0]), 2.0)], [(c, e) for c, e, _ in table])
    vox = np.array([[-1, -1, -1]])
    for c, e, idx in table:
        if len(idx):
            assert np.all(locate_np(nodes, vox, 1, 2.0, P[idx]) == ids[(tuple(c.tolist()), float(e))])
    out = np.array([[1.0, 0.0, 0.0], [0.0, -1.5, 0.0], [np.nan, 0.0, 0.0], [0.0, 0.0, np.inf], [-1.0, -1.0, -1.0]])
    got = locate_np(nodes, vox, 1, 2.0, out)
    assert got[:4].tolist() == [-1, -1, -1, -1] and got[4] >= 0      # (the cube is half open: its corner is inside)
    # an unsubdivided cube answers with its root
    nodes0, _ = node_table_from_leaves([(np.zeros(3), 1.0)], [(np.zeros(3), 1.0)])
    assert locate_np(nodes0, np.zeros((1, 3), dtype=int), 1, 1.0, [[0.5, 0.5, 0.5], [1.5, 0, 0]]).tolist() == [0, -1]


def test_locate_boundaries_and_out_of_domain():
    rng = np.random.default_rng(3)
    P = np.concatenate([rng.uniform(0.0, 2.0, (4000, 3)), rng.uniform(-2.0, 0.0, (500, 3))])
    og = OGrid(1)
    og.insert_points(0, P)
    og.subdivide(4)
    hm = _grid_map(og, 1)
    nd = hm.nodes
    depth = _depths(nd)
    internal = np.nonzero(nd["first_child"] >= 0)[0]
    assert depth[internal].max() >= 2
    # the centre of every split node lies on its three splitting planes; so do the face centres of its children
    centres = nd["corner"][internal] + (nd["edge"][internal] / 2.0)[:, None]
    Q = np.concatenate([centres, centres + nd["edge"][internal][:, None] * [0.25, 0.0, 0.0],
                        nd["corner"][internal]])
    # the test really holds points ON a splitting plane at every depth of the tree
    for d in range(int(depth[internal].max()) + 1):
        sel = internal[depth[internal] == d]
        planes = (nd["corner"][sel] + (nd["edge"][sel] / 2.0)[:, None])
        assert len(sel) and any(np.any(Q[:, a][:, None] == planes[:, a][None, :]) for a in range(3)), d
    got = hm.locate(Q)
    assert np.all(got >= 0)
    # documented answer: the half-open cube [corner, corner + edge) that holds the point - exact for these dyadic,
    # non-negative or small coordinates - and a leaf
    assert np.all(nd["first_child"][got] < 0)
    for q, n in zip(Q, got):
        c, e = nd["corner"][n], nd["edge"][n]
        assert all(Fraction(c[a]) <= Fraction(q[a]) < Fraction(c[a]) + Fraction(e) for a in range(3))
    # voxel faces, negative coordinates, -0.0
    faces = np.array([[1.0, 0.5, 0.5], [-1.0, -0.5, -0.5], [-0.0, 0.5, 0.5], [0.5, 2.0 - 2.0 ** -52, 0.5]])
    for q, n in zip(faces, hm.locate(faces)):
        assert n >= 0
        root = n
        while root >= len(hm.voxels):
            root = int(np.nonzero((nd["first_child"] <= root) & (nd["first_child"] + 8 > root))[0][0])
        assert hm.voxels[root].tolist() == np.floor(q + 0.0).astype(int).tolist()
    # outside every voxel, outside the domain, not finite: -1, no exception
    bad = np.array([[2.5, 0.5, 0.5], [0.5, 0.5, -2.5], [1e300, 0.0, 0.0], [0.0, -2.0 ** 31, 0.0],
                    [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf]])
    assert hm.locate(bad).tolist() == [-1] * len(bad)


def test_locate_input_forms():
    nodes, _ = node_table_from_leaves([(np.zeros(3), 1.0)], [(np.zeros(3), 1.0)])
    vox = np.zeros((1, 3), dtype=int)
    P = np.random.default_rng(0).random((50, 3)).astype(np.float32)
    ref = locate_np(nodes, vox, 0, 1.0, P.astype(np.float64))
    assert np.array_equal(locate_np(nodes, vox, 0, 1.0, P), ref)
    assert np.array_equal(locate_np(nodes, vox, 0, 1.0, np.asfortranarray(P)), ref)
    assert np.array_equal(locate_np(nodes, vox, 0, 1.0, P.tolist()), ref)
    assert np.array_equal(locate_np(nodes, vox, 0, 1.0, np.repeat(P, 2, axis=0)[::2]), ref)
    e = locate_np(nodes, vox, 0, 1.0, np.empty((0, 3)))
    assert e.shape == (0,) and e.dtype == np.int32
    with pytest.raises(ValueError):
        locate_np(nodes, vox, 0, 1.0, np.zeros((4, 2)))
    with pytest.raises(ValueError):
        locate_np(nodes, vox, 0, 1.0, np.zeros(3))


# ---- pooled planes and distances against exact arithmetic ----------------------------------------------------------------
def _exact(P):
    rows = [[Fraction(float(x)) for x in p] for p in np.asarray(P, dtype=np.float64)]
    n = len(rows)
    m = [sum(r[a] for r in rows) / n for a in range(3)]
    c = [sum((r[i] - m[i]) * (r[j] - m[j]) for r in rows) / n for i, j in _UPPER]
    return m, c


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_pooled_against_fractions(dtype):
    rng = np.random.default_rng(7)
    a = [(5, rng.random((9, 3))), (2, rng.random((4, 3)) + 5.0e6), (9, np.empty((0, 3)))]
    b = [(2, rng.random((7, 3)) + 5.0e6), (11, rng.random((1, 3)))]
    c = [(5, rng.random((30, 3)) * [1.0, 1.0, 1e-6])]
    pl = pooled_leaf_statistics_np([a, b, c], dtype=dtype)
    assert isinstance(pl, LeafPlanes) and pl.node.tolist() == [2, 5, 11] and pl.node.dtype == np.int32
    pools = {2: np.concatenate([a[1][1], b[0][1]]), 5: np.concatenate([a[0][1], c[0][1]]), 11: b[1][1]}
    unit = EPS if dtype is np.float64 else float(np.finfo(np.longdouble).eps)
    for i, node in enumerate(pl.node.tolist()):
        P = pools[node]
        n = len(P)
        assert pl.count[i] == n
        m, cv = _exact(P)
        scale = float(np.abs(P).max())
        for k in range(3):
            assert abs(Fraction(float(pl.mean[i, k])) - m[k]) <= Fraction(4 * n * unit * scale + EPS * abs(float(m[k])))
        for k, (r, s) in enumerate(_UPPER):
            err = abs(Fraction(float(pl.covariance[i, r, s])) - cv[k])
            assert err <= Fraction(8 * n * unit * scale * scale + EPS * abs(float(cv[k])))
    assert len(pooled_leaf_statistics_np([])) == 0 and len(pooled_leaf_statistics_np([[], []])) == 0


def test_point_to_plane_against_fractions():
    rng = np.random.default_rng(8)
    flat = rng.random((40, 3)) * [1.0, 1.0, 1e-3]
    fat = rng.random((40, 3))
    few = rng.random((3, 3))
    pl = pooled_leaf_statistics_np([[(4, flat), (6, fat), (8, few)]])
    Q = rng.random((60, 3))
    node = np.tile([4, 6, 8, -1, 5], 12)
    row, dist = point_to_plane_np(node, pl, Q, min_points=8, max_variance=1e-3)
    assert row.dtype == np.int32 and dist.dtype == np.float64
    assert np.array_equal(row, np.tile([0, -1, -1, -1, -1], 12))       # fat: rejected, few: under-populated, 5: no row
    assert np.all(np.isnan(dist[row < 0])) and np.all(np.isfinite(dist[row >= 0]))
    row2, dist2 = point_to_plane_np(node, pl, Q, min_points=1, max_variance=None)
    assert np.array_equal(row2, np.tile([0, 1, 2, -1, -1], 12))
    for dtype, r_, d_ in ((np.float64, row2, dist2),) + \
            ((np.longdouble,) + point_to_plane_np(node, pl, Q, 1, None, dtype=np.longdouble),):
        unit = EPS if dtype is np.float64 else float(np.finfo(np.longdouble).eps)
        for i in np.nonzero(r_ >= 0)[0]:
            nrm = [Fraction(float(x)) for x in pl.normal[r_[i]]]
            d = [Fraction(float(Q[i, a])) - Fraction(float(pl.mean[r_[i], a])) for a in range(3)]
            exact = sum(x * y for x, y in zip(nrm, d))
            mag = sum(abs(x * y) for x, y in zip(nrm, d))
            assert abs(Fraction(float(d_[i])) - exact) <= 4 * Fraction(unit) * mag + Fraction(EPS) * abs(exact)
    r0, d0 = point_to_plane_np(np.empty(0, dtype=np.int32), pl, np.empty((0, 3)))
    assert r0.shape == (0,) and d0.shape == (0,)


# ---- the plug path end to end on the host ------------------------------------------------------------------------------
class HostOctree(OctreeBase):
    """A caller's own octree type that lives on the host (the oracle's tree behind the OctreeBase surface)."""

    def __init__(self, octree_config, corner_min, edge_length):
        super().__init__(octree_config, corner_min, edge_length)
        self._t = OTree(np.asarray(corner_min), edge_length)

    def insert_points(self, points):
        self._t.insert_points(points)

    def subdivide(self, subdivision_criteria):
        self._t.subdivide(subdivision_criteria)

    def subdivide_as(self, other):
        self._t.subdivide_as(other._t)

    def filter(self, filtering_criteria):
        self._t.filter(filtering_criteria)

    def map_leaf_points(self, function):
        self._t.map_leaf_points(function)

    def apply_mask(self, mask):
        self._t.apply_mask(np.asarray(mask, dtype=bool))

    def get_points(self):
        return self._t.get_points()

    def get_leaf_points(self, non_empty=True):
        return [Voxel(np.asarray(v.corner, dtype=np.float64), float(v.edge), self._t.points[v.idx])
                for v in self._t.leaves(non_empty)]

    n_points = property(lambda self: self._t.n_points)
    n_leaves = property(lambda self: self._t.n_leaves)
    n_nodes = property(lambda self: self._t.n_nodes)


class HostManager(OctreeManager):
    pass


def _check_answers(obj, clouds, extra_bad):
    """locate / leaf_planes / point_to_plane of a plug-path object against the host definitions on its own leaves."""
    corner, edge = obj.node_cubes()
    planes = obj.leaf_planes()
    assert np.all(np.diff(planes.node) > 0)
    total = 0
    for pose, P in clouds.items():
        node = obj.locate(P)
        assert node.dtype == np.int32 and np.all(node >= 0)
        a = P - corner[node]
        assert np.all((a >= 0) & (a < edge[node][:, None]))
        total += len(P)
    assert int(planes.count.sum()) == total
    one = obj.leaf_planes([next(iter(clouds))])
    assert int(one.count.sum()) == len(next(iter(clouds.values())))
    with pytest.raises(KeyError):
        obj.leaf_planes([99])
    Q = np.concatenate([next(iter(clouds.values()))[:200] + 1e-4, extra_bad])
    res = obj.point_to_plane(Q, min_points=5, max_variance=None)
    assert np.all(res.node[-len(extra_bad):] == -1) and np.all(res.row[-len(extra_bad):] == -1)
    ok = res.row >= 0
    assert ok.sum() > 100 and np.all(np.isnan(res.distance[~ok]))
    assert np.all(res.planes.node[res.row[ok]] == res.node[ok]) and np.all(res.planes.count[res.row[ok]] >= 5)
    ref = np.einsum("ij,ij->i", res.planes.normal[res.row[ok]], Q[ok] - res.planes.mean[res.row[ok]])
    assert np.allclose(res.distance[ok], ref, rtol=0, atol=1e-12)
    assert obj.locate(np.empty((0, 3))).shape == (0,)
    with pytest.raises(ValueError):
        obj.locate(np.zeros((3, 4)))


def test_plug_manager_on_the_host():
    rng = np.random.default_rng(11)
    m = HostManager(HostOctree, OctreeConfigBase(), np.array([-2.0, -2.0, -2.0]), 4.0)
    clouds = {3: rng.uniform(-2, 2, (1500, 3)) * [1, 1, 0.1], 7: rng.uniform(-2, 2, (900, 3)) * [1, 0.1, 1]}
    for p, P in clouds.items():
        m.insert_points(p, P)
    m.subdivide([MaxPoints(30)])
    _check_answers(m, clouds, np.array([[2.0, 0, 0], [np.nan, 0, 0], [0, -2.5, 0]]))


def test_empty_plug_manager_and_no_leaves():
    # trees that hold nothing yet: the roots are the leaves (and building the table terminates)
    nodes, ids = node_table_from_leaves([(np.zeros(3), 4.0), (np.array([4.0, 0.0, 0.0]), 4.0)], [])
    assert nodes["first_child"].tolist() == [-1, -1] and sorted(ids.values()) == [0, 1]
    m = HostManager(HostOctree, OctreeConfigBase(), np.zeros(3), 4.0)
    Q = np.array([[1.0, 1.0, 1.0], [4.0, 1.0, 1.0], [np.nan, 0.0, 0.0], [0.0, 0.0, 0.0]])
    assert m.locate(Q).tolist() == [0, -1, -1, 0]
    planes = m.leaf_planes()
    assert isinstance(planes, LeafPlanes) and len(planes) == 0 and len(planes.node) == 0
    res = m.point_to_plane(Q)
    assert res.node.tolist() == [0, -1, -1, 0] and np.all(res.row == -1) and np.all(np.isnan(res.distance))
    corner, edge = m.node_cubes()
    assert corner.tolist() == [[0.0, 0.0, 0.0]] and edge.tolist() == [4.0]
    # a pose without points changes nothing
    m.insert_points(1, np.empty((0, 3)))
    assert m.locate(Q).tolist() == [0, -1, -1, 0] and len(m.leaf_planes()) == 0


def test_plug_grid_on_the_host():
    rng = np.random.default_rng(12)
    g = Grid(GridConfig(octree_manager_type=HostManager, octree_type=HostOctree, octree_config=OctreeConfigBase(),
                        voxel_edge_length=2))
    assert g._plug is not None
    clouds = {0: rng.uniform(-2, 4, (2500, 3)) * [1, 1, 0.2], 1: rng.uniform(0, 4, (1200, 3))}
    # the one step of the plug path that runs on the device is the voxel bucketing of insert_points
    # (grid/_plugged.py); without a GPU the test does that step in NumPy and hands the voxels to the plug's managers
    for pose, P in clouds.items():
        vox = (np.floor_divide(P, 2.0) * 2).astype(int)
        uniq, inv = np.unique(vox, axis=0, return_inverse=True)
        g._plug._pose_voxels[pose] = []
        for j, coords in enumerate(uniq):
            key = tuple(int(c) for c in coords)
            if key not in g._plug._managers:
                g._plug._managers[key] = HostManager(HostOctree, OctreeConfigBase(), np.array(coords), 2)
            g._plug._pose_voxels[pose].append(key)
            g._plug._managers[key].insert_points(pose, P[inv.reshape(-1) == j])
    g.subdivide([MaxPoints(40)])
    _check_answers(g, clouds, np.array([[9.0, 0, 0], [0, np.inf, 0], [0, 0, -5.0]]))


# ---- header and signature table ------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "octreelib_hip.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_entries_declared_and_in_signature_table():
    from octreelib_amd import _native as nat

    header = _header()
    for name, decl in ENTRIES.items():
        assert decl + ";" in header, f"{name} is not declared as `{decl}`"
        res, _ = nat.SIGNATURES[name]
        assert res is C.c_int
    p, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    assert nat.SIGNATURES["octl_forest_pooled_leaf_stats"][1] == [p, p, i32, i64, p, p, p, p, p, p, C.POINTER(i64)]
    assert nat.SIGNATURES["octl_forest_locate"][1] == [p, p, i64, p]
    assert nat.SIGNATURES["octl_forest_locate_device"][1] == [p, p, i64, p]
    assert nat.SIGNATURES["octl_forest_point_to_plane"][1] == [p, p, i64, i32, f64, p, p, p]
    assert nat.SIGNATURES["octl_forest_point_to_plane_device"][1] == [p, p, i64, i32, f64, p, p, p]
    if os.path.exists(nat.lib_path()):
        lib = nat.load()
        for name in ENTRIES:
            assert getattr(lib, name).argtypes == nat.SIGNATURES[name][1]
        assert lib.octl_abi_version() == 1


def test_exported_from_the_package():
    import octreelib_amd

    for name in ("LeafPlanes", "PointToPlane", "locate_np", "pooled_leaf_statistics_np", "point_to_plane_np"):
        assert name in octreelib_amd.__all__ and hasattr(octreelib_amd, name)
