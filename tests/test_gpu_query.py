"""Map queries on the device: octl_forest_locate, octl_forest_pooled_leaf_stats, octl_forest_point_to_plane and their
Python surface (Grid / OctreeManager / Octree: locate, leaf_planes, point_to_plane).

Contracts (eps = 2^-53, L = 4096):
 * locate equals locate_np on the downloaded tables, exactly, and agrees with where a late pose's points are placed;
 * pooled planes: with B pooled blocks of at most n_max points, a = the leaf's centre, R = max |p - a|_inf over the
   pooled points and gamma = (ceil(n_max / 64) + ceil(n_max / L) + B + 16) eps, every mean component is within
   2 gamma R + eps |mean| and every covariance entry within 4 gamma R^2 of the longdouble two-pass value; the eigen
   contract is that of leaf_statistics (64 eps |C|_F);
 * distances: within 4 eps (|nx dx| + |ny dy| + |nz dz|) of the longdouble value formed from the returned plane."""

import ctypes as C
import math

import numpy as np
import pytest

from octreelib_amd import MaxPoints, NotPlanar, synthetic
from octreelib_amd import _native as nat
from octreelib_amd._engine import Forest
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree_manager import OctreeManager
from octreelib_amd.query import LeafPlanes, locate_np, point_to_plane_np, pooled_leaf_statistics_np

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
L = 64 * 64
_UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
BAD = np.array([[1e300, 0.0, 0.0], [0.0, -2.0 ** 31, 0.0], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5],
                [0.5, 0.5, -np.inf], [-777.5, 3.0, 3.0]])


# ---- helpers -------------------------------------------------------------------------------------------------------
def _counter(name):
    c = C.c_uint64(0)
    getattr(nat.load(), name)(C.byref(c))
    return c.value


def _host_locate(f: Forest, Q):
    return locate_np(f.nodes, f.voxels, f.mode, f._cube[1], Q)


class _DevBuf:
    def __init__(self, ctx, nbytes):
        self.ctx, self.p = ctx, C.c_void_p()
        ctx.check(ctx.lib.octl_dev_alloc(ctx.handle, max(int(nbytes), 8), C.byref(self.p)))

    def upload(self, a):
        a = np.ascontiguousarray(a)
        self.ctx.check(self.ctx.lib.octl_dev_upload(self.ctx.handle, self.p, nat.ptr(a), a.nbytes))

    def download(self, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        if out.nbytes:
            self.ctx.check(self.ctx.lib.octl_dev_download(self.ctx.handle, nat.ptr(out), self.p, out.nbytes))
        return out

    def free(self):
        self.ctx.lib.octl_dev_free(self.ctx.handle, self.p)


def _locate_device_form(f: Forest, Q):
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    xin, out = _DevBuf(f.ctx, Q.nbytes), _DevBuf(f.ctx, 4 * len(Q))
    try:
        xin.upload(Q)
        f.locate_device(xin.p, len(Q), out.p)
        return out.download(len(Q), np.int32)
    finally:
        xin.free()
        out.free()


def _boundary_queries(nd):
    """Points with coordinates exactly on splitting planes: centres of the split nodes, points on one of their
    planes, and corners.  Asserts that every depth of the tree contributes a splitting plane the set lies on."""
    fc = nd["first_child"]
    internal = np.nonzero(fc >= 0)[0]
    assert len(internal)
    half = (nd["edge"][internal] / 2.0)[:, None]
    centres = nd["corner"][internal] + half
    Q = np.concatenate([centres, centres + half * [0.5, 0.0, 0.25], nd["corner"][internal]])
    depth = nd["depth"][internal]
    for d in range(int(depth.max()) + 1):
        planes = centres[depth == d]
        assert len(planes), f"no split node at depth {d}"
        assert any(np.isin(Q[:, a], planes[:, a]).any() for a in range(3)), d
    return Q


def _check_locate(f: Forest, Q, what):
    Q = np.concatenate([Q, BAD])
    got = f.locate(Q)
    ref = _host_locate(f, Q)
    assert got.dtype == np.int32 and np.array_equal(got, ref), (what, int((got != ref).sum()))
    assert np.array_equal(_locate_device_form(f, Q), got), what
    assert np.all(got[-len(BAD):] == -1), what
    return got[:-len(BAD)]


def _second_scan(P, seed=0):
    """Queries around a cloud: its points jittered, some pushed out of the scene."""
    rng = np.random.default_rng(seed)
    Q = P[rng.permutation(len(P))[: min(len(P), 20000)]] + rng.normal(0.0, 0.01, (min(len(P), 20000), 3))
    Q[: len(Q) // 10] += rng.uniform(-3.0, 3.0, (len(Q) // 10, 3))
    return Q


# ---- locate ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["count", "planar"])
def test_locate_planar_scene(rule):
    P = synthetic.planar_cloud(60000, (4, 4, 2), seed=3, sigma=0.001)
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P)
    g.subdivide([MaxPoints(64)] if rule == "count" else [NotPlanar(1e-4, min_points=16)])
    f = g._forest
    assert f.nodes["depth"].max() >= 2
    node = _check_locate(f, np.concatenate([_second_scan(P), _boundary_queries(f.nodes), P[:5000]]), rule)
    assert (node >= 0).mean() > 0.8 and (node < 0).any()
    assert np.all(f.nodes["first_child"][node[node >= 0]] < 0)
    # every stored point locates to the leaf that stores it
    for v in g.get_leaf_points(0)[::7]:
        assert np.all(g.locate(v.get_points()) == v.node)


def test_locate_multi_pose_manager_octree_utm_unsubdivided():
    rng = np.random.default_rng(5)
    # a multi-pose grid whose scheme comes from a pose subset, negative coordinates
    g = Grid(GridConfig(voxel_edge_length=2))
    clouds = [rng.uniform(-5.0, 5.0, (20000, 3)) * [1, 1, 0.3] for _ in range(3)]
    for p, P in enumerate(clouds):
        g.insert_points(p, P)
    g.subdivide([MaxPoints(30)], pose_numbers=[0, 2])
    _check_locate(g._forest, np.concatenate([_second_scan(np.vstack(clouds), 1), _boundary_queries(g._forest.nodes)]),
                  "multi-pose")
    # a manager and a single octree (one cube)
    m = OctreeManager(Octree, OctreeConfig(), np.array([-4.0, -4.0, -4.0]), 8.0)
    for p in (4, 9):
        m.insert_points(p, rng.uniform(-4.0, 4.0, (8000, 3)))
    m.subdivide([MaxPoints(25)])
    Qm = np.concatenate([rng.uniform(-5.0, 5.0, (20000, 3)), _boundary_queries(m._forest.nodes),
                         [[4.0, 0, 0], [-4.0, -4.0, -4.0]]])
    node = _check_locate(m._forest, Qm, "manager")
    assert (node < 0).any() and (node >= 0).any() and np.array_equal(m.locate(Qm), node)
    t = Octree(OctreeConfig(), np.zeros(3), 4.0)
    assert np.array_equal(t.locate(np.ones((3, 3))), _host_locate(t._forest, np.ones((3, 3))))   # (no points yet)
    t.insert_points(rng.random((5000, 3)) * 4.0)
    assert t.locate([[1.0, 1.0, 1.0], [4.0, 1.0, 1.0]]).tolist() == [0, -1]   # unsubdivided: the root
    t.subdivide([MaxPoints(20)])
    _check_locate(t._forest, np.concatenate([rng.uniform(-1, 5, (5000, 3)), _boundary_queries(t._forest.nodes)]),
                  "octree")
    # far from the origin (UTM magnitudes)
    off = np.array([5.0e6, 4.0e5, 100.0])
    U = synthetic.planar_cloud(30000, (3, 3, 2), seed=9) + off
    gu = Grid(GridConfig(voxel_edge_length=1))
    gu.insert_points(0, U)
    gu.subdivide([MaxPoints(48)])
    node = _check_locate(gu._forest, np.concatenate([_second_scan(U, 2), _boundary_queries(gu._forest.nodes)]), "utm")
    assert (node >= 0).mean() > 0.5
    # an unsubdivided grid answers with root nodes
    g0 = Grid(GridConfig(voxel_edge_length=1))
    g0.insert_points(0, rng.random((3000, 3)) * 3.0)
    node = _check_locate(g0._forest, rng.uniform(-1.0, 4.0, (4000, 3)), "unsubdivided")
    assert node.max() < len(g0._forest.voxels) and (node >= 0).any()
    # input forms
    P32 = (rng.random((500, 3)) * 3.0).astype(np.float32)
    ref = g0.locate(P32.astype(np.float64))
    assert np.array_equal(g0.locate(P32), ref) and np.array_equal(g0.locate(np.asfortranarray(P32)), ref)
    assert np.array_equal(g0.locate(P32.tolist()), ref)
    assert g0.locate(np.empty((0, 3))).shape == (0,)
    with pytest.raises(ValueError):
        g0.locate(np.zeros((4, 2)))


def test_locate_agrees_with_placement():
    P = synthetic.planar_cloud(40000, (4, 4, 2), seed=3)
    Q = synthetic.planar_cloud(15000, (5, 4, 2), seed=11)        # a late pose that also brings new voxels
    g1, g2 = Grid(GridConfig(voxel_edge_length=1)), Grid(GridConfig(voxel_edge_length=1))
    for g in (g1, g2):
        g.insert_points(0, P)
        g.subdivide([MaxPoints(50)])
    before = g1.locate(Q)
    g2.insert_points(1, Q)
    f2 = g2._forest
    blk = f2.blocks
    late = np.nonzero(blk["slot"] == 1)[0]
    assert len(late) > 100
    c1, e1 = g1.node_cubes()
    c2, e2 = g2.node_cubes()
    seen = 0
    for b in late.tolist():
        pts = f2.xyz[blk["start"][b]: blk["start"][b] + blk["size"][b]]
        assert np.all(g2.locate(pts) == blk["node"][b])
        # ... and the grid that never saw the pose names the same cube, or has no voxel there
        n1 = g1.locate(pts)
        hit = n1 >= 0
        assert np.all(c1[n1[hit]] == c2[blk["node"][b]]) and np.all(e1[n1[hit]] == e2[blk["node"][b]])
        assert np.all(f2.nodes["depth"][blk["node"][b]] == 0) or hit.all()
        seen += len(pts)
    assert seen == len(Q) and (before < 0).any() and (before >= 0).any()


def test_queries_are_read_only_and_launch_shape():
    P = synthetic.planar_cloud(60000, (4, 4, 2), seed=3)
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P)
    g.insert_points(1, synthetic.planar_cloud(30000, (4, 4, 2), seed=3, stream=1))
    g.subdivide([MaxPoints(64)])
    f = g._forest
    Q = np.concatenate([_second_scan(P, 3), BAD])
    err_before = f.lib.octl_last_error(f.ctx.handle)

    def snapshot():
        f._invalidate()
        return (tuple(v.tobytes() for v in f.nodes.values()), tuple(v.tobytes() for v in f.blocks.values()),
                f.perm.tobytes(), f.xyz.tobytes(), tuple(f._slot_counts(s) for s in (0, 1)))

    s0 = snapshot()
    planes = g.leaf_planes()
    g.locate(Q)
    _locate_device_form(f, Q)
    g.point_to_plane(Q)
    g.leaf_planes([1])
    assert snapshot() == s0
    assert f.lib.octl_last_error(f.ctx.handle) == err_before
    f._pooled = None
    g.leaf_planes()
    # launch and host-wait counts: constant in n and equal to the documented shape
    xin, n_out, r_out, d_out = (_DevBuf(f.ctx, Q.nbytes), _DevBuf(f.ctx, 4 * len(Q)), _DevBuf(f.ctx, 4 * len(Q)),
                                _DevBuf(f.ctx, 8 * len(Q)))
    xin.upload(Q)
    node = np.empty(len(Q), dtype=np.int32)
    row = np.empty(len(Q), dtype=np.int32)
    dist = np.empty(len(Q), dtype=np.float64)
    lib, h = f.lib, f.handle
    calls = {
        "locate": lambda n: lib.octl_forest_locate(h, nat.ptr(Q), n, nat.ptr(node)),
        "locate_device": lambda n: lib.octl_forest_locate_device(h, xin.p, n, n_out.p),
        "p2p": lambda n: lib.octl_forest_point_to_plane(h, nat.ptr(Q), n, 8, -1.0, nat.ptr(node), nat.ptr(row),
                                                        nat.ptr(dist)),
        "p2p_device": lambda n: lib.octl_forest_point_to_plane_device(h, xin.p, n, 8, -1.0, n_out.p, r_out.p, d_out.p),
    }
    expect = {"locate": (1, 1), "locate_device": (1, 0), "p2p": (1, 1), "p2p_device": (1, 0)}
    try:
        for name, fn in calls.items():
            assert fn(len(Q)) == 0      # (warm: staging allocated, voxel codes on the device)
            f.ctx.sync()
            for n in (100, len(Q)):
                a, b = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
                assert fn(n) == 0
                got = (_counter("octl_debug_launches") - a, _counter("octl_debug_host_syncs") - b)
                assert got == expect[name], (name, n, got)
            f.ctx.sync()
        # the device forms answer what the host forms answer
        ref = g.point_to_plane(Q)
        assert np.array_equal(n_out.download(len(Q), np.int32), ref.node)
        assert np.array_equal(r_out.download(len(Q), np.int32), ref.row)
        assert np.array_equal(d_out.download(len(Q), np.float64), ref.distance, equal_nan=True)
    finally:
        for b in (xin, n_out, r_out, d_out):
            b.free()
    assert len(planes) == len(g.leaf_planes())
    # a later insertion is placed as if no query had happened (the error word is clean)
    g.insert_points(2, synthetic.planar_cloud(5000, (4, 4, 2), seed=3, stream=2))
    assert g.n_points(2) == 5000


# ---- pooled planes ---------------------------------------------------------------------------------------------------
def _assert_eigen(w, v, cov):
    n = len(w)
    fn = np.sqrt((cov ** 2).sum(axis=(1, 2)))
    assert np.all(w[:, 0] <= w[:, 1]) and np.all(w[:, 1] <= w[:, 2])
    assert np.abs(np.einsum("nki,nkj->nij", v, v) - np.eye(3)).max() <= 64 * EPS
    res = np.linalg.norm(np.einsum("nij,njk->nik", cov, v) - v * w[:, None, :], axis=1)
    assert np.all(res <= 64 * EPS * fn[:, None])
    for col in range(3):   # sign rule
        x = v[:, :, col]
        assert np.all(x[np.arange(n), np.argmax(np.abs(x), axis=1)] > 0)


def _check_planes(obj, f: Forest, planes: LeafPlanes, slots, leaves_of_slot, what):
    """Rows complete and ascending; every row within the stated bound of the longdouble two-pass value."""
    blk = f.blocks
    sel = np.isin(blk["slot"], slots)
    assert np.array_equal(planes.node, np.unique(blk["node"][sel])), what
    assert planes.node.dtype == np.int32 and len(planes) > 0, what
    by_pose = [[(v.node, v.get_points()) for v in leaves_of_slot(s)] for s in sorted(slots)]
    ref = pooled_leaf_statistics_np(by_pose, dtype=np.longdouble)
    assert np.array_equal(ref.node, planes.node) and np.array_equal(ref.count, planes.count), what
    nd = f.nodes
    pools = {}
    for leaves in by_pose:
        for node, pts in leaves:
            pools.setdefault(node, []).append(pts)
    worst = 0.0
    for i, node in enumerate(planes.node.tolist()):
        parts = pools[node]
        a = nd["corner"][node] + nd["edge"][node] / 2.0
        R = max(float(np.abs(p.astype(np.longdouble) - a).max()) for p in parts)
        n_max = max(len(p) for p in parts)
        g = (math.ceil(n_max / 64) + math.ceil(n_max / L) + len(parts) + 16) * EPS
        em = np.abs(planes.mean[i].astype(np.longdouble) - ref.mean[i])
        assert np.all(em <= 2 * g * R + EPS * np.abs(ref.mean[i])), (what, node, em, R)
        ec = np.abs(planes.covariance[i].astype(np.longdouble) - ref.covariance[i])
        assert np.all(ec <= 4 * g * R * R), (what, node, float(ec.max()), R)
        if R > 0:
            worst = max(worst, float(ec.max() / (4 * g * R * R)))
    print(f"{what}: {len(planes)} leaves, worst covariance error / bound = {worst:.3f}")
    _assert_eigen(planes.eigenvalues, planes.eigenvectors, planes.covariance)


@pytest.mark.parametrize("n_poses", [1, 2, 5])
def test_pooled_planes_poses(n_poses):
    g = Grid(GridConfig(voxel_edge_length=1))
    for p in range(n_poses):
        g.insert_points(10 + p, synthetic.planar_cloud(15000, (3, 3, 2), seed=4, stream=p, sigma=0.002))
    g.subdivide([MaxPoints(48)])
    f = g._forest
    leaves = lambda s: g.get_leaf_points(10 + s)
    _check_planes(g, f, g.leaf_planes(), list(range(n_poses)), leaves, f"{n_poses} poses")
    if n_poses == 5:
        sub = g.leaf_planes([11, 14])
        _check_planes(g, f, sub, [1, 4], leaves, "subset")
        assert g.leaf_planes([14, 11]) is sub            # (same selection: the copy made for it)
        with pytest.raises(KeyError):
            g.leaf_planes([3])
        # the same bits whatever cap: the selection alternates between NULL and all ones - the same poses, but another
        # selection to the library, which therefore computes the table again for every call instead of downloading
        # the one it holds
        full = g.leaf_planes()
        n = len(full)
        ones = np.ones(5, dtype=np.uint8)
        outs = []
        for cap, sel, n_sel in ((n, nat.ptr(ones), 5), (n + 1000, None, 0), (n + 7, nat.ptr(ones), 5)):
            before = _counter("octl_debug_launches")
            node = np.empty(cap, dtype=np.int32)
            cnt = np.empty(cap, dtype=np.int64)
            mean = np.empty((cap, 3))
            cov = np.empty((cap, 6))
            w = np.empty((cap, 3))
            v = np.empty((cap, 9))
            got = C.c_int64(0)
            f.ctx.check(f.lib.octl_forest_pooled_leaf_stats(f.handle, sel, n_sel, cap, nat.ptr(node), nat.ptr(cnt),
                                                            nat.ptr(mean), nat.ptr(cov), nat.ptr(w), nat.ptr(v),
                                                            C.byref(got)))
            assert got.value == n
            assert _counter("octl_debug_launches") > before, "the table was not computed again"
            outs.append((node[:n].tobytes(), cnt[:n].tobytes(), mean[:n].tobytes(), cov[:n].tobytes(),
                         w[:n].tobytes(), v[:n].tobytes()))
        assert outs[0] == outs[1] == outs[2]
        f._pooled = None      # (the device table is now the all-ones selection's: the next leaf_planes() asks again)
        assert outs[0][2] == full.mean.tobytes() and outs[0][4] == full.eigenvalues.tobytes()
        # other leaves emptied by filter: a leaf that kept all its points keeps its bits
        g.filter([lambda pts: len(pts) >= 6])
        after = g.leaf_planes()
        assert 0 < len(after) and f.n_ord < 5 * 15000
        pos = np.searchsorted(full.node, after.node)
        same = full.count[pos] == after.count
        assert same.sum() > 10 and (~same).sum() > 0
        for name in ("mean", "covariance", "eigenvalues", "eigenvectors"):
            assert getattr(after, name)[same].tobytes() == getattr(full, name)[pos][same].tobytes(), name
        _check_planes(g, f, after, list(range(5)), leaves, "after filter")


def test_pooled_planes_ransac_displaced_utm_large_block():
    # after RANSAC + apply_mask
    g = Grid(GridConfig(voxel_edge_length=1))
    for p in range(2):
        g.insert_points(p, synthetic.planar_cloud(30000, (3, 3, 2), seed=6, stream=p, sigma=0.002))
    g.subdivide([MaxPoints(64)])
    n_before = g._forest.n_ord
    np.random.seed(1)
    g.map_leaf_points_cuda_ransac(poses_per_batch=2, threshold=0.01, hypotheses_number=128, initial_points_number=6)
    leaves = lambda s: g.get_leaf_points(s)
    planes = g.leaf_planes()
    assert g._forest.n_ord < n_before
    _check_planes(g, g._forest, planes, [0, 1], leaves, "after RANSAC")
    assert np.median(planes.eigenvalues[planes.count >= 16, 0]) < 1e-4      # the inliers are flat

    # map_leaf_points moved rows out of their cubes: R is measured, not assumed
    def fn(p):
        return p + np.array([0.0, 0.0, 0.4]) if len(p) % 2 else p[::-1]

    g.map_leaf_points(fn, [1])
    _check_planes(g, g._forest, g.leaf_planes(), [0, 1], leaves, "displaced rows")
    # UTM magnitudes
    gu = Grid(GridConfig(voxel_edge_length=1))
    for p in range(2):
        gu.insert_points(p, synthetic.planar_cloud(20000, (3, 3, 2), seed=9, stream=p) + [5.0e6, 4.0e5, 100.0])
    gu.subdivide([MaxPoints(48)])
    _check_planes(gu, gu._forest, gu.leaf_planes(), [0, 1], lambda s: gu.get_leaf_points(s), "utm")
    # blocks above 4096 points (no subdivide: one leaf per voxel), three poses of different sizes
    rng = np.random.default_rng(2)
    gl = Grid(GridConfig(voxel_edge_length=2))
    for p, n in enumerate((3 * L + 17, 100, L + 1)):
        gl.insert_points(p, rng.random((n, 3)) * [2.0, 2.0, 0.02] + [0.0, 0.0, 1.0])
    big = gl.leaf_planes()
    assert big.count.tolist() == [3 * L + 17 + 100 + L + 1]
    _check_planes(gl, gl._forest, big, [0, 1, 2], lambda s: gl.get_leaf_points(s), "large blocks")
    assert abs(big.normal[0, 2]) > 1 - 1e-6
    # a manager and an octree speak the same surface
    m = OctreeManager(Octree, OctreeConfig(), np.zeros(3), 4.0)
    for p in (7, 2):
        m.insert_points(p, rng.random((6000, 3)) * 4.0)
    m.subdivide([MaxPoints(40)])
    slot = {7: 0, 2: 1}
    _check_planes(m, m._forest, m.leaf_planes([2]), [1], lambda s: m.get_leaf_points(True, {v: k for k, v in slot.items()}[s]),
                  "manager subset")
    t = Octree(OctreeConfig(), np.zeros(3), 4.0)
    assert len(t.leaf_planes()) == 0
    t.insert_points(rng.random((6000, 3)) * 4.0)
    t.subdivide([MaxPoints(30)])
    _check_planes(t, t._forest, t.leaf_planes(), [0], lambda s: t.get_leaf_points(), "octree")


# ---- point to plane ---------------------------------------------------------------------------------------------------
def test_point_to_plane_distances_and_rules():
    """Scene and thresholds were chosen on the host path (oracle tree + locate_np + pooled_leaf_statistics_np, no GPU):
    map = planar_cloud(30000, (4, 4, 2), seed 3, sigma 0.001, inlier_fraction 0.8 - as the queries) split at 64 points, queries = stream 1 of the same scene
    with the first 1500 moved four voxels along x, min_points 8, max_variance 1e-3.  The host definition alone gave:
    accepted 61.6 %, missed voxel 7.5 %, leaf without points 0.3 %, under-populated 6.5 %, rejected 24.1 %."""
    P = synthetic.planar_cloud(30000, (4, 4, 2), seed=3, sigma=0.001, inlier_fraction=0.8)
    Q = synthetic.planar_cloud(20000, (4, 4, 2), seed=3, stream=1, sigma=0.001, inlier_fraction=0.8)
    Q[:1500, 0] += 4.0
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P)
    g.subdivide([MaxPoints(64)])
    mp, mv = 8, 1e-3
    res = g.point_to_plane(Q, min_points=mp, max_variance=mv)
    pl = res.planes
    assert res.node.dtype == np.int32 and res.row.dtype == np.int32 and res.distance.dtype == np.float64
    assert np.array_equal(res.node, g.locate(Q))
    # row / NaN rules: the host definition on the same table
    row_ref, _ = point_to_plane_np(res.node, pl, Q, mp, mv)
    assert np.array_equal(res.row, row_ref)
    ok = res.row >= 0
    assert np.all(np.isnan(res.distance[~ok])) and np.all(np.isfinite(res.distance[ok]))
    pos = np.minimum(np.searchsorted(pl.node, np.maximum(res.node, 0)), len(pl) - 1)
    has = (res.node >= 0) & (pl.node[pos] == res.node)
    missed = res.node < 0
    under = has & (pl.count[pos] < mp)
    rejected = has & (pl.count[pos] >= mp) & (pl.eigenvalues[pos, 0] > mv)
    shares = {k: float(v.mean()) for k, v in (("accepted", ok), ("missed", missed), ("under", under),
                                             ("rejected", rejected), ("empty", (res.node >= 0) & ~has))}
    print("shares:", shares)
    assert shares["accepted"] >= 0.5 and shares["missed"] >= 0.01 and shares["under"] >= 0.01 \
        and shares["rejected"] >= 0.01, shares
    assert np.array_equal(ok, has & ~under & ~rejected)
    assert np.all(pl.node[res.row[ok]] == res.node[ok])
    # distances against longdouble from the RETURNED plane bits
    nrm = pl.normal[res.row[ok]].astype(np.longdouble)
    d = Q[ok].astype(np.longdouble) - pl.mean[res.row[ok]].astype(np.longdouble)
    terms = nrm * d
    err = np.abs(res.distance[ok].astype(np.longdouble) - terms.sum(axis=1))
    bound = 4 * EPS * np.abs(terms).sum(axis=1)
    print("distance error / bound, worst:", float((err / np.maximum(bound, np.finfo(np.longdouble).tiny)).max()))
    assert np.all(err <= bound)
    assert np.median(np.abs(res.distance[ok])) < 0.05       # (a second scan of the same planes)
    # no thresholds: every leaf with points answers
    loose = g.point_to_plane(Q, min_points=1, max_variance=None)
    assert np.array_equal(loose.row >= 0, has) and loose.planes is pl
    # a pose subset makes another table
    g.insert_points(1, Q[2000:])
    both = g.point_to_plane(Q[:3000], [0, 1], min_points=mp)
    only1 = g.point_to_plane(Q[:3000], [1], min_points=mp)
    assert len(both.planes) >= len(only1.planes) > 0 and both.planes is not only1.planes
    assert np.array_equal(both.node, only1.node)
    e = g.point_to_plane(np.empty((0, 3)))
    assert e.node.shape == e.row.shape == e.distance.shape == (0,)


def test_point_to_plane_staleness():
    P = synthetic.planar_cloud(20000, (3, 3, 2), seed=3)
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P)
    g.subdivide([MaxPoints(64)])
    f = g._forest
    Q = np.ascontiguousarray(P[:1000] + 0.001)
    node, row, dist = np.empty(1000, np.int32), np.empty(1000, np.int32), np.empty(1000)

    def abi():
        return f.lib.octl_forest_point_to_plane(f.handle, nat.ptr(Q), 1000, 8, -1.0, nat.ptr(node), nat.ptr(row),
                                                nat.ptr(dist))

    assert abi() == nat.OCTL_E_STATE and b"no pooled" in f.lib.octl_last_error(f.ctx.handle)
    g.leaf_planes()
    assert abi() == 0
    np.random.seed(2)
    g.map_leaf_points_cuda_ransac(threshold=0.01, hypotheses_number=64)      # RANSAC + apply_mask
    assert abi() == nat.OCTL_E_STATE and b"stale" in f.lib.octl_last_error(f.ctx.handle)
    r1 = g.point_to_plane(Q)                                                   # the method recomputes
    assert abi() == 0 and np.array_equal(row, r1.row)
    g.insert_points(1, P[:500] + 0.002)
    assert abi() == nat.OCTL_E_STATE
    r2 = g.point_to_plane(Q)
    assert (r2.row >= 0).any() and int(r2.planes.count.sum()) == int(r1.planes.count.sum()) + 500
    g.filter([lambda pts: len(pts) >= 4])
    assert abi() == nat.OCTL_E_STATE
    assert len(g.point_to_plane(Q).planes) <= len(r2.planes)


# ---- the plug path ------------------------------------------------------------------------------------------------------
class _PlugManager(OctreeManager):
    pass


def test_plug_path_matches_device():
    P0 = synthetic.planar_cloud(6000, (2, 2, 2), seed=8)
    P1 = synthetic.planar_cloud(4000, (2, 2, 2), seed=8, stream=1)
    Q = np.concatenate([synthetic.planar_cloud(3000, (3, 2, 2), seed=8, stream=2), BAD])
    dev = Grid(GridConfig(voxel_edge_length=1))
    plug = Grid(GridConfig(voxel_edge_length=1, octree_manager_type=_PlugManager))
    for g in (dev, plug):
        g.insert_points(0, P0)
        g.insert_points(1, P1)
        g.subdivide([MaxPoints(64)])
    assert plug._plug is not None
    cd, ed = dev.node_cubes()
    cp, ep = plug.node_cubes()
    a, b = dev.point_to_plane(Q, min_points=6, max_variance=5e-3), plug.point_to_plane(Q, min_points=6, max_variance=5e-3)
    assert np.array_equal(a.node >= 0, b.node >= 0) and (a.node < 0).any()
    hit = a.node >= 0
    assert np.array_equal(cd[a.node[hit]], cp[b.node[hit]]) and np.array_equal(ed[a.node[hit]], ep[b.node[hit]])
    # the same leaves have planes; as cubes they are the same set
    key = lambda c, e, ids: sorted((tuple(c[i]), float(e[i])) for i in ids)
    assert key(cd, ed, a.planes.node) == key(cp, ep, b.planes.node)
    order_d = np.lexsort(np.column_stack([cd[a.planes.node], ed[a.planes.node]]).T[::-1])
    order_p = np.lexsort(np.column_stack([cp[b.planes.node], ep[b.planes.node]]).T[::-1])
    assert np.array_equal(a.planes.count[order_d], b.planes.count[order_p])
    # the device's planes within the stated bound of the plug path's (longdouble two-pass, rounded to f64: eps |value|
    # of its own), R / n_max / B from the leaf's pooled blocks as in _check_planes
    pools = {}
    for p in (0, 1):
        for v in dev.get_leaf_points(p):
            pools.setdefault(v.node, []).append(v.get_points())
    for i, j in zip(order_d.tolist(), order_p.tolist()):
        node = int(a.planes.node[i])
        parts = pools[node]
        centre = cd[node] + ed[node] / 2.0
        R = max(float(np.abs(q.astype(np.longdouble) - centre).max()) for q in parts)
        n_max = max(len(q) for q in parts)
        gam = (math.ceil(n_max / 64) + math.ceil(n_max / L) + len(parts) + 16) * EPS
        mb, cb = b.planes.mean[j], b.planes.covariance[j]
        assert np.all(np.abs(a.planes.mean[i] - mb) <= 2 * gam * R + EPS * np.abs(mb) + EPS * np.abs(mb)), node
        assert np.all(np.abs(a.planes.covariance[i] - cb) <= 4 * gam * R * R + EPS * np.abs(cb)), node
    both = (a.row >= 0) & (b.row >= 0)
    assert both.sum() > 500 and np.mean((a.row >= 0) == (b.row >= 0)) > 0.99
    assert np.allclose(a.distance[both], b.distance[both], rtol=0, atol=1e-9)
    with pytest.raises(KeyError):
        plug.leaf_planes([5])
