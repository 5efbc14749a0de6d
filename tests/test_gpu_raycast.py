"""The ray query on the device: octl_forest_raycast / _raycast_device and Grid / OctreeManager / Octree .raycast.

One contract: all fields of the answer (node, t, row) EQUAL those of the brute force octreelib_amd.query.raycast_np over
the map's own leaves - and, for the plane form, the map's own leaf_planes - in the host form and in the device form.  The
order (t, node) is total, so there is no tolerance to state.  Shapes are small because brute force is the checker."""

import numpy as np
import pytest

from octreelib_amd import MaxPoints, RayHits, normalize_directions, raycast_np, synthetic
from octreelib_amd import _native as nat
from octreelib_amd._engine import Forest
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree.octree_base import OctreeConfigBase
from octreelib_amd.octree_manager import OctreeManager
from octreelib_amd.query import RAY_CAP_EDGES, ray_inputs
from tests._raycast import DIRECTIONS, assert_hits_equal, box_rays, lattice_points, lattice_rays, leaves_of, tie_mask
from tests.test_cpu_query import HostManager, HostOctree
from tests.test_gpu_query import BAD, _counter, _DevBuf

pytestmark = pytest.mark.gpu


# ---- helpers -------------------------------------------------------------------------------------------------------
def _device_form(f: Forest, O, Dn, tmin, tmax, slots, surface, **kw):
    n = len(O)
    bufs = [_DevBuf(f.ctx, 24 * n), _DevBuf(f.ctx, 24 * n), _DevBuf(f.ctx, 8 * n), _DevBuf(f.ctx, 8 * n),
            _DevBuf(f.ctx, 4 * n), _DevBuf(f.ctx, 8 * n), _DevBuf(f.ctx, 4 * n)]
    try:
        for b, a in zip(bufs, (O, Dn, tmin, tmax)):
            b.upload(a)
        f.raycast_device(bufs[0].p, bufs[1].p, bufs[2].p, bufs[3].p, n, bufs[4].p, bufs[5].p, bufs[6].p, slots, surface,
                         **kw)
        return RayHits(bufs[4].download(n, np.int32), bufs[5].download(n, np.float64), bufs[6].download(n, np.int32))
    finally:
        for b in bufs:
            b.free()


def _leaf_set(f: Forest, slots=None):
    """((ids, corner, edge), count) of the scheme leaves with the alive points of the chosen slots, from the map's own
    node and block tables."""
    nd, b = f.nodes, f.blocks
    m = np.ones(len(b["node"]), dtype=bool) if slots is None else np.isin(b["slot"], list(slots))
    per_node = np.bincount(b["node"][m], weights=b["size"][m], minlength=len(nd["edge"])).astype(np.int64)
    return leaves_of(nd, per_node)


def _check(obj, O, D, t_max, what, t_min=0.0, pose_numbers=None, surface="cube", octree=False, **kw):
    """Both forms of the device answer against raycast_np over the map's own leaves (and planes)."""
    f = obj._forest
    slots = None if octree or pose_numbers is None else [obj._slots[p] for p in pose_numbers]
    sel = {} if octree else {"pose_numbers": pose_numbers}
    got = obj.raycast(O, D, t_max, min_range=t_min, surface=surface, **sel, **kw)
    assert isinstance(got, RayHits)
    planes = None
    if surface == "plane":
        planes = obj.leaf_planes() if octree else obj.leaf_planes(pose_numbers)
    cube, count = _leaf_set(f, slots)
    O, Dn, tmin, tmax = ray_inputs(O, normalize_directions(D), t_min, t_max)
    ref = raycast_np(O, Dn, tmax, *cube, t_min=tmin, count=count, planes=planes, surface=surface, **kw)
    assert_hits_equal(got, ref, what + " (host form)")
    assert_hits_equal(_device_form(f, O, Dn, tmin, tmax, slots, surface, **kw), ref, what + " (device form)")
    return ref, cube, count


def _grid(clouds, K, L=1):
    g = Grid(GridConfig(voxel_edge_length=L))
    for p, P in clouds.items():
        g.insert_points(p, P)
    g.subdivide([MaxPoints(K)])
    return g


# ---- the scenes -----------------------------------------------------------------------------------------------------------
def test_lattice_ties_and_grazing_contacts():
    g = _grid({0: lattice_points()}, 8)
    assert g._forest.nodes["depth"].max() == 2
    O, D = lattice_rays()
    ref, cube, count = _check(g, O, D, 6.0, "lattice")
    ties = tie_mask(O, normalize_directions(D), 6.0, cube, count=count)
    print(f"lattice: {len(O)} rays, {ref.hit.mean():.3f} hit, {ties.sum()} with a tie in t")
    assert ties.sum() >= 100 and 0.3 < ref.hit.mean() < 1.0
    _check(g, O, D, 6.0, "lattice, min_range", t_min=0.25)
    _check(g, O, D, 0.5, "lattice, short", t_min=0.125, min_points=8)
    _check(g, O, D, 6.0, "lattice, nothing holds 9", min_points=9)
    _check(g, O, D, 6.0, "lattice, planes", surface="plane")


def test_sparse_grid_with_gaps_at_the_cap():
    rng = np.random.default_rng(2)
    vox = np.argwhere(rng.random((14, 14, 3)) < 0.25) * [3, 3, 2] - [20, 20, 2]      # occupied voxels with gaps between
    P = np.concatenate([v + rng.random((40, 3)) for v in vox])
    g = _grid({0: P}, 12)
    O, D = box_rays(rng, [-20, -20, -2], [22, 22, 4], 1500, 120.0)
    ref, _, _ = _check(g, O, D, RAY_CAP_EDGES, "sparse grid, range at the cap")
    assert 0.1 < ref.hit.mean() < 0.9 and (ref.t[ref.hit] > 100.0).sum() > 50
    _check(g, O, D, 200.0 + RAY_CAP_EDGES, "sparse grid, the cap from min_range", t_min=200.0)
    A = np.repeat(np.array([[-30.0, 1.0, 0.5], [-30.0, -8.0, 1.0], [4.0, 40.0, 0.0], [1.5, 1.5, -40.0]]), 6, axis=0)
    Da = np.tile(DIRECTIONS[np.abs(DIRECTIONS).sum(axis=1) == 1], (4, 1))
    _check(g, A, Da, 100.0, "sparse grid, axis rays")
    # one call above the cap: Python refuses, the ABI refuses, the device form (which cannot look) finds nothing
    over = float(np.nextafter(RAY_CAP_EDGES, 1e9))
    with pytest.raises(ValueError, match="voxel edges"):
        g.raycast(O[:50], D[:50], over)
    f = g._forest
    o, d, tmin, tmax = ray_inputs(O[:50], normalize_directions(D[:50]), 0.0, over)
    node, t, row = np.empty(50, dtype=np.int32), np.empty(50), np.empty(50, dtype=np.int32)
    rc = f.lib.octl_forest_raycast(f.handle, nat.ptr(o), nat.ptr(d), nat.ptr(tmin), nat.ptr(tmax), 50, None, 0, 0, 1, -1.0,
                                   nat.ptr(node), nat.ptr(t), nat.ptr(row))
    assert rc == nat.OCTL_E_INVALID and b"voxel edges" in f.lib.octl_last_error(f.ctx.handle)
    dead = _device_form(f, o, d, tmin, tmax, None, "cube")
    assert np.all(dead.node == -1) and np.all(np.isinf(dead.t)) and np.all(dead.row == -1)
    # dead rays are answered, not refused - whatever their range
    bad = g.raycast(BAD, np.tile([[1.0, 0.0, 0.0]], (len(BAD), 1)), 50.0)
    assert np.all(bad.node[[2, 3, 4]] == -1)
    assert g.raycast(O[:4], D[:4], np.inf).node.tolist() == [-1] * 4 and g.raycast(O[:4], np.zeros((4, 3)), 9.0).hit.sum() == 0


def test_non_dyadic_octree_faces_and_splitting_planes():
    rng = np.random.default_rng(5)
    c0, e0 = 0.1, 3.3
    t = Octree(OctreeConfig(), np.array([c0, c0, c0]), e0)
    P = c0 + rng.random((5000, 3)) * e0 * [1.0, 1.0, 0.3]
    P = P[np.all((P - c0 >= 0) & (P - c0 < e0), axis=1)]
    t.insert_points(P)
    t.subdivide([MaxPoints(20)])
    nd = t._forest.nodes
    assert nd["depth"].max() >= 3
    inner = np.nonzero(nd["first_child"] >= 0)[0]
    split = nd["corner"][inner] + (nd["edge"][inner] / 2.0)[:, None]             # points on the splitting planes
    O, D = [], []
    for a in range(3):                      # through every face, on the faces, an ulp outside the cube
        for sign, wall in ((1.0, c0), (-1.0, c0 + e0)):
            o = c0 + rng.random((60, 3)) * e0 * [1.0, 1.0, 0.3]
            o[:, a] = wall - sign * 1.0
            d = np.zeros((60, 3))
            d[:, a] = sign
            d[20:40] += rng.normal(0.0, 0.2, (20, 3))
            b = (a + 1) % 3
            o[40:50, b], o[50:55, b], o[55:, b] = c0, np.nextafter(c0, -1.0), np.nextafter(c0 + e0, 9.0)
            o[45:50, b] = c0 + e0
            O.append(o)
            D.append(d)
    S = np.repeat(split[:100], 3, axis=0)
    S[:, 0] -= 5.0
    O.append(S)
    D.append(np.tile(np.array([[1.0, 0, 0], [1.0, 0.3, 0], [1.0, 0, -0.2]]), (100, 1)))
    O, D = np.concatenate(O), np.concatenate(D)
    ref, _, _ = _check(t, O, D, 1e6, "non-dyadic octree", octree=True)
    assert 0.3 < ref.hit.mean() < 0.98
    _check(t, O, D, 2e6, "non-dyadic octree from afar", t_min=3.0, octree=True)      # (one cube has no cap)
    _check(t, O, D, 9.0, "non-dyadic octree, planes", surface="plane", min_points=5, octree=True)


def test_utm_offsets_random_rays_both_surfaces_and_an_unsplit_voxel():
    rng = np.random.default_rng(7)
    off = np.array([5.0e6, 4.0e5, 100.0])
    U = synthetic.planar_cloud(6000, (3, 3, 2), seed=9) + off
    g = _grid({0: U[:4000], 1: U[4000:]}, 32)
    assert g._forest.nodes["depth"].max() >= 2
    # 2 000 random rays from origins inside and outside the map
    O, D = box_rays(rng, off, off + [3, 3, 2], 2000, 2.0)
    O[:200] = np.floor(O[:200])                                                      # on voxel walls
    D[:100] = DIRECTIONS[rng.integers(0, len(DIRECTIONS), 100)]
    cube, _, _ = _check(g, O, D, 8.0, "utm, cube")
    assert cube.hit.mean() >= 0.25 and (~cube.hit).mean() >= 0.25
    plane, _, _ = _check(g, O, D, 8.0, "utm, plane", surface="plane", max_variance=1e-3)
    later = plane.hit & (plane.node != cube.node)
    print(f"utm: cube {cube.hit.mean():.3f} hit, plane {plane.hit.mean():.3f}, {later.sum()} rays pass a rejected leaf")
    assert later.sum() >= 100          # the first crossed occupied leaf is rejected and a later one accepted
    planes = g.leaf_planes()
    assert np.array_equal(planes.node[plane.row[plane.hit]], plane.node[plane.hit])
    # float32 rays are widened on the host, exactly
    O32, D32 = O[:300].astype(np.float32), D[:300].astype(np.float32)
    assert_hits_equal(g.raycast(O32, D32, 8.0), g.raycast(O32.astype(np.float64), D32.astype(np.float64), 8.0), "float32")
    # one voxel of 5 000 points, never subdivided: a root that is a leaf
    B = rng.random((5000, 3))
    g0 = Grid(GridConfig(voxel_edge_length=1))
    g0.insert_points(0, B)
    O0, D0 = box_rays(rng, [0, 0, 0], [1, 1, 1], 300, 2.0)
    r0, _, _ = _check(g0, O0, D0, 5.0, "one unsplit voxel")
    assert r0.hit.any() and not r0.hit.all()
    _check(g0, O0, D0, 5.0, "one unsplit voxel, plane", surface="plane")
    # a manager: one cube, pose numbers that are not slots
    m = OctreeManager(Octree, OctreeConfig(), np.array([-4.0, -4.0, -4.0]), 8.0)
    Pm = {4: rng.uniform(-4.0, 4.0, (3000, 3)) * [1, 1, 0.2], 9: rng.uniform(-4.0, 4.0, (2000, 3)) * [1, 0.2, 1]}
    for p, X in Pm.items():
        m.insert_points(p, X)
    m.subdivide([MaxPoints(25)])
    Om, Dm = box_rays(rng, [-4, -4, -4], [4, 4, 4], 600, 3.0)
    both, _, _ = _check(m, Om, Dm, 30.0, "manager")
    only9, _, _ = _check(m, Om, Dm, 30.0, "manager, pose 9", pose_numbers=[9])
    assert not np.array_equal(both.node, only9.node)
    with pytest.raises(KeyError):
        m.raycast(Om, Dm, 30.0, pose_numbers=[5])


def test_three_poses_a_subset_and_emptied_leaves_after_ransac():
    clouds = {p: synthetic.planar_cloud(5000, (2, 2, 2), seed=6, stream=p, sigma=0.002) for p in (0, 1, 2)}
    g = _grid(clouds, 64)
    f = g._forest
    rng = np.random.default_rng(11)
    O, D = box_rays(rng, [0, 0, 0], [2, 2, 2], 1500, 1.5)
    allp, _, _ = _check(g, O, D, 8.0, "three poses")
    sub, _, _ = _check(g, O, D, 8.0, "poses 0 and 2", pose_numbers=[2, 0])
    one, _, _ = _check(g, O, D, 8.0, "pose 1, at least 4 points", pose_numbers=[1], min_points=4)
    assert not np.array_equal(allp.node, sub.node) and not np.array_equal(sub.node, one.node)
    _check(g, O, D, 8.0, "poses 0 and 2, planes", pose_numbers=[0, 2], surface="plane")
    with pytest.raises(KeyError):
        g.raycast(O, D, 8.0, pose_numbers=[7])
    # RANSAC + apply_mask: the tables are stale, the next call makes them again; emptied leaves stop being hits
    held_before = _leaf_set(f)[1]
    np.random.seed(1)
    g.map_leaf_points_cuda_ransac(poses_per_batch=3, threshold=0.01, hypotheses_number=128, initial_points_number=6)
    assert 0 < f.n_ord < 15000
    after, _, _ = _check(g, O, D, 8.0, "after RANSAC")
    assert not np.array_equal(after.node, allp.node)
    _check(g, O, D, 8.0, "after RANSAC, poses 0 and 2", pose_numbers=[0, 2])
    _check(g, O, D, 8.0, "after RANSAC, planes", surface="plane")
    g.filter([lambda pts: len(pts) >= 12])
    cube, count = _leaf_set(f)
    emptied = cube[0][(held_before > 0) & (count == 0)]
    last, _, _ = _check(g, O, D, 8.0, "after filter")
    print(f"{len(emptied)} leaves emptied, {np.isin(allp.node, emptied).sum()} rays had hit one of them")
    assert len(emptied) > 0 and np.isin(allp.node, emptied).any() and not np.isin(last.node, emptied).any()


def test_plug_types_answer_as_the_device_grid_does():
    rng = np.random.default_rng(12)
    clouds = {0: rng.uniform(-2, 4, (2500, 3)) * [1, 1, 0.2], 1: rng.uniform(0, 4, (1200, 3))}
    plug = Grid(GridConfig(octree_manager_type=HostManager, octree_type=HostOctree, octree_config=OctreeConfigBase(),
                           voxel_edge_length=2))
    dev = Grid(GridConfig(voxel_edge_length=2))
    assert plug._plug is not None
    for p, P in clouds.items():
        plug.insert_points(p, P)
        dev.insert_points(p, P)
    plug.subdivide([MaxPoints(40)])
    dev.subdivide([MaxPoints(40)])
    O, D = box_rays(rng, [-2, -2, -1], [4, 4, 4], 400, 2.0)
    pc, pe = plug.node_cubes()
    nd = dev._forest.nodes
    for sel in (None, [1]):
        a = plug.raycast(O, D, 12.0, min_range=0.5, pose_numbers=sel)
        b = dev.raycast(O, D, 12.0, min_range=0.5, pose_numbers=sel)
        assert isinstance(a, RayHits) and np.array_equal(a.t, b.t) and np.array_equal(a.hit, b.hit)
        assert 0.2 < a.hit.mean() < 0.98
        # (the two number their nodes differently: the leaf is compared by its cube)
        assert np.array_equal(pc[a.node[a.hit]], nd["corner"][b.node[b.hit]])
        assert np.array_equal(pe[a.node[a.hit]], nd["edge"][b.node[b.hit]])
    with pytest.raises(ValueError, match="voxel edges"):
        plug.raycast(O, D, 600.0)


# ---- refusals, n = 0, launch shape, nothing else disturbed -----------------------------------------------------------------
def test_refusals_empty_input_launch_shape_and_untouched_tables():
    P = synthetic.planar_cloud(20000, (3, 3, 2), seed=3)
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P[:12000])
    g.insert_points(1, P[12000:])
    f = g._forest
    lib, h = f.lib, f.handle
    rng = np.random.default_rng(7)
    O, D = box_rays(rng, [0, 0, 0], [3, 3, 2], 20000, 1.0)
    O, D = np.concatenate([O, BAD]), np.concatenate([D, np.tile([[0.0, 1.0, 0.0]], (len(BAD), 1))])
    O, Dn, tmin, tmax = ray_inputs(O, normalize_directions(D), 0.0, 10.0)
    n = len(O)
    node, t, row = np.empty(n, dtype=np.int32), np.empty(n), np.empty(n, dtype=np.int32)

    def abi(m, surface=0, min_points=1, mv=-1.0):
        return lib.octl_forest_raycast(h, nat.ptr(O), nat.ptr(Dn), nat.ptr(tmin), nat.ptr(tmax), m, None, 0, surface,
                                       min_points, mv, nat.ptr(node), nat.ptr(t), nat.ptr(row))

    assert abi(100) == nat.OCTL_E_STATE and b"before build" in lib.octl_last_error(f.ctx.handle)
    g.subdivide([MaxPoints(64)])
    Q = np.ascontiguousarray(P[:500] + 0.01)
    near = g.nearest(Q, 4, max_distance=0.3)
    planes = g.leaf_planes()
    # refusals, at the ABI and in Python
    assert abi(100, surface=2) == nat.OCTL_E_INVALID and abi(100, surface=-1) == nat.OCTL_E_INVALID
    assert abi(100, min_points=-1) == nat.OCTL_E_INVALID and abi(100, mv=float("nan")) == nat.OCTL_E_INVALID
    assert abi(-1) == nat.OCTL_E_INVALID
    with pytest.raises(ValueError, match="surface"):
        g.raycast(O[:10], D[:10], 5.0, surface="mesh")
    with pytest.raises(ValueError):
        g.raycast(O[:10], D[:9], 5.0)
    with pytest.raises(ValueError):
        g.raycast(O[:10], D[:10], np.ones(4))
    with pytest.raises(ValueError):
        g.raycast(np.zeros((4, 2)), np.zeros((4, 2)), 5.0)
    with pytest.raises(TypeError):
        g.raycast(O[:10], D[:10])
    # n = 0
    e = g.raycast(np.empty((0, 3)), np.empty((0, 3)), 5.0)
    assert e.node.shape == e.t.shape == e.row.shape == (0,) and e.node.dtype == np.int32 and e.t.dtype == np.float64
    assert abi(0) == 0
    # launch and host-wait counts with the tables in place: constant in n
    bufs = [_DevBuf(f.ctx, 24 * n), _DevBuf(f.ctx, 24 * n), _DevBuf(f.ctx, 8 * n), _DevBuf(f.ctx, 8 * n),
            _DevBuf(f.ctx, 4 * n), _DevBuf(f.ctx, 8 * n), _DevBuf(f.ctx, 4 * n)]
    for b, a in zip(bufs, (O, Dn, tmin, tmax)):
        b.upload(a)
    p = [b.p for b in bufs]

    def dev(m, surface):
        return lib.octl_forest_raycast_device(h, p[0], p[1], p[2], p[3], m, None, 0, surface, 1 if surface == 0 else 8,
                                              -1.0, p[4], p[5], p[6])

    calls = {"cube": (lambda m: abi(m), (1, 1)), "cube_device": (lambda m: dev(m, 0), (1, 0)),
             "plane": (lambda m: abi(m, 1, 8), (1, 1)), "plane_device": (lambda m: dev(m, 1), (1, 0))}
    try:
        for name, (fn, expect) in calls.items():
            assert fn(n) == 0          # (warm: staging allocated, voxel codes and the tables on the device)
            f.ctx.sync()
            for m in (100, n):
                a, b = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
                assert fn(m) == 0
                got = (_counter("octl_debug_launches") - a, _counter("octl_debug_host_syncs") - b)
                assert got == expect, (name, m, got)
            f.ctx.sync()
            # the two forms of a surface agree on all n rays (host form first: its answers are in node, t, row)
            if name.endswith("_device"):
                assert np.array_equal(bufs[4].download(n, np.int32), node) and np.array_equal(bufs[5].download(n, np.float64), t)
                assert np.array_equal(bufs[6].download(n, np.int32), row)
                assert (node >= 0).mean() > 0.25 and np.all(node[-len(BAD) + 2:-1] == -1)
    finally:
        for b in bufs:
            b.free()
    # another selection makes a new index: more than the one launch
    a = _counter("octl_debug_launches")
    g.raycast(O[:100], D[:100], 5.0, pose_numbers=[1])
    assert _counter("octl_debug_launches") - a > 1
    g.raycast(O[:100], D[:100], 5.0)                 # (back to every pose, as nearest below asks)
    # nearest and leaf_planes around the raycasts: the same bits, no launch more than a warm call makes
    g.nearest(Q, 4, max_distance=0.3)
    a, b = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
    near2 = g.nearest(Q, 4, max_distance=0.3)
    assert (_counter("octl_debug_launches") - a, _counter("octl_debug_host_syncs") - b) == (1, 1)
    for name in ("pose", "index", "distance2", "count"):
        assert getattr(near2, name).tobytes() == getattr(near, name).tobytes(), name
    g.raycast(O[:100], D[:100], 5.0, surface="plane")
    f._pooled = None
    a = _counter("octl_debug_launches")
    planes2 = g.leaf_planes()
    assert planes2 is not planes and _counter("octl_debug_launches") == a          # (the device still holds the table)
    for name in ("node", "count", "mean", "covariance", "eigenvalues", "eigenvectors"):
        assert getattr(planes2, name).tobytes() == getattr(planes, name).tobytes(), name
    # rows moved outside their leaves: a leaf's cube does not say where its points are
    g.map_leaf_points(lambda q: q + np.array([0.0, 0.0, 0.4]), [1])
    with pytest.raises(RuntimeError, match="outside their leaves"):
        g.raycast(O[:10], D[:10], 5.0)
    assert abi(100) == nat.OCTL_E_STATE and abi(100, 1, 8) == nat.OCTL_E_STATE
