"""Ray evidence on the device: octl_forest_ray_evidence / _ray_evidence_device and Grid / OctreeManager / Octree
.ray_evidence.

One contract: both counters of every node EQUAL those of the brute force octreelib_amd.query.ray_evidence_np over the
map's own leaves, in the host form and in the device form.  The counters are integer atomics, so there is no order and
no tolerance to state.  Shapes are small because brute force is the checker."""

import ctypes as C

import numpy as np
import pytest

from octreelib_amd import MaxPoints, RayEvidence, synthetic
from octreelib_amd import _native as nat
from octreelib_amd._engine import Forest
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.query import RAY_CAP_EDGES, evidence_inputs
from tests._evidence import assert_evidence_equal, evidence_of_nodes, measured
from tests._raycast import DIRECTIONS, assert_hits_equal, box_rays, lattice_points, lattice_rays
from tests.test_gpu_query import BAD, _counter, _DevBuf

pytestmark = pytest.mark.gpu


# ---- helpers -------------------------------------------------------------------------------------------------------
class _DeviceRays:
    """The five inputs of n rays and zeroed counters for N nodes in device memory."""

    def __init__(self, f: Forest, inp, N):
        n = len(inp[0])
        self.f, self.n, self.N = f, n, N
        self.bufs = [_DevBuf(f.ctx, 24 * n), _DevBuf(f.ctx, 24 * n), _DevBuf(f.ctx, 8 * n), _DevBuf(f.ctx, 8 * n),
                     _DevBuf(f.ctx, 8 * n), _DevBuf(f.ctx, 4 * N), _DevBuf(f.ctx, 4 * N)]
        for b, a in zip(self.bufs, inp):
            if n:
                b.upload(a)
        self.zero()

    def zero(self):
        for b in self.bufs[5:]:
            b.upload(np.zeros(max(self.N, 2), dtype=np.uint32))      # (a buffer has at least 8 bytes)

    def call(self, m=None, n_nodes=None):
        p = [b.p for b in self.bufs]
        return self.f.lib.octl_forest_ray_evidence_device(self.f.handle, p[0], p[1], p[2], p[3], p[4],
                                                          self.n if m is None else m, p[5], p[6],
                                                          self.N if n_nodes is None else n_nodes)

    def counters(self) -> RayEvidence:
        return RayEvidence(self.bufs[5].download(self.N, np.uint32), self.bufs[6].download(self.N, np.uint32))

    def free(self):
        for b in self.bufs:
            b.free()


def _device_form(f: Forest, inp, N) -> RayEvidence:
    dr = _DeviceRays(f, inp, N)
    try:
        assert dr.call() == 0
        return dr.counters()
    finally:
        dr.free()


def _check(obj, O, D, ranges, margin, what, min_range=0.0, returned=None):
    """Both forms of the device answer against ray_evidence_np over the map's own leaves."""
    f = obj._forest
    got = obj.ray_evidence(O, D, ranges, margin, min_range, returned)
    assert isinstance(got, RayEvidence)
    inp = evidence_inputs(O, D, ranges, margin, min_range, returned)
    nd = f.nodes
    ref = evidence_of_nodes(nd, *inp)
    assert len(got) == len(nd["edge"]) == f.n_scheme_nodes()
    assert_evidence_equal(got, ref, what + " (host form)")
    assert_evidence_equal(_device_form(f, inp, len(ref)), ref, what + " (device form)")
    inner = nd["first_child"] >= 0
    assert ref.hits[inner].sum() == 0 and ref.through[inner].sum() == 0
    return ref, inp


def _both_sizes(obj, rng, O, D, lo, hi, margin, what, **kw):
    """n = 100 and n = 20 006 (more than one workgroup, no multiple of 256) from the scene's rays, measured ranges."""
    out = None
    for n in (100, 20006):
        idx = rng.integers(0, len(O), n)
        r, ret = measured(rng, n, lo, hi)
        out, _ = _check(obj, O[idx], D[idx], r, margin, f"{what}, n = {n}", returned=ret, **kw)
    return out


def _grid(clouds, K, L=1):
    g = Grid(GridConfig(voxel_edge_length=L))
    for p, P in clouds.items():
        g.insert_points(p, P)
    g.subdivide([MaxPoints(K)])
    return g


# ---- the scenes -----------------------------------------------------------------------------------------------------------
def test_lattice_walls_and_grazing_contacts():
    g = _grid({0: lattice_points()}, 8)
    assert g._forest.nodes["depth"].max() == 2
    O, D = lattice_rays()
    rng = np.random.default_rng(0)
    r, ret = measured(rng, len(O), 0.0, 4.0)
    ref, _ = _check(g, O, D, r, 0.125, "lattice", returned=ret)
    print(f"lattice: {len(O)} rays, {int(ref.hits.sum())} hits, {int(ref.through.sum())} throughs")
    assert ref.hits.sum() > 500 and ref.through.sum() > 5000
    _check(g, O, D, r, 0.0, "lattice, margin 0")
    _check(g, O, D, r, 0.25, "lattice, blind range", min_range=0.5)
    ref = _both_sizes(g, rng, O, D, 0.0, 4.0, 0.125, "lattice")
    assert ref.hits.max() > 20


def test_sparse_grid_with_gaps_at_the_cap():
    rng = np.random.default_rng(2)
    vox = np.argwhere(rng.random((14, 14, 3)) < 0.25) * [3, 3, 2] - [20, 20, 2]      # occupied voxels with gaps between
    P = np.concatenate([v + rng.random((40, 3)) for v in vox])
    g = _grid({0: P}, 12)
    f = g._forest
    O, D = box_rays(rng, [-20, -20, -2], [22, 22, 4], 1500, 120.0)
    ref, _ = _check(g, O, D, RAY_CAP_EDGES - 0.5, 0.5, "sparse grid, range at the cap")
    assert ref.through.sum() > 300
    _check(g, O, D, 200.0 + RAY_CAP_EDGES - 1.0, 1.0, "sparse grid, the cap from min_range", min_range=200.0)
    A = np.repeat(np.array([[-30.0, 1.0, 0.5], [-30.0, -8.0, 1.0], [4.0, 40.0, 0.0], [1.5, 1.5, -40.0]]), 6, axis=0)
    Da = np.tile(DIRECTIONS[np.abs(DIRECTIONS).sum(axis=1) == 1], (4, 1))
    _check(g, A, Da, 100.0, 0.5, "sparse grid, axis rays")
    _both_sizes(g, rng, O, D, 100.0, 250.0, 0.5, "sparse grid")
    # one call above the cap: Python refuses, the ABI refuses, the device form (which cannot look) adds nothing
    with pytest.raises(ValueError, match="voxel edges"):
        g.ray_evidence(O[:50], D[:50], RAY_CAP_EDGES, 0.5)
    with pytest.raises(ValueError, match="voxel edges"):
        g.carve_rays(O[:50], D[:50], RAY_CAP_EDGES, 0.5)
    inp = evidence_inputs(O[:50], D[:50], RAY_CAP_EDGES, 0.5)
    N = f.n_scheme_nodes()
    through, hits, nn = np.zeros(N, dtype=np.uint32), np.zeros(N, dtype=np.uint32), C.c_int64(0)
    rc = f.lib.octl_forest_ray_evidence(f.handle, *[nat.ptr(a) for a in inp], 50, N, nat.ptr(through), nat.ptr(hits),
                                        C.byref(nn))
    assert rc == nat.OCTL_E_INVALID and b"voxel edges" in f.lib.octl_last_error(f.ctx.handle)
    over = _device_form(f, inp, N)
    assert over.through.sum() == 0 and over.hits.sum() == 0
    # dead rays are answered, not refused - whatever their range
    bad = g.ray_evidence(BAD[2:5], np.tile([[1.0, 0.0, 0.0]], (3, 1)), 50.0, 0.5)
    assert bad.through.sum() == 0 and bad.hits.sum() == 0
    assert g.ray_evidence(O[:4], D[:4], np.inf, 0.5).through.sum() == 0
    assert g.ray_evidence(O[:4], np.zeros((4, 3)), 9.0, 0.5).through.sum() == 0


def test_non_dyadic_octree():
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
    S = np.repeat(split[:100], 3, axis=0)
    S[:, 0] -= 5.0
    Ds = np.tile(np.array([[1.0, 0, 0], [1.0, 0.3, 0], [1.0, 0, -0.2]]), (100, 1))
    Ob, Db = box_rays(rng, [c0] * 3, [c0 + e0] * 3, 400, 2.0)
    O, D = np.concatenate([S, Ob]), np.concatenate([Ds, Db])
    r, ret = measured(rng, len(O), 1.0, 9.0)
    ref, _ = _check(t, O, D, r, 0.05, "non-dyadic octree", returned=ret)
    assert ref.hits.sum() > 100 and ref.through.sum() > 1000
    _check(t, O, D, 2e6, 1.0, "non-dyadic octree from afar", min_range=3.0)      # (one cube has no cap)
    _both_sizes(t, rng, O, D, 1.0, 9.0, 0.05, "non-dyadic octree")


def test_utm_offsets_and_an_unsplit_voxel():
    rng = np.random.default_rng(7)
    off = np.array([5.0e6, 4.0e5, 100.0])
    U = synthetic.planar_cloud(6000, (3, 3, 2), seed=9) + off
    g = _grid({0: U[:4000], 1: U[4000:]}, 32)
    assert g._forest.nodes["depth"].max() >= 2
    O, D = box_rays(rng, off, off + [3, 3, 2], 2000, 2.0)
    O[:200] = np.floor(O[:200])                                                      # on voxel walls
    D[:100] = DIRECTIONS[rng.integers(0, len(DIRECTIONS), 100)]
    r, ret = measured(rng, len(O), 0.5, 6.0)
    ref, _ = _check(g, O, D, r, 0.02, "utm", returned=ret)
    assert ref.hits.sum() > 500 and ref.through.sum() > 5000
    _both_sizes(g, rng, O, D, 0.5, 6.0, 0.02, "utm")
    # float32 rays are widened on the host, exactly
    O32, D32 = O[:300].astype(np.float32), D[:300].astype(np.float32)
    assert_evidence_equal(g.ray_evidence(O32, D32, 4.0, 0.1),
                          g.ray_evidence(O32.astype(np.float64), D32.astype(np.float64), 4.0, 0.1), "float32")
    # one voxel of 5 000 points, never subdivided: a root that is a leaf
    g0 = Grid(GridConfig(voxel_edge_length=1))
    g0.insert_points(0, rng.random((5000, 3)))
    O0, D0 = box_rays(rng, [0, 0, 0], [1, 1, 1], 300, 2.0)
    r0, _ = _check(g0, O0, D0, 1.5, 0.5, "one unsplit voxel")
    assert len(r0) == 1 and 0 < r0.hits[0] < 300 and 0 < r0.through[0] < 300


def test_one_origin_heavy_same_address_atomics_and_accumulation():
    P = synthetic.planar_cloud(12000, (3, 3, 2), seed=4)
    g = _grid({0: P}, 64)
    f = g._forest
    rng = np.random.default_rng(3)
    n = 20000
    o = P[17] + 1e-3                 # (next to a stored point: inside a leaf)
    T = rng.uniform([0, 0, 0], [3, 3, 2], (n, 3))
    O = np.tile(o, (n, 1))
    D = T - o
    r = np.sqrt((D * D).sum(axis=1))
    ref, inp = _check(g, O, D, r, 0.03, "one origin")
    # every ray leaves through the leaf of the origin (and its neighbours): thousands of adds on a few counters
    home = f.locate(o[None])[0]
    assert home >= 0
    print(f"one origin: through[home] = {ref.through[home]}, max = {ref.through.max()}, hits {int(ref.hits.sum())}")
    assert ref.through[home] > 0.9 * n and ref.hits.sum() > n // 2
    got = g.ray_evidence(O, D, r, 0.03)
    assert int(got.hits.sum()) == int(ref.hits.sum()) and int(got.through.sum()) == int(ref.through.sum())
    # the device form ADDS: twice into the same buffers doubles every counter
    dr = _DeviceRays(f, inp, len(ref))
    try:
        assert dr.call() == 0 and dr.call() == 0
        twice = dr.counters()
        assert np.array_equal(twice.through, 2 * ref.through) and np.array_equal(twice.hits, 2 * ref.hits)
        both = ref + ref
        assert np.array_equal(both.through, twice.through) and np.array_equal(both.hits, twice.hits)
    finally:
        dr.free()


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
    inp = evidence_inputs(O, D, rng.uniform(0.5, 5.0, len(O)), 0.05)
    n = len(O)
    nn = C.c_int64(-1)
    cnt = np.zeros((2, 1), dtype=np.uint32)

    def abi(m, cap=None, ptrs=None, out=True):
        a = [nat.ptr(x) for x in inp] if ptrs is None else ptrs
        cap = cnt.shape[1] if cap is None else cap
        return lib.octl_forest_ray_evidence(h, *a, m, cap, nat.ptr(cnt[0]) if out else None,
                                            nat.ptr(cnt[1]) if out else None, C.byref(nn))

    assert abi(100) == nat.OCTL_E_STATE and b"before build" in lib.octl_last_error(f.ctx.handle)
    assert lib.octl_forest_carve(h, nat.ptr(cnt[0]), nat.ptr(cnt[1]), 1, None, 0, 2, 0, None) == nat.OCTL_E_STATE
    g.subdivide([MaxPoints(64)])
    # the size query, then counters of that size
    assert abi(100, cap=0, out=False) == 0
    N = nn.value
    assert N == len(f.nodes["edge"]) == f.n_scheme_nodes() and N > 100
    cnt = np.full((2, N), 7, dtype=np.uint32)
    assert abi(100, cap=N - 1) == 0 and np.all(cnt == 7)          # (too small: nothing is written)
    Q = np.ascontiguousarray(P[:500] + 0.01)
    near = g.nearest(Q, 4, max_distance=0.3)
    planes = g.leaf_planes()
    cast = g.raycast(O[:2000], D[:2000], 6.0)
    # refusals, at the ABI and in Python
    assert abi(-1) == nat.OCTL_E_INVALID and abi(1 << 31) == nat.OCTL_E_INVALID
    for k in range(5):
        ptrs = [nat.ptr(x) for x in inp]
        ptrs[k] = None
        assert abi(100, ptrs=ptrs) == nat.OCTL_E_INVALID, k
    assert abi(100, out=False) == nat.OCTL_E_INVALID
    with pytest.raises(ValueError):
        g.ray_evidence(O[:10], D[:9], 5.0, 0.1)
    with pytest.raises(ValueError):
        g.ray_evidence(O[:10], D[:10], np.ones(4), 0.1)
    with pytest.raises(ValueError, match="margin"):
        g.ray_evidence(O[:10], D[:10], 5.0, -0.1)
    with pytest.raises(ValueError, match="margin"):
        g.ray_evidence(O[:10], D[:10], 5.0, np.nan)
    with pytest.raises(TypeError):
        g.ray_evidence(O[:10], D[:10], 5.0)
    # n = 0: zeros, no kernel
    a = _counter("octl_debug_launches")
    assert abi(0) == 0 and np.all(cnt == 0)
    e = g.ray_evidence(np.empty((0, 3)), np.empty((0, 3)), 5.0, 0.1)
    assert len(e) == N and e.through.dtype == np.uint32 and e.through.sum() == 0 and e.hits.sum() == 0
    assert _counter("octl_debug_launches") == a
    # launch and host-wait counts: constant in n (host form: one fill + one kernel, one wait; device form: one kernel)
    dr = _DeviceRays(f, inp, N)
    try:
        assert dr.call(n_nodes=N + 1) == nat.OCTL_E_INVALID and dr.call(n_nodes=0) == nat.OCTL_E_INVALID
        calls = {"host": (lambda m: abi(m), (2, 1)), "device": (lambda m: dr.call(m), (1, 0))}
        for name, (fn, expect) in calls.items():
            assert fn(n) == 0          # (warm: staging allocated, voxel codes on the device)
            f.ctx.sync()
            for m in (100, n):
                a, b = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
                assert fn(m) == 0
                got = (_counter("octl_debug_launches") - a, _counter("octl_debug_host_syncs") - b)
                assert got == expect, (name, m, got)
            f.ctx.sync()
        # the two forms agree on all n rays (the host form's answer is in cnt; the device form ran n, 100 and n rays)
        ref = evidence_of_nodes(f.nodes, *inp)
        assert_evidence_equal(RayEvidence(cnt[0], cnt[1]), ref, "host form, all rays")
        few = evidence_of_nodes(f.nodes, *[x[:100] for x in inp])
        assert_evidence_equal(dr.counters(), ref + ref + few, "device form, accumulated")
    finally:
        dr.free()
    # evidence is read-only: raycast, nearest and leaf_planes around it return the same bits, from the same tables
    g.raycast(O[:2000], D[:2000], 6.0)
    g.nearest(Q, 4, max_distance=0.3)
    a = _counter("octl_debug_launches")
    cast2 = g.raycast(O[:2000], D[:2000], 6.0)
    near2 = g.nearest(Q, 4, max_distance=0.3)
    assert _counter("octl_debug_launches") - a == 2           # (one kernel each: no table was made again)
    assert_hits_equal(cast2, cast, "raycast around ray_evidence")
    for name in ("pose", "index", "distance2", "count"):
        assert getattr(near2, name).tobytes() == getattr(near, name).tobytes(), name
    f._pooled = None
    planes2 = g.leaf_planes()
    for name in ("node", "count", "mean", "covariance", "eigenvalues", "eigenvectors"):
        assert getattr(planes2, name).tobytes() == getattr(planes, name).tobytes(), name
    # rows moved outside their leaves: the scheme alone decides, the answer stands
    before = g.ray_evidence(O[:3000], D[:3000], 4.0, 0.1)
    g.map_leaf_points(lambda q: q + np.array([0.0, 0.0, 0.4]), [1])
    with pytest.raises(RuntimeError, match="outside their leaves"):
        g.raycast(O[:10], D[:10], 5.0)
    assert_evidence_equal(g.ray_evidence(O[:3000], D[:3000], 4.0, 0.1), before, "after map_leaf_points")


def test_allocation_failures_leave_the_forest_answering():
    P = synthetic.planar_cloud(8000, (2, 2, 2), seed=8)
    rng = np.random.default_rng(9)
    O, D = box_rays(rng, [0, 0, 0], [2, 2, 2], 3000, 1.0)
    r = rng.uniform(0.5, 3.0, len(O))

    def arm(nth):
        seen = C.c_int64(0)
        nat.get_context().check(nat.load().octl_debug_fail_alloc(int(nth), C.byref(seen)))
        return seen.value

    def fresh():
        g = _grid({0: P[:5000], 1: P[5000:]}, 48)
        g._forest.ensure_built()
        return g

    g = fresh()
    want_ev = g.ray_evidence(O, D, r, 0.05)
    want_cast = g.raycast(O, D, 6.0)
    want_removed = g.carve(want_ev, 2, 0, [0])
    want_blocks = {k: v.copy() for k, v in g._forest.blocks.items()}
    assert 0 < want_removed < 5000
    ops = {"ray_evidence": lambda g: g.ray_evidence(O, D, r, 0.05),
           "carve": lambda g: g.carve(want_ev, 2, 0, [0]),
           "carve_rays": lambda g: g.carve_rays(O, D, r, 0.05, pose_numbers=[0])}
    for name, op in ops.items():
        hits, nth = 0, 1
        while True:
            g = fresh()
            arm(nth)
            raised = False
            try:
                op(g)
            except MemoryError as e:
                raised = True
                assert "injected by octl_debug_fail_alloc" in str(e)
            finally:
                arm(0)
            if not raised:
                break
            hits += 1
            # the forest answers as before, and the same request, nothing injected, completes
            assert g.n_points(0) == 5000 and g.n_points(1) == 3000
            assert_hits_equal(g.raycast(O, D, 6.0), want_cast, f"{name}, allocation {nth} failed")
            assert_evidence_equal(g.ray_evidence(O, D, r, 0.05), want_ev, f"{name}, allocation {nth} failed")
            if name != "ray_evidence":
                assert op(g) == want_removed
                for k, v in g._forest.blocks.items():
                    assert np.array_equal(v, want_blocks[k]), (name, nth, k)
            nth += 1
            assert nth < 30
        print(f"{name}: {hits} allocations failed in turn")
        assert hits >= 1, name
