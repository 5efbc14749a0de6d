"""Nearest-point-to-plane scan-to-map registration on the device: octl_forest_nearest_plane_registration_system (csrc/
register_nearest_plane.hip) and its Python surface (octreelib_amd.nearest_plane_registration_system,
align_nearest_planes over a Grid, an OctreeManager or an Octree).

Contracts (eps = 2^-53):
 * per point: neighbours has the bits of nearest(transform_np(T, Q), 1, ...); node is locate(m) of the matched stored
   point m (-1 without a match); row is point_to_plane_np(node, leaf_planes, p, ...)[0]; residual is NaN exactly where
   row is -1, otherwise within 4 eps sum |n_i (p_i - mean_i)| of the longdouble value (the bound tests/
   test_gpu_query.py holds point_to_plane to), and the bits of the device's point_to_plane(p) wherever node ==
   locate(p);
 * sums: every one of the 28 entries is within (D + 8) eps sum |term| of the np.longdouble evaluation of the
   definition with answers= the device's own per-point answers, D = 16 + 6 + 3 + ceil(ceil(n / 4096) / 256) + 6 + 3
   as tests/test_gpu_registration.py derives it (the term is the code of k_reg_partial, the tree is its tree); the
   counts are exact;
 * the bits are a function of the call alone: the same call twice, and the host and the device form, agree."""

import ctypes as C
import functools

import numpy as np
import pytest

from octreelib_amd import (MaxPoints, Neighbours, align_nearest_planes, nearest_plane_registration_system, synthetic,
                           upload_async)
from octreelib_amd import _native as nat
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree_manager import OctreeManager
from octreelib_amd.query import locate_np, nearest_np, point_to_plane_np
from octreelib_amd.registration import (align_np, nearest_plane_registration_system_np, se3_exp, transform_np)
from tests.test_cpu_nearest import lattice_case
from tests.test_cpu_nearest_plane_registration import (GAP_LEAF, GAP_R, assert_gap_geometry, gap_scene)
from tests.test_cpu_point_registration import sums28
from tests.test_gpu_point_registration import (FIELDS, T_SMALL, _assert_neighbours, _grid, _names, _same_bits)
from tests.test_gpu_point_registration import _device_form as _point_device_form
from tests.test_gpu_query import BAD, _counter, _DevBuf
from tests.test_gpu_registration import _abs_term_sums, _depth_bound
from tests.test_gpu_registration import _device_form as _own_leaf_device_form

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
LD = np.longdouble


# ---- helpers -------------------------------------------------------------------------------------------------------
def _is_octree(obj):
    return isinstance(obj, Octree)


def _kw(obj, sel):
    return {} if _is_octree(obj) else {"pose_numbers": sel}


def _system(obj, Q, T, r, sel=None, **kw):
    return nearest_plane_registration_system(obj, Q, T, max_distance=r, **_kw(obj, sel), **kw)


def _check_sums(s, Q, T, c, delta, what):
    """s: a RegistrationSystem with its per-point answers.  Counts exact, sums within the bound; returns the worst
    error / bound ratio."""
    n = len(Q)
    p = transform_np(T, Q)
    ref = nearest_plane_registration_system_np(None, s.planes, None, Q, T, c, max_distance=1.0, huber_delta=delta,
                                               dtype=LD, answers=(s.neighbours, s.node, s.row, s.residual))
    sabs, used = _abs_term_sums(s.planes, p, c, s.row, s.residual, None, delta)
    assert s.n_used == int(used.sum()) == ref.n_used, what
    assert s.n_located == int((s.node >= 0).sum()) == int((s.neighbours.count > 0).sum()) == ref.n_located, what
    got, want = sums28(s).astype(LD), sums28(ref)
    bound = (_depth_bound(n) + 8) * LD(EPS) * sabs
    err = np.abs(got - want)
    ratio = float((err / np.maximum(bound, np.finfo(LD).tiny)).max()) if n else 0.0
    print(f"{what}: n = {n}, used {s.n_used}, located {s.n_located}, worst sum error / bound = {ratio:.4f}")
    assert np.all(err <= bound), (what, n, np.nonzero(err > bound)[0], ratio)
    assert np.array_equal(s.H, s.H.T)
    return ratio


def _check_per_point(obj, s, clouds, Q, T, r, sel, mp, mv, what):
    """The per-point contract of the module docstring.  clouds: what Neighbours.index refers to.  Returns the masks
    (matched, leaf of the match is not the query's, match in another top-level voxel, matched without a plane)."""
    p = transform_np(T, Q)
    n = len(Q)
    nb = s.neighbours
    assert isinstance(nb, Neighbours)
    _assert_neighbours(nb, obj.nearest(p, 1, max_distance=r, **_kw(obj, sel)), what)
    assert s.node.dtype == np.int32 and s.row.dtype == np.int32 and s.residual.dtype == np.float64
    assert s.node.shape == s.row.shape == s.residual.shape == (n,)
    has = nb.count > 0
    m = np.zeros((n, 3))
    for k, a in clouds:
        of = has & (nb.pose[:, 0] == k)
        m[of] = a[nb.index[of, 0]]
    # (d2 of the answer is the distance to m: the index names the row that was inserted)
    d = p[has] - m[has]
    assert np.array_equal((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], nb.distance2[has, 0]), what
    node = np.full(n, -1, dtype=np.int32)
    if has.any():
        node[has] = obj.locate(m[has])
    assert np.all(node[has] >= 0) and np.array_equal(s.node, node), what
    planes = obj.leaf_planes(**({} if _is_octree(obj) else {"pose_numbers": sel}))
    assert s.planes is planes
    row, _ = point_to_plane_np(node, planes, p, mp, mv)
    assert np.array_equal(s.row, row), what
    ok = s.row >= 0
    assert np.array_equal(np.isnan(s.residual), ~ok) and np.all(np.isfinite(s.residual[ok])), what
    terms = planes.normal[s.row[ok]].astype(LD) * (p[ok].astype(LD) - planes.mean[s.row[ok]].astype(LD))
    err = np.abs(s.residual[ok].astype(LD) - terms.sum(axis=1))
    bound = 4 * EPS * np.abs(terms).sum(axis=1)
    print(f"{what}: residual error / bound, worst: "
          f"{float((err / np.maximum(bound, np.finfo(LD).tiny)).max()) if ok.any() else 0.0:.4f}")
    assert np.all(err <= bound), what
    own = obj.point_to_plane(p, **_kw(obj, sel), min_points=mp, max_variance=mv)
    same = has & (own.node == s.node)
    assert np.array_equal(s.row[same], own.row[same]), what
    assert np.array_equal(s.residual[same].view(np.uint64), own.distance[same].view(np.uint64)), what
    other_leaf = has & (own.node != s.node)
    return has, same, other_leaf, has & ~ok, m


def _device_form(f, Q, T, c, r, mp=8, mv=None, delta=None, slots=None, per_point=False):
    """(28 sums, 2 counts[, slot, index, distance2, node, row, residual]) of the device entry on uploaded points."""
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    n = len(Q)
    bufs = [_DevBuf(f.ctx, Q.nbytes), _DevBuf(f.ctx, 28 * 8), _DevBuf(f.ctx, 16)]
    kinds = [(4, np.int32), (8, np.int64), (8, np.float64), (4, np.int32), (4, np.int32), (8, np.float64)]
    if per_point:
        bufs += [_DevBuf(f.ctx, size * n) for size, _ in kinds]
    try:
        if n:
            bufs[0].upload(Q)
        extra = [b.p for b in bufs[3:]] if per_point else [None] * 6
        f.leaf_planes(slots)
        f.nearest_plane_registration_system_device(bufs[0].p, n, T, c, bufs[1].p, bufs[2].p, r, mp, mv, delta, slots,
                                                   *extra)
        out = [bufs[1].download(28, np.float64), bufs[2].download(2, np.int64)]
        if per_point:
            out += [b.download(n, dt) for b, (_, dt) in zip(bufs[3:], kinds)]
        return out
    finally:
        for b in bufs:
            b.free()


def _assert_device_form(f, s, dev, names, what):
    assert dev[0].tobytes() == sums28(s).tobytes() and dev[1].tolist() == [s.n_used, s.n_located], what
    if len(dev) > 2:
        names = np.asarray(list(names) + [-1], dtype=np.int32)
        assert np.array_equal(names[dev[2]], s.neighbours.pose[:, 0]), what
        assert np.array_equal(dev[3], s.neighbours.index[:, 0]) and np.array_equal(dev[4], s.neighbours.distance2[:, 0])
        assert np.array_equal(dev[5], s.node) and np.array_equal(dev[6], s.row), what
        assert np.array_equal(dev[7].view(np.uint64), s.residual.view(np.uint64)), what


# ---- test 1: per point and sums, after RANSAC + apply_mask and one filter; a manager with a subset; an octree -------
def test_per_point_and_sums_after_mask_and_filter():
    clouds = [(p, synthetic.planar_cloud(3000, (2, 2, 2), seed=6, stream=p, sigma=0.002)) for p in range(2)]
    g = _grid(clouds)
    f = g._forest
    assert f.nodes["depth"].max() >= 2
    np.random.seed(1)
    g.map_leaf_points_cuda_ransac(poses_per_batch=2, threshold=0.01, hypotheses_number=128, initial_points_number=6)
    g.filter([lambda pts: len(pts) >= 6])
    assert 0 < f.n_ord < 6000
    rng = np.random.default_rng(2)
    S = np.vstack([P for _, P in clouds])
    S = S[rng.permutation(len(S))[:2500]] + rng.normal(0.0, 0.01, (2500, 3))
    S[:250] += rng.uniform(-3.0, 3.0, (250, 3))
    Q = np.concatenate([transform_np(np.linalg.inv(T_SMALL), S), BAD])
    c = np.array([1.0, 1.0, 1.0])
    p = transform_np(T_SMALL, Q)
    worst = 0.0
    mp, mv = 8, 5e-6
    seen = np.zeros(5, dtype=np.int64)
    for sel, r, delta in ((None, 0.05, None), (None, 0.3, 0.01), ([1], 0.3, 0.01), ([0], 0.05, None)):
        slots = None if sel is None else [g._slots[k] for k in sel]
        what = f"poses {sel} r = {r} delta = {delta}"
        s = _system(g, Q, T_SMALL, r, sel, min_points=mp, max_variance=mv, huber_delta=delta, origin=c, per_point=True)
        has, same, other_leaf, no_plane, m = _check_per_point(g, s, clouds, Q, T_SMALL, r, sel, mp, mv, what)
        assert 0 < s.n_used < s.n_located < len(Q) - len(BAD) and not has[-len(BAD):].any()
        # the classes of query: outside every voxel yet matched, the match in a neighbouring leaf, in a neighbouring
        # voxel, a leaf whose plane fails max_variance (matched, located, not used)
        outside = g.locate(p) < 0
        other_voxel = has & np.any(np.floor(m) != np.floor(p), axis=1)
        seen += [int((outside & ~has).sum()), int((outside & has).sum()), int((other_leaf & ~other_voxel).sum()),
                 int(other_voxel.sum()), int(no_plane.sum())]
        pl = s.planes
        thick = no_plane & (pl.count[np.searchsorted(pl.node, np.maximum(s.node, 0))] >= mp)
        assert thick.sum() > 0 and s.n_located - s.n_used >= thick.sum(), what
        if delta is not None:
            ar = np.abs(s.residual[s.row >= 0])
            assert (ar > delta).sum() > 20 and (ar <= delta).sum() > 20, what
        worst = max(worst, _check_sums(s, Q, T_SMALL, c, delta, what))
        dev = _device_form(f, Q, T_SMALL, c, r, mp, mv, delta, slots, per_point=True)
        _assert_device_form(f, s, dev, _names(g), what)
        # without the per-point answers: the other instance of the kernel, the same sums
        assert _same_bits(_system(g, Q, T_SMALL, r, sel, min_points=mp, max_variance=mv, huber_delta=delta, origin=c),
                          s), what
    print(f"classes (outside unmatched, outside matched, other leaf, other voxel, no accepted plane): {seen.tolist()}; "
          f"worst sum error / bound over the settings: {worst:.4f}")
    assert np.all(seen > 0), seen
    # the default origin is the centroid of the transformed scan's finite points
    s = _system(g, Q[:-len(BAD)], T_SMALL, 0.3)
    assert np.array_equal(s.origin, transform_np(T_SMALL, Q[:-len(BAD)]).mean(axis=0))
    assert s.node is None and s.neighbours is None and s.planes is None


def test_manager_subset_and_octree():
    rng = np.random.default_rng(5)
    # a manager: one cube, pose numbers that are not slots, a subset of them
    m = OctreeManager(Octree, OctreeConfig(), np.array([-4.0, -4.0, -4.0]), 8.0)
    Pm = {4: rng.uniform(-4.0, 4.0, (3000, 3)) * [1, 1, 0.02], 9: rng.uniform(-4.0, 4.0, (2000, 3)) * [1, 0.02, 1],
          11: rng.uniform(-4.0, 4.0, (1000, 3)) * [0.02, 1, 1]}
    for k, X in Pm.items():
        m.insert_points(k, X)
    m.subdivide([MaxPoints(25)])
    clouds = list(Pm.items())
    Qm = np.concatenate([Pm[4][:400] + 0.01, Pm[9][:400] - 0.01, Pm[11][:200] + 0.02, BAD])
    T = se3_exp([0.002, -0.001, 0.003, 0.01, -0.02, 0.015], [0.0, 0.0, 0.0])
    Qm = np.concatenate([transform_np(np.linalg.inv(T), Qm[:-len(BAD)]), BAD])
    for sel, r in ((None, 0.5), ([9, 4], 0.5), ([11], 6.0)):          # (one cube has no cap on the radius)
        what = f"manager poses {sel} r = {r}"
        s = _system(m, Qm, T, r, sel, min_points=6, max_variance=1e-2, huber_delta=0.02, origin=[0.0, 0.0, 0.0],
                    per_point=True)
        chosen = clouds if sel is None else [(k, Pm[k]) for k in sorted(sel)]
        has, *_ = _check_per_point(m, s, chosen, Qm, T, r, sel, 6, 1e-2, what)
        assert set(np.unique(s.neighbours.pose[has]).tolist()) == {k for k, _ in chosen} and s.n_used > 100
        _check_sums(s, Qm, T, [0.0, 0.0, 0.0], 0.02, what)
        slots = None if sel is None else [m._slots[k] for k in sel]
        _assert_device_form(m._forest, s, _device_form(m._forest, Qm, T, [0.0, 0.0, 0.0], r, 6, 1e-2, 0.02, slots,
                                                       per_point=True), _names(m), what)
    a = align_nearest_planes(m, transform_np(np.linalg.inv(T), np.concatenate([X[:500] for X in Pm.values()])),
                             max_distance=0.5, pose_numbers=[4, 9, 11])
    # (the surface alone: the slabs are 0.16 thick and cross one another - test_the_gap_on_the_device has the recovery)
    assert a.converged and np.abs(a.transform - T).max() < 0.02
    # an octree: a cube that is not dyadic, queries on its faces and an ulp outside them
    c0, e0 = 0.1, 3.3
    t = Octree(OctreeConfig(), np.array([c0, c0, c0]), e0)
    P = c0 + rng.random((4000, 3)) * e0 * [1.0, 1.0, 0.01]
    P = P[np.all((P - c0 >= 0) & (P - c0 < e0), axis=1)]
    t.insert_points(P)
    t.subdivide([MaxPoints(20)])
    assert t._forest.nodes["depth"].max() >= 3
    face = rng.random((600, 3)) * e0 * [1.0, 1.0, 0.01] + c0
    for a in range(3):
        face[100 * a: 100 * a + 25, a] = c0
        face[100 * a + 25: 100 * a + 50, a] = np.nextafter(c0, -1.0)
        face[100 * a + 50: 100 * a + 75, a] = np.nextafter(c0 + e0, 10.0)
        face[100 * a + 75: 100 * a + 100, a] = c0 + e0 + 0.05
    Qt = np.concatenate([face, P[:500] + rng.normal(0.0, 0.01, (500, 3)), P[:100], BAD])
    To = se3_exp([0.0, 0.0, 0.001, 0.002, 0.0, 0.0], [1.7, 1.7, 0.1])
    for r in (0.15, 6.0):
        what = f"octree r = {r}"
        s = _system(t, Qt, To, r, huber_delta=0.005, origin=[1.7, 1.7, 0.1], per_point=True)
        has, same, other_leaf, _, _ = _check_per_point(t, s, [(0, P)], Qt, To, r, None, 8, None, what)
        assert other_leaf.sum() > 0 and same.sum() > 0 and not has[-len(BAD):].any()
        _check_sums(s, Qt, To, [1.7, 1.7, 0.1], 0.005, what)
        assert np.all(np.isfinite(sums28(s)))
    with pytest.raises(ValueError, match="pose_numbers"):
        nearest_plane_registration_system(t, Qt, max_distance=0.1, pose_numbers=[0])
    with pytest.raises(TypeError):
        nearest_plane_registration_system(t._forest, Qt, max_distance=0.1)
    # NaN and inf queries alone: nothing is used, no NaN reaches a sum
    s = _system(t, BAD, None, 0.25, origin=[1.7, 1.7, 0.1], per_point=True)
    assert s.n_used == 0 and s.n_located == 0 and not sums28(s).any() and np.all(s.neighbours.count == 0)
    assert np.all(s.node == -1) and np.all(s.row == -1) and np.all(np.isnan(s.residual))
    with pytest.raises(ValueError, match="at least 6"):
        s.solve()


# ---- test 2: ties ------------------------------------------------------------------------------------------------------
def test_lattice_ties():
    """The 1/8-pitch lattice with r = 1/8 (tests/test_gpu_point_registration.py): a query half-way between lattice
    points has up to eight nearest points at the same d2, pose 1 repeats every third point of pose 0 - (slot, index)
    decides which stored point, and so which leaf, answers."""
    P0, P1, Q7, _, r = lattice_case()
    clouds = [(0, P0), (1, P1)]
    g = _grid(clouds, leaf=8)
    assert g._forest.nodes["depth"].max() >= 2
    S = np.concatenate([Q7, Q7[::2] + [1.0 / 16, 0.0, 0.0], Q7[::3] + [1.0 / 16, 1.0 / 16, 1.0 / 16]])
    two = g.nearest(S, 2, max_distance=r)
    assert ((two.count == 2) & (two.distance2[:, 0] == two.distance2[:, 1])).sum() > 200      # (the ties are there)
    s = _system(g, S, None, r, min_points=2, per_point=True, origin=[1.0, 1.0, 1.0])
    has, *_ = _check_per_point(g, s, clouds, S, None, r, None, 2, None, "lattice")
    _assert_neighbours(s.neighbours, nearest_np(S, clouds, 1, max_distance=r), "lattice, the definition")
    assert has.all() and 100 < s.n_used < len(S)        # (a leaf of one lattice point has no plane at min_points = 2)
    _check_sums(s, S, None, [1.0, 1.0, 1.0], None, "lattice")


# ---- test 3: shapes --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planar_grid():
    P = synthetic.planar_cloud(20000, (3, 3, 2), seed=3)
    clouds = [(0, P[:12000]), (1, P[12000:])]
    g = _grid(clouds, leaf=64)
    rng = np.random.default_rng(7)
    Q = np.ascontiguousarray(np.concatenate([P + rng.normal(0.0, 0.01, P.shape), P, P, P[:10001]])[:70001])
    T, c = se3_exp([0.002, -0.001, 0.003, 0.01, -0.005, 0.004], [1.5, 1.5, 1.0]), [1.5, 1.5, 1.0]
    return g, clouds, P, Q, T, c


@pytest.mark.parametrize("n", [0, 1, 63, 64, 255, 256, 257, 4095, 4096, 4097])
def test_shapes(n):
    g, clouds, _, Q, T, c = _planar_grid()
    Qn = np.ascontiguousarray(Q[:n])
    s = _system(g, Qn, T, 0.2, huber_delta=0.01, origin=c, per_point=True)
    _check_per_point(g, s, clouds, Qn, T, 0.2, None, 8, None, f"n = {n}")
    _check_sums(s, Qn, T, c, 0.01, f"n = {n}")
    assert s.n_located == n and (n < 63 or s.n_used >= 0.5 * n)
    _assert_device_form(g._forest, s, _device_form(g._forest, Qn, T, c, 0.2, 8, None, 0.01), _names(g), f"n = {n}")
    if n == 0:
        assert not sums28(s).any() and not np.signbit(sums28(s)).any()
        a, b = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
        _system(g, Qn, T, 0.2, origin=c)
        assert (_counter("octl_debug_launches") - a, _counter("octl_debug_host_syncs") - b) == (0, 0)


def test_second_fold_row():
    """2^20 + 1 queries are 257 chunks: thread 0 of the fold adds two rows."""
    g, clouds, _, Q, T, c = _planar_grid()
    n = 2 ** 20 + 1
    assert _depth_bound(n) == 36
    Qn = np.ascontiguousarray(np.resize(Q[:60000], (n, 3)))
    s = _system(g, Qn, T, 0.2, huber_delta=0.01, origin=c, per_point=True)
    ref = g.nearest(transform_np(T, Qn), 1, max_distance=0.2)
    _assert_neighbours(s.neighbours, ref, "2^20 + 1 queries")
    first = _system(g, Qn[:60000], T, 0.2, huber_delta=0.01, origin=c, per_point=True)
    # (the queries repeat with period 60000, and an answer depends on its query alone)
    assert np.array_equal(s.node, np.resize(first.node, n)) and np.array_equal(s.row, np.resize(first.row, n))
    assert np.array_equal(s.residual.view(np.uint64), np.resize(first.residual, n).view(np.uint64))
    _check_sums(s, Qn, T, c, 0.01, "2^20 + 1 queries")
    assert s.n_used > 0.8 * n


# ---- test 4: reproducibility, launch shape ----------------------------------------------------------------------------
def test_reproducible_and_constant_launches():
    g, clouds, P, Q, T, c = _planar_grid()
    f = g._forest
    a = _system(g, Q, T, 0.2, huber_delta=0.01, origin=c)
    assert a.n_used > 0.8 * len(Q)
    assert _same_bits(a, _system(g, Q, T, 0.2, huber_delta=0.01, origin=c))
    dev = _device_form(f, Q, T, c, 0.2, 8, None, 0.01)
    assert dev[0].tobytes() == sums28(a).tobytes() and dev[1].tolist() == [a.n_used, a.n_located]
    xin, out = _DevBuf(f.ctx, Q.nbytes), _DevBuf(f.ctx, 256)
    try:
        xin.upload(Q)
        counts_p = C.c_void_p(out.p.value + 28 * 8)
        calls = {"host": lambda m: _system(g, Q[:m], T, 0.2, origin=c),
                 "device": lambda m: f.nearest_plane_registration_system_device(xin.p, m, T, c, out.p, counts_p, 0.2)}
        expect = {"host": (3, 1), "device": (3, 0)}
        for name, fn in calls.items():
            fn(len(Q))                  # (warm: staging allocated, voxel codes, the planes and the index on the device)
            f.ctx.sync()
            for m in (257, 70001):
                la, sa = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
                fn(m)
                got = (_counter("octl_debug_launches") - la, _counter("octl_debug_host_syncs") - sa)
                assert got == expect[name], (name, m, got)
            f.ctx.sync()
    finally:
        xin.free()
        out.free()
    # align_nearest_planes on a resident scan: 3 launches and 1 host wait per iteration, the tables made once
    S = transform_np(np.linalg.inv(T), P[:9000])
    per_run = {}
    for iters in (1, 3):
        g2 = _grid(clouds, leaf=64)
        g2.leaf_planes()
        g2.nearest(S[:10], 1, max_distance=0.2)      # (the tables of the selection exist: what is counted is the loop)
        g2._forest.ctx.sync()
        la, sa = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
        res = align_nearest_planes(g2, S, max_distance=0.2, max_iterations=iters, tolerance=0.0)
        per_run[iters] = (_counter("octl_debug_launches") - la, _counter("octl_debug_host_syncs") - sa)
        assert res.iterations == iters
    step = (per_run[3][0] - per_run[1][0], per_run[3][1] - per_run[1][1])
    assert step == (6, 2), (per_run, step)              # two more iterations: 3 launches and 1 wait each
    # ... and from cold tables: one preparation, whatever the number of iterations
    cold = {}
    for iters in (1, 3):
        g3 = _grid(clouds, leaf=64)
        g3._forest.ensure_built()
        g3._forest.ctx.sync()
        la = _counter("octl_debug_launches")
        align_nearest_planes(g3, S, max_distance=0.2, max_iterations=iters, tolerance=0.0)
        cold[iters] = _counter("octl_debug_launches") - la
    assert cold[3] - cold[1] == 6 and cold[1] > per_run[1][0], (cold, per_run)
    # a DeviceCloud is read where it lies
    dc = upload_async(S)
    res_dc = align_nearest_planes(g, dc, max_distance=0.2, max_iterations=3, tolerance=0.0)
    res_h = align_nearest_planes(g, S, max_distance=0.2, max_iterations=3, tolerance=0.0)
    assert res_dc.transform.tobytes() == res_h.transform.tobytes() and res_dc.costs == res_h.costs
    dc.release()


# ---- test 5: state and errors -----------------------------------------------------------------------------------------
def test_state_and_errors():
    P = synthetic.planar_cloud(20000, (3, 3, 2), seed=3)
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P[:12000])
    g.insert_points(1, P[12000:])
    f = g._forest
    lib, h = f.lib, f.handle
    Q = np.ascontiguousarray(P[:5000] + 0.001)
    n = len(Q)
    T12 = np.ascontiguousarray(np.eye(4)[:3])
    c = np.zeros(3)
    sums, counts = np.empty(28), np.empty(2, dtype=np.int64)
    six = (np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int64), np.empty(n), np.empty(n, dtype=np.int32),
           np.empty(n, dtype=np.int32), np.empty(n))
    none6 = (None,) * 6

    def abi(m=100, r=0.1, T=T12, origin=c, out=none6, sys=sums, sel=None, mp=8, mv=-1.0):
        return lib.octl_forest_nearest_plane_registration_system(
            h, nat.ptr(Q), m, nat.ptr(T), nat.ptr(origin), r, 0.0, nat.ptr(sel), 0 if sel is None else len(sel), mp, mv,
            nat.ptr(sys), nat.ptr(counts), *[nat.ptr(a) for a in out])

    err = lambda: lib.octl_last_error(f.ctx.handle)
    assert abi() == nat.OCTL_E_STATE and b"nearest_plane_registration_system before build" in err()
    with pytest.raises(TypeError):
        nearest_plane_registration_system(g, Q)
    g.subdivide([MaxPoints(64)])
    # no pooled table yet: refused by the C entry, whatever the scan
    assert abi() == nat.OCTL_E_STATE and b"no pooled leaf planes" in err()
    assert abi(m=0) == nat.OCTL_E_STATE and b"no pooled leaf planes" in err()
    g.leaf_planes()
    assert abi() == 0                                           # (warm: voxel codes and the index on the device)

    def state():
        f._pooled = None
        pl = g.leaf_planes()
        nb = g.nearest(Q[:500], 1, max_distance=0.1)
        return ([g.get_points(k).tobytes() for k in (0, 1)]
                + [getattr(pl, k).tobytes() for k in ("node", "count", "mean", "eigenvalues", "eigenvectors")]
                + [getattr(nb, k).tobytes() for k in FIELDS])

    before = state()
    launches = _counter("octl_debug_launches")
    for r in (0.0, -0.5, float("nan"), float("inf"), 2.0000001):
        assert abi(r=r) == nat.OCTL_E_INVALID
        with pytest.raises(ValueError):
            nearest_plane_registration_system(g, Q[:10], max_distance=r)
        with pytest.raises(ValueError):
            align_nearest_planes(g, Q[:10], max_distance=r)
    assert b"voxel edge" in err()
    bad_T = T12.copy()
    bad_T[1, 2] = np.nan
    assert abi(T=bad_T) == nat.OCTL_E_INVALID and b"transform is not finite" in err()
    assert abi(origin=np.array([0.0, np.inf, 0.0])) == nat.OCTL_E_INVALID and b"origin is not finite" in err()
    with pytest.raises(ValueError):
        nearest_plane_registration_system(g, Q[:10], bad_T, max_distance=0.1)
    assert abi(m=-1) == nat.OCTL_E_INVALID
    assert abi(m=2 ** 31) == nat.OCTL_E_INVALID
    assert abi(sys=None) == nat.OCTL_E_INVALID
    for k in range(6):                                          # (all six per-point outputs or none)
        subset = tuple(a if j != k else None for j, a in enumerate(six))
        assert abi(out=subset) == nat.OCTL_E_INVALID and b"bad nearest_plane_registration_system arguments" in err()
        only = tuple(a if j == k else None for j, a in enumerate(six))
        assert abi(out=only) == nat.OCTL_E_INVALID
    assert abi(sel=np.ones(3, dtype=np.uint8)) == nat.OCTL_E_INVALID and b"slot selection" in err()
    # the refusals of the search come first, in its order: a bad radius before a bad transform
    assert abi(r=-1.0, T=bad_T) == nat.OCTL_E_INVALID and b"max_distance" in err()
    # planes and points must come from the same poses
    one = np.array([0, 1], dtype=np.uint8)
    assert abi(sel=one) == nat.OCTL_E_STATE and b"another pose selection" in err()
    assert abi(sel=one, m=0) == nat.OCTL_E_STATE                # (whatever the scan)
    with pytest.raises(RuntimeError, match="another pose selection"):
        f.ctx.check(abi(sel=one))
    assert _counter("octl_debug_launches") == launches          # (every refusal came before anything ran)
    assert state() == before
    assert abi(sel=np.ones(2, dtype=np.uint8)) == 0             # (every pose, spelled out: the same selection)
    g.leaf_planes([1])
    assert abi(sel=one) == 0
    assert abi() == nat.OCTL_E_STATE and b"another pose selection" in err()
    s1 = nearest_plane_registration_system(g, Q, max_distance=0.1, pose_numbers=[1])     # (the function makes its table)
    s = nearest_plane_registration_system(g, Q, max_distance=0.1)
    assert 0 < s1.n_located < s.n_located and s.n_used > 0.8 * n
    assert abi(r=2.0) == 0                                      # (twice the voxel edge is allowed)
    assert abi(m=n, out=six) == 0 and counts[0] == s.n_used and counts[1] == s.n_located
    assert state() == before
    with pytest.raises(KeyError):
        nearest_plane_registration_system(g, Q[:10], max_distance=0.1, pose_numbers=[7])
    with pytest.raises(ValueError):
        nearest_plane_registration_system(g, np.zeros((4, 2)), max_distance=0.1)
    # a stale table: the contents changed after the planes were made
    g.leaf_planes()
    g.filter([lambda pts: len(pts) >= 30])
    assert abi() == nat.OCTL_E_STATE and b"stale" in err()
    assert nearest_plane_registration_system(g, Q, max_distance=0.1).n_used > 0     # (the function makes them again)
    # rows moved outside their leaves: no cube bounds what it holds
    g.map_leaf_points(lambda p: p + np.array([0.0, 0.0, 0.4]), [1])
    with pytest.raises(RuntimeError, match="outside their leaves"):
        nearest_plane_registration_system(g, Q[:10], max_distance=0.1)
    with pytest.raises(RuntimeError, match="outside their leaves"):
        align_nearest_planes(g, Q[:10], max_distance=0.1)
    assert abi() == nat.OCTL_E_STATE


def test_allocation_failures_leave_the_map_usable():
    """octl_debug_fail_alloc swept over every growth of a first call (the planes, staging, scratch, the block index),
    each on a map of its own.  After a failure the map answers as before, and the retried call equals the undisturbed
    one."""
    P = synthetic.planar_cloud(8000, (2, 2, 2), seed=3)
    Q = np.ascontiguousarray(P[:3000] + 0.001)

    def arm(nth):
        seen = C.c_int64(0)
        nat.get_context().check(nat.load().octl_debug_fail_alloc(int(nth), C.byref(seen)))
        return seen.value

    def fresh():
        g = _grid([(0, P[:5000]), (1, P[5000:])], leaf=64)
        g._forest.ensure_built()
        return g

    want = nearest_plane_registration_system(fresh(), Q, max_distance=0.1, per_point=True)
    hits = 0
    for nth in range(1, 60):
        g = fresh()
        arm(nth)
        raised = False
        try:
            nearest_plane_registration_system(g, Q, max_distance=0.1, per_point=True)
        except MemoryError as e:
            raised = True
            assert "injected by octl_debug_fail_alloc" in str(e)
        finally:
            arm(0)
        if not raised:
            break
        hits += 1
        assert len(g.locate(Q)) == len(Q)
        again = nearest_plane_registration_system(g, Q, max_distance=0.1, per_point=True)
        assert _same_bits(again, want) and np.array_equal(again.neighbours.index, want.neighbours.index)
        assert np.array_equal(again.node, want.node) and np.array_equal(again.row, want.row)
    assert not raised and hits >= 3, hits


# ---- test 6: the gap -----------------------------------------------------------------------------------------------------
def test_the_gap_on_the_device():
    clouds, Q, T_true, patch = gap_scene()
    g = _grid(clouds, leaf=GAP_LEAF)
    f = g._forest
    assert_gap_geometry(clouds, Q, T_true, patch, g.locate, f.nodes["edge"])
    err = lambda a: float(np.abs(a.transform - T_true).max())
    a = align_nearest_planes(g, Q, max_distance=GAP_R)
    print(f"device: {a.iterations} iterations, {a.reason}, n_used {a.n_used}, error {err(a):.2e}, costs {a.costs}")
    assert a.converged and a.reason == "converged" and a.n_used > 0.7 * len(Q) and err(a) <= 1e-9
    # the NumPy alignment over the device's own tables
    planes = g.leaf_planes()
    locate = lambda X: locate_np(f.nodes, f.voxels, f.mode, f._cube[1], X)
    ref = align_np(lambda T, c: nearest_plane_registration_system_np(locate, planes, clouds, Q, T, c,
                                                                     max_distance=GAP_R))
    assert ref.converged and np.abs(a.transform - ref.transform).max() <= 1e-9 and a.iterations == ref.iterations
    dc = upload_async(Q)
    b = align_nearest_planes(g, dc, max_distance=GAP_R)
    dc.release()
    assert b.transform.tobytes() == a.transform.tobytes() and b.iterations == a.iterations
    one = align_nearest_planes(g, Q, max_distance=GAP_R, pose_numbers=[1], min_points=5)
    assert one.converged and err(one) <= 1e-9
    # the plane of the query's own leaf has nothing to hold on to at this start
    s0 = g.registration_system(Q)
    no = g.align(Q)
    print(f"own leaf: n_used at the start {s0.n_used}, {no.iterations} iterations, {no.reason}, error {err(no):.2e}")
    assert s0.n_used < 6 or err(no) > 1e-3


# ---- test 7: untouched paths ---------------------------------------------------------------------------------------------
def test_other_queries_are_untouched():
    P = synthetic.planar_cloud(20000, (3, 3, 2), seed=3)
    g = _grid([(0, P[:12000]), (1, P[12000:])], leaf=64)
    f = g._forest
    rng = np.random.default_rng(8)
    Q = np.ascontiguousarray(np.concatenate([P[:4000] + rng.normal(0.0, 0.01, (4000, 3)), BAD]))

    def snapshot():
        f._pooled = None
        planes = g.leaf_planes()
        f.ctx.sync()
        out, launches = [], []
        for fn in (lambda: g.nearest(Q, 1, max_distance=0.3), lambda: g.nearest(Q, 8, max_distance=0.3),
                   lambda: g.registration_system(Q, T_SMALL, max_distance=0.1, huber_delta=0.02, origin=[1.5, 1.5, 1.0],
                                                 per_point=True),
                   lambda: g.point_registration_system(Q, T_SMALL, max_distance=0.3, huber_delta=0.02,
                                                       origin=[1.5, 1.5, 1.0], per_point=True)):
            fn()                        # (warm: the tables of the selection exist)
            a = _counter("octl_debug_launches")
            out.append(fn())
            launches.append(_counter("octl_debug_launches") - a)
        bits = [getattr(planes, k).tobytes() for k in ("node", "count", "mean", "covariance", "eigenvalues",
                                                       "eigenvectors")]
        bits += [getattr(nb, k).tobytes() for nb in (out[0], out[1], out[3].neighbours) for k in FIELDS]
        bits += [sums28(out[2]).tobytes(), out[2].node.tobytes(), out[2].row.tobytes(), out[2].residual.tobytes()]
        bits += [sums28(out[3]).tobytes()]
        return bits, launches

    before, launches_before = snapshot()
    assert launches_before == [1, 1, 2, 3]
    nearest_plane_registration_system(g, Q, T_SMALL, max_distance=0.3, huber_delta=0.02, per_point=True)
    nearest_plane_registration_system(g, Q, T_SMALL, max_distance=0.2, pose_numbers=[1])
    align_nearest_planes(g, Q[:-len(BAD)], max_distance=0.2, max_iterations=2)
    after, launches_after = snapshot()
    assert after == before and launches_after == launches_before


# ---- test 8: one driver, three layouts -----------------------------------------------------------------------------------
def test_three_systems_take_turns_on_one_map():
    """The three systems go through one host driver and lay out the same two buffers of the map differently: the
    staging of the host forms holds 0, 3 or 6 per-point columns behind the queries, the scratch holds records or none.
    Called in rotation on ONE map - both forms, with and without the per-point answers, at n = 257 (a second pass of
    the lanes), then 4097 (a second chunk row), then 1 (a call that shrinks after the buffers grew) - every answer has
    the bits the same call gives on a fresh map of the same contents: the 28 sums, the 2 counts and every per-point
    column.  No tolerance."""
    _, clouds, _, Q, T, c = _planar_grid()
    r, delta = 0.2, 0.01

    def host(f, system, Qn, per_point):
        if system == "own leaf":
            s = f.registration_system(Qn, T, origin=c, max_distance=r, huber_delta=delta, per_point=per_point)
            cols = [s.node, s.row, s.residual]
        elif system == "point":
            s = f.point_registration_system(Qn, T, origin=c, max_distance=r, huber_delta=delta, per_point=per_point)
            cols = [getattr(s.neighbours, k) for k in FIELDS] if per_point else []
        else:
            s = f.nearest_plane_registration_system(Qn, T, origin=c, max_distance=r, huber_delta=delta,
                                                    per_point=per_point)
            cols = ([getattr(s.neighbours, k) for k in FIELDS] if per_point else []) + [s.node, s.row, s.residual]
        return [sums28(s), np.array([s.n_used, s.n_located])] + (cols if per_point else [])

    def device(f, system, Qn, per_point):
        if system == "own leaf":
            f.leaf_planes(None)
            return _own_leaf_device_form(f, Qn, T, c, per_point, max_distance=r, huber_delta=delta)
        if system == "point":
            return _point_device_form(f, Qn, T, c, r, delta, None, per_point)
        return _device_form(f, Qn, T, c, r, 8, None, delta, None, per_point)

    shared = _grid(clouds, leaf=64)._forest
    calls = 0
    for n in (257, 4097, 1):
        Qn = np.ascontiguousarray(Q[:n])
        for form in (host, device):
            for per_point in (False, True):
                for system in ("own leaf", "point", "nearest plane"):
                    what = (system, form.__name__, per_point, n)
                    got = form(shared, system, Qn, per_point)
                    want = form(_grid(clouds, leaf=64)._forest, system, Qn, per_point)
                    assert len(got) == len(want) and (len(got) > 2) == per_point, what
                    for k, (a, b) in enumerate(zip(got, want)):
                        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k)
                    assert n == 1 or 0 < got[1][0] <= got[1][1] <= n, (what, got[1])      # (used, located)
                    calls += 1
    assert calls == 36
