"""Point-to-point scan-to-map registration on the device: octl_forest_point_registration_system (csrc/
register_points.hip) and its Python surface (Grid / OctreeManager / Octree: point_registration_system, align_points).

Contracts (eps = 2^-53):
 * per point: pose, index, distance2 and count EQUAL nearest_np(transform_np(T, Q), stored points, k=1) - the order
   (d2, slot, index) is total, so there is no tolerance to state;
 * sums: every one of the 28 entries is within (D + 8) eps sum |term| of the np.longdouble evaluation of the
   definition over the device's own per-point answers.  D = 16 + 6 + 3 + ceil(ceil(n / 4096) / 256) + 6 + 3 = the
   additions a term can pass through (the tree of k_reg_partial, unchanged); 8 = the roundings of forming a term: 7 at
   most (csrc/reg_point_term.h counts them per sum) and one for their second-order products.  A term is a product that
   enters a sum: w d_y e_z and w d_z e_y are two terms of g_w, w d_y^2 and w d_z^2 two of H_ww(0, 0) - so a
   cancellation inside a cross product is covered.  The structural zeros have the bound 0.  The counts are exact;
 * the bits are a function of the call alone: the same call twice, and the host and the device form, agree."""

import ctypes as C
import functools
import math

import numpy as np
import pytest

from octreelib_amd import MaxPoints, Neighbours, nearest_np, synthetic
from octreelib_amd import _native as nat
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree_manager import OctreeManager
from octreelib_amd.registration import align_np, point_registration_system_np, se3_exp, transform_np
from tests.test_cpu_nearest import lattice_case
from tests.test_cpu_point_registration import LATTICE_ORIGIN, MOTIONS, R_MAX, lattice_scene, sums28
from tests.test_gpu_query import BAD, _counter, _DevBuf

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
CHUNK = 4096
K_ROUNDINGS = 8
LD = np.longdouble
FIELDS = ("pose", "index", "distance2", "count")


def _depth_bound(n):
    return 16 + 6 + 3 + math.ceil(math.ceil(n / CHUNK) / 256) + 6 + 3


def _names(obj):
    return [p for p, _ in sorted(obj._slots.items(), key=lambda kv: kv[1])]


def _abs_term_sums(clouds, p, c, nb, delta):
    """sum |term| of each of the 28 sums in longdouble, over the points the per-point answers select."""
    used = nb.count > 0
    pose, index = nb.pose[used, 0], nb.index[used, 0]
    m = np.empty((int(used.sum()), 3))
    for k, a in clouds:
        m[pose == k] = a[index[pose == k]]
    e = np.abs((p[used] - m).astype(LD))
    d = np.abs(p[used].astype(LD) - np.asarray(c, dtype=np.float64).astype(LD))
    d2 = nb.distance2[used, 0]
    w = np.ones(len(d2), dtype=LD)
    rho = d2.astype(LD) / 2
    if delta is not None:
        tail = d2 > np.float64(delta) * np.float64(delta)
        s = np.sqrt(d2[tail].astype(LD))
        w[tail] = LD(delta) / s
        rho[tail] = LD(delta) * (s - LD(delta) / 2)
    x, y, z = (w * d[:, 0]).sum(), (w * d[:, 1]).sum(), (w * d[:, 2]).sum()
    sq = lambda a, b: (w * d[:, a] * d[:, b]).sum()
    cr = lambda a, b: (w * (d[:, a] * e[:, b] + d[:, b] * e[:, a])).sum()
    W, zero = w.sum(), LD(0)
    return np.array([sq(1, 1) + sq(2, 2), sq(0, 1), sq(0, 2), zero, z, y,
                     sq(0, 0) + sq(2, 2), sq(1, 2), z, zero, x,
                     sq(0, 0) + sq(1, 1), y, x, zero,
                     W, zero, zero, W, zero, W,
                     cr(1, 2), cr(2, 0), cr(0, 1), (w * e[:, 0]).sum(), (w * e[:, 1]).sum(), (w * e[:, 2]).sum(),
                     rho.sum()], dtype=LD)


def _check_sums(s, clouds, Q, T, c, delta, what):
    """s: a RegistrationSystem with its neighbours, `clouds` what their index refers to.  Counts exact, sums within the
    bound; returns the worst error / bound ratio."""
    n = len(Q)
    p = transform_np(T, Q)
    nb = s.neighbours
    ref = point_registration_system_np(clouds, Q, T, c, max_distance=1.0, huber_delta=delta, dtype=LD, answers=nb)
    assert s.n_used == int((nb.count > 0).sum()) == ref.n_used, what
    assert s.n_located == int(np.all(np.isfinite(p), axis=1).sum()) == ref.n_located, what
    got, want = sums28(s).astype(LD), sums28(ref)
    bound = (_depth_bound(n) + K_ROUNDINGS) * LD(EPS) * _abs_term_sums(clouds, p, c, nb, delta)
    err = np.abs(got - want)
    assert np.all(err <= bound), (what, n, np.nonzero(err > bound)[0], got[err > bound], want[err > bound])
    live = bound > 0
    ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
    print(f"{what}: n = {n}, used {s.n_used}, located {s.n_located}, worst sum error / bound = {ratio:.4f}")
    assert np.array_equal(s.H, s.H.T) and s.H[3, 3] == s.H[4, 4] == s.H[5, 5]
    zeros = np.array([s.H[0, 3], s.H[1, 4], s.H[2, 5], s.H[3, 4], s.H[3, 5], s.H[4, 5]])
    assert not zeros.any() and not np.signbit(zeros).any(), what
    return ratio


def _assert_neighbours(got, ref, what):
    assert isinstance(got, Neighbours)
    for name in FIELDS:
        a, b = getattr(got, name), getattr(ref, name)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, a.shape, b.dtype, b.shape)
        if not np.array_equal(a, b):
            bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
            i = int(bad[0])
            raise AssertionError(f"{what}: {name} differs in {len(bad)} of {len(a)} rows, first {i}: got "
                                 f"{[getattr(got, f)[i].tolist() for f in FIELDS]}, expected "
                                 f"{[getattr(ref, f)[i].tolist() for f in FIELDS]}")


def _device_form(f, Q, T, c, r, delta=None, slots=None, per_point=False):
    """(28 sums, 2 counts[, slot, index, distance2]) of the device entry on uploaded points."""
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    n = len(Q)
    bufs = [_DevBuf(f.ctx, Q.nbytes), _DevBuf(f.ctx, 28 * 8), _DevBuf(f.ctx, 16)]
    if per_point:
        bufs += [_DevBuf(f.ctx, 4 * n), _DevBuf(f.ctx, 8 * n), _DevBuf(f.ctx, 8 * n)]
    try:
        if n:
            bufs[0].upload(Q)
        extra = [b.p for b in bufs[3:]] if per_point else [None, None, None]
        f.point_registration_system_device(bufs[0].p, n, T, c, bufs[1].p, bufs[2].p, r, delta, slots, *extra)
        out = [bufs[1].download(28, np.float64), bufs[2].download(2, np.int64)]
        if per_point:
            out += [bufs[3].download(n, np.int32), bufs[4].download(n, np.int64), bufs[5].download(n, np.float64)]
        return out
    finally:
        for b in bufs:
            b.free()


def _same_bits(a, b):
    return sums28(a).tobytes() == sums28(b).tobytes() and (a.n_used, a.n_located) == (b.n_used, b.n_located)


def _grid(clouds, leaf=32, edge=1):
    g = Grid(GridConfig(voxel_edge_length=edge))
    for p, P in clouds:
        g.insert_points(p, P)
    g.subdivide([MaxPoints(leaf)])
    return g


T_SMALL = se3_exp([0.01, -0.015, 0.02, 0.008, -0.01, 0.004], [1.0, 1.0, 1.0])


# ---- test 1: per-point identity and sums, after RANSAC + apply_mask and one filter --------------------------------
def test_identity_and_sums_after_mask_and_filter():
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
    for sel, r, delta in ((None, 0.05, None), (None, 0.3, 0.02), ([1], 0.3, 0.02), ([0], 0.05, None)):
        chosen = clouds if sel is None else [clouds[k] for k in sel]
        slots = None if sel is None else [g._slots[k] for k in sel]
        what = f"poses {sel} r = {r} delta = {delta}"
        # the definition over the points that are left, its indices mapped back to rows of the inserted clouds
        keep = [np.sort(_survivor_rows(f, g._slots[k])) for k, _ in chosen]
        ref = nearest_np(p, [(k, P[keep[j]]) for j, (k, P) in enumerate(chosen)], 1, max_distance=r)
        for j, (k, _) in enumerate(chosen):
            of = ref.pose == k
            ref.index[of] = keep[j][ref.index[of]]
        s = g.point_registration_system(Q, T_SMALL, max_distance=r, pose_numbers=sel, huber_delta=delta, origin=c,
                                        per_point=True)
        _assert_neighbours(s.neighbours, ref, what)
        assert 0 < s.n_used < len(Q) - len(BAD) and np.all(s.neighbours.count[-len(BAD):] == 0)
        assert s.n_located == len(Q) - 3            # (1e300 and -2^31 stay finite under T; NaN and the infinities do not)
        worst = max(worst, _check_sums(s, clouds, Q, T_SMALL, c, delta, what))
        dev = _device_form(f, Q, T_SMALL, c, r, delta, slots, per_point=True)
        assert dev[0].tobytes() == sums28(s).tobytes() and dev[1].tolist() == [s.n_used, s.n_located], what
        names = np.asarray(_names(g) + [-1], dtype=np.int32)
        assert np.array_equal(names[dev[2]], ref.pose[:, 0]) and np.array_equal(dev[3], ref.index[:, 0])
        assert np.array_equal(dev[4], ref.distance2[:, 0])
        # without the per-point answers: the other instance of the kernel, the same sums
        assert _same_bits(g.point_registration_system(Q, T_SMALL, max_distance=r, pose_numbers=sel, huber_delta=delta,
                                                      origin=c), s), what
    print(f"worst sum error / bound over the settings: {worst:.4f}")
    # the default origin is the centroid of the transformed scan's finite points
    s = g.point_registration_system(Q[:-len(BAD)], T_SMALL, max_distance=0.3)
    assert np.array_equal(s.origin, transform_np(T_SMALL, Q[:-len(BAD)]).mean(axis=0))


def _survivor_rows(f, slot):
    off = np.concatenate([[0], np.cumsum(f.slot_sizes)])
    f._perm = None
    perm = f.perm
    return perm[(perm >= off[slot]) & (perm < off[slot + 1])] - off[slot]


# ---- test 2: ties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moved", [False, True])
def test_lattice_ties(moved):
    """The 1/8-pitch lattice with r = 1/8: a query half-way between lattice points has up to eight nearest points at
    the same d2, pose 1 repeats every third point of pose 0 - (slot, index) decides, as in the definition.  Every
    coordinate, the quarter turn and the shift are exact in f64."""
    P0, P1, Q7, _, r = lattice_case()
    clouds = [(0, P0), (1, P1)]
    g = _grid(clouds, leaf=8)
    assert g._forest.nodes["depth"].max() >= 2
    T, Tinv = np.eye(4), np.eye(4)
    if moved:
        T[:2, :2] = [[0.0, -1.0], [1.0, 0.0]]       # a quarter turn about z ...
        T[:3, 3] = [2.0 - 1.0 / 16, 1.0 / 16, 1.0 / 16]      # ... back into the lattice's box, shifted by 1/16
        Tinv[:3, :3] = T[:3, :3].T
        Tinv[:3, 3] = -(T[:3, :3].T @ T[:3, 3])       # (exact: every entry is dyadic)
    # queries on lattice points (a tie between the poses) and half-way between them (ties between points)
    S = np.concatenate([Q7, Q7[::2] + [1.0 / 16, 0.0, 0.0], Q7[::3] + [1.0 / 16, 1.0 / 16, 1.0 / 16]])
    Q = transform_np(Tinv, S)
    p = transform_np(T, Q)
    assert np.array_equal(p, S)
    ref = nearest_np(p, clouds, 1, max_distance=r)
    two = nearest_np(p, clouds, 2, max_distance=r)
    assert ((two.count == 2) & (two.distance2[:, 0] == two.distance2[:, 1])).sum() > 200      # (the ties are there)
    s = g.point_registration_system(Q, T, max_distance=r, per_point=True, origin=[1.0, 1.0, 1.0])
    _assert_neighbours(s.neighbours, ref, f"lattice moved={moved}")
    _check_sums(s, clouds, Q, T, [1.0, 1.0, 1.0], None, f"lattice moved={moved}")


# ---- test 3: shapes --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lattice_grid():
    clouds, Q, T_true = lattice_scene(n_scan=1728)
    return _grid(clouds, leaf=16), clouds, Q, T_true


@pytest.mark.parametrize("n", [0, 1, 255, 257, 4097])
def test_shapes(n):
    g, clouds, Q, T_true = _lattice_grid()
    Qn = np.ascontiguousarray(np.resize(Q, (n, 3))) if n else np.empty((0, 3))
    T = se3_exp([0.003, 0.0, -0.002, 0.004, -0.003, 0.0], LATTICE_ORIGIN) @ T_true
    s = g.point_registration_system(Qn, T, max_distance=R_MAX, huber_delta=0.01, origin=LATTICE_ORIGIN, per_point=True)
    _assert_neighbours(s.neighbours, nearest_np(transform_np(T, Qn), clouds, 1, max_distance=R_MAX), f"n = {n}")
    _check_sums(s, clouds, Qn, T, LATTICE_ORIGIN, 0.01, f"n = {n}")
    assert s.n_used >= 0.9 * n and s.n_located == n
    dev = _device_form(g._forest, Qn, T, LATTICE_ORIGIN, R_MAX, 0.01)
    assert dev[0].tobytes() == sums28(s).tobytes() and dev[1].tolist() == [s.n_used, s.n_located]
    if n == 0:
        assert not sums28(s).any() and not np.signbit(sums28(s)).any()
        a, b = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
        g.point_registration_system(Qn, T, max_distance=R_MAX)
        assert (_counter("octl_debug_launches") - a, _counter("octl_debug_host_syncs") - b) == (0, 0)


def test_second_fold_row():
    """2^20 + 1 queries are 257 chunks: thread 0 of the fold adds two rows.  The map is 64 points in one voxel, so the
    definition is one (n, 64) distance matrix."""
    rng = np.random.default_rng(3)
    P = rng.random((64, 3))
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P)
    g.subdivide([MaxPoints(16)])
    n = 2 ** 20 + 1
    Q = np.ascontiguousarray(P[rng.integers(0, 64, n)] + rng.normal(0.0, 0.05, (n, 3)))
    r, delta, c = 0.1, 0.04, [0.5, 0.5, 0.5]
    s = g.point_registration_system(Q, None, max_distance=r, huber_delta=delta, origin=c, per_point=True)
    assert _depth_bound(n) == 36
    best = np.empty(n, dtype=np.int64)
    d2 = np.empty(n)
    for a in range(0, n, 1 << 16):
        q = Q[a: a + (1 << 16)]
        dx, dy, dz = (q[:, None, k] - P[None, :, k] for k in range(3))
        m = (dx * dx + dy * dy) + dz * dz
        best[a: a + len(q)] = m.argmin(axis=1)        # (the first of equal minima: the smaller index)
        d2[a: a + len(q)] = m[np.arange(len(q)), best[a: a + len(q)]]
    hit = d2 <= r * r
    nb = s.neighbours
    assert np.array_equal(nb.count, hit.astype(np.int32)) and np.array_equal(nb.index[:, 0], np.where(hit, best, -1))
    assert np.array_equal(nb.distance2[:, 0], np.where(hit, d2, np.inf)) and 0.3 < hit.mean() < 0.99
    _check_sums(s, [(0, P)], Q, None, c, delta, "2^20 + 1 queries")


# ---- test 4: reproducibility, launch shape ----------------------------------------------------------------------------
def test_reproducible_and_constant_launches():
    P = synthetic.planar_cloud(20000, (3, 3, 2), seed=3)
    clouds = [(0, P[:12000]), (1, P[12000:])]
    g = _grid(clouds, leaf=64)
    f = g._forest
    rng = np.random.default_rng(7)
    Q = np.ascontiguousarray(np.concatenate([P + rng.normal(0.0, 0.01, P.shape), P, P, P[:10001]])[:70001])
    T, c = se3_exp([0.002, -0.001, 0.003, 0.01, -0.005, 0.004], [1.5, 1.5, 1.0]), [1.5, 1.5, 1.0]
    a = g.point_registration_system(Q, T, max_distance=0.2, huber_delta=0.02, origin=c)
    assert a.n_used > 0.8 * len(Q)
    assert _same_bits(a, g.point_registration_system(Q, T, max_distance=0.2, huber_delta=0.02, origin=c))
    dev = _device_form(f, Q, T, c, 0.2, 0.02)
    assert dev[0].tobytes() == sums28(a).tobytes() and dev[1].tolist() == [a.n_used, a.n_located]
    xin, out = _DevBuf(f.ctx, Q.nbytes), _DevBuf(f.ctx, 256)
    try:
        xin.upload(Q)
        counts_p = C.c_void_p(out.p.value + 28 * 8)
        calls = {"host": lambda m: g.point_registration_system(Q[:m], T, max_distance=0.2, origin=c),
                 "device": lambda m: f.point_registration_system_device(xin.p, m, T, c, out.p, counts_p, 0.2)}
        expect = {"host": (3, 1), "device": (3, 0)}
        for name, fn in calls.items():
            fn(len(Q))                  # (warm: staging allocated, voxel codes and the index on the device)
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
    # align_points on a resident scan: 3 launches and 1 host wait per iteration, the index made once
    S = transform_np(np.linalg.inv(T), P[:9000])
    per_run = {}
    for iters in (1, 3):
        g2 = _grid(clouds, leaf=64)
        g2._forest.ensure_built()
        g2.nearest(S[:10], 1, max_distance=0.2)         # (the index of the selection exists: what is counted is the loop)
        g2._forest.ctx.sync()
        la, sa = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
        res = g2.align_points(S, max_distance=0.2, max_iterations=iters, tolerance=0.0)
        per_run[iters] = (_counter("octl_debug_launches") - la, _counter("octl_debug_host_syncs") - sa)
        assert res.iterations == iters
    step = (per_run[3][0] - per_run[1][0], per_run[3][1] - per_run[1][1])
    assert step == (6, 2), (per_run, step)              # two more iterations: 3 launches and 1 wait each
    # ... and from a cold index: one preparation, whatever the number of iterations
    cold = {}
    for iters in (1, 3):
        g3 = _grid(clouds, leaf=64)
        g3._forest.ensure_built()
        g3._forest.ctx.sync()
        la = _counter("octl_debug_launches")
        g3.align_points(S, max_distance=0.2, max_iterations=iters, tolerance=0.0)
        cold[iters] = _counter("octl_debug_launches") - la
    assert cold[3] - cold[1] == 6 and cold[1] > per_run[1][0], (cold, per_run)
    # a DeviceCloud is read where it lies
    from octreelib_amd import upload_async
    dc = upload_async(S)
    res_dc = g.align_points(dc, max_distance=0.2, max_iterations=3, tolerance=0.0)
    res_h = g.align_points(S, max_distance=0.2, max_iterations=3, tolerance=0.0)
    assert res_dc.transform.tobytes() == res_h.transform.tobytes() and res_dc.costs == res_h.costs
    dc.release()


# ---- test 5: geometry edges -------------------------------------------------------------------------------------------
def test_geometry_edges():
    rng = np.random.default_rng(5)
    # a cube that is not dyadic, queries on its faces and an ulp outside them
    c0, e0 = 0.1, 3.3
    t = Octree(OctreeConfig(), np.array([c0, c0, c0]), e0)
    P = c0 + rng.random((4000, 3)) * e0 * [1.0, 1.0, 0.3]
    P = P[np.all((P - c0 >= 0) & (P - c0 < e0), axis=1)]
    t.insert_points(P)
    t.subdivide([MaxPoints(20)])
    assert t._forest.nodes["depth"].max() >= 3
    face = rng.random((600, 3)) * e0 * [1.0, 1.0, 0.3] + c0
    for a in range(3):
        face[100 * a: 100 * a + 25, a] = c0
        face[100 * a + 25: 100 * a + 50, a] = np.nextafter(c0, -1.0)
        face[100 * a + 50: 100 * a + 75, a] = np.nextafter(c0 + e0, 10.0)
        face[100 * a + 75: 100 * a + 100, a] = c0 + e0 + 0.05
    Qt = np.concatenate([face, P[:500] + rng.normal(0.0, 0.01, (500, 3)), P[:100], BAD])
    T = se3_exp([0.0, 0.0, 0.001, 0.002, 0.0, 0.0], [1.7, 1.7, 0.6])
    for r in (0.15, 6.0):                      # (one cube has no cap on the radius)
        s = t.point_registration_system(Qt, T, max_distance=r, huber_delta=0.05, origin=[1.7, 1.7, 0.6],
                                        per_point=True)
        _assert_neighbours(s.neighbours, nearest_np(transform_np(T, Qt), [(0, P)], 1, max_distance=r), f"octree r={r}")
        _check_sums(s, [(0, P)], Qt, T, [1.7, 1.7, 0.6], 0.05, f"octree r={r}")
        assert np.all(s.neighbours.count[-len(BAD):] == 0) and np.all(np.isfinite(sums28(s)))
    a = t.align_points(transform_np(np.linalg.inv(T), P[:800]), max_distance=0.1)
    assert a.converged and np.abs(a.transform - T).max() <= 1e-9
    # UTM magnitudes with an explicit origin
    off = np.array([5.0e6, 4.0e5, 100.0])
    U = synthetic.planar_cloud(5000, (2, 2, 2), seed=9) + off
    gu = _grid([(0, U)], leaf=48)
    Qu = np.concatenate([U[:1500] + rng.normal(0.0, 0.01, (1500, 3)), BAD])
    cu = off + [1.0, 1.0, 1.0]
    Tu = se3_exp([0.0005, -0.0005, 0.001, 0.003, 0.002, -0.001], cu)
    s = gu.point_registration_system(Qu, Tu, max_distance=0.25, huber_delta=0.02, origin=cu, per_point=True)
    _assert_neighbours(s.neighbours, nearest_np(transform_np(Tu, Qu), [(0, U)], 1, max_distance=0.25), "utm")
    _check_sums(s, [(0, U)], Qu, Tu, cu, 0.02, "utm")
    assert s.n_used > 1000 and np.linalg.cond(s.H) < 1e6
    # NaN and inf queries alone: nothing is used, no NaN reaches a sum
    s = gu.point_registration_system(BAD, None, max_distance=0.25, origin=cu, per_point=True)
    assert s.n_used == 0 and s.n_located == 3 and not sums28(s).any() and np.all(s.neighbours.count == 0)
    with pytest.raises(ValueError, match="at least 6"):
        s.solve()
    # a manager: one cube, pose numbers that are not slots
    m = OctreeManager(Octree, OctreeConfig(), np.array([-4.0, -4.0, -4.0]), 8.0)
    Pm = {4: rng.uniform(-4.0, 4.0, (3000, 3)) * [1, 1, 0.2], 9: rng.uniform(-4.0, 4.0, (2000, 3)) * [1, 0.2, 1]}
    for k, X in Pm.items():
        m.insert_points(k, X)
    m.subdivide([MaxPoints(25)])
    Qm = np.concatenate([Pm[4][:300] + 0.01, Pm[9][:300] - 0.01, BAD])
    s = m.point_registration_system(Qm, None, max_distance=0.5, per_point=True, origin=[0.0, 0.0, 0.0])
    _assert_neighbours(s.neighbours, nearest_np(Qm, [(4, Pm[4]), (9, Pm[9])], 1, max_distance=0.5), "manager")
    assert {4, 9} <= set(np.unique(s.neighbours.pose).tolist())
    s9 = m.point_registration_system(Qm, None, max_distance=0.5, pose_numbers=[9], per_point=True)
    _assert_neighbours(s9.neighbours, nearest_np(Qm, [(9, Pm[9])], 1, max_distance=0.5), "manager, pose 9")


# ---- test 6: state and errors -----------------------------------------------------------------------------------------
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
    slot, index, d2 = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int64), np.empty(n)

    def abi(m=100, r=0.1, T=T12, origin=c, out=(None, None, None), sys=sums):
        return lib.octl_forest_point_registration_system(h, nat.ptr(Q), m, nat.ptr(T), nat.ptr(origin), r, 0.0, None,
                                                         0, nat.ptr(sys), nat.ptr(counts), *[nat.ptr(a) for a in out])

    err = lambda: lib.octl_last_error(f.ctx.handle)
    assert abi() == nat.OCTL_E_STATE and b"point_registration_system before build" in err()
    with pytest.raises(TypeError):
        g.point_registration_system(Q)
    g.subdivide([MaxPoints(64)])
    assert abi() == 0                                           # (warm: voxel codes and the index on the device)
    launches = _counter("octl_debug_launches")
    for r in (0.0, -0.5, float("nan"), float("inf"), 2.0000001):
        assert abi(r=r) == nat.OCTL_E_INVALID
        with pytest.raises(ValueError):
            g.point_registration_system(Q[:10], max_distance=r)
        with pytest.raises(ValueError):
            g.align_points(Q[:10], max_distance=r)
    assert b"voxel edge" in err()
    bad_T = T12.copy()
    bad_T[1, 2] = np.nan
    assert abi(T=bad_T) == nat.OCTL_E_INVALID and b"transform is not finite" in err()
    assert abi(origin=np.array([0.0, np.inf, 0.0])) == nat.OCTL_E_INVALID and b"origin is not finite" in err()
    with pytest.raises(ValueError):
        g.point_registration_system(Q[:10], bad_T, max_distance=0.1)
    assert abi(m=-1) == nat.OCTL_E_INVALID
    assert abi(sys=None) == nat.OCTL_E_INVALID
    for subset in ((slot, None, None), (slot, index, None), (None, index, d2)):
        assert abi(out=subset) == nat.OCTL_E_INVALID and b"bad point_registration_system arguments" in err()
    assert _counter("octl_debug_launches") == launches          # (every refusal came before anything ran)
    assert abi(r=2.0) == 0                                      # (twice the voxel edge is allowed)
    assert abi(m=n, out=(slot, index, d2)) == 0 and counts[0] > 0.9 * n
    with pytest.raises(KeyError):
        g.point_registration_system(Q[:10], max_distance=0.1, pose_numbers=[7])
    with pytest.raises(ValueError):
        g.point_registration_system(np.zeros((4, 2)), max_distance=0.1)
    # rows moved outside their leaves: no cube bounds what it holds
    g.map_leaf_points(lambda p: p + np.array([0.0, 0.0, 0.4]), [1])
    with pytest.raises(RuntimeError, match="outside their leaves"):
        g.point_registration_system(Q[:10], max_distance=0.1)
    with pytest.raises(RuntimeError, match="outside their leaves"):
        g.align_points(Q[:10], max_distance=0.1)
    assert abi() == nat.OCTL_E_STATE


def test_allocation_failures_leave_the_map_usable():
    """octl_debug_fail_alloc swept over every growth of a first call (staging, scratch, the block index), each on a
    map of its own.  After a failure the map answers as before, and the retried call equals the undisturbed one."""
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

    want = fresh().point_registration_system(Q, max_distance=0.1, per_point=True)
    hits = 0
    for nth in range(1, 40):
        g = fresh()
        arm(nth)
        raised = False
        try:
            g.point_registration_system(Q, max_distance=0.1, per_point=True)
        except MemoryError as e:
            raised = True
            assert "injected by octl_debug_fail_alloc" in str(e)
        finally:
            arm(0)
        if not raised:
            break
        hits += 1
        assert len(g.locate(Q)) == len(Q)
        again = g.point_registration_system(Q, max_distance=0.1, per_point=True)
        assert _same_bits(again, want) and np.array_equal(again.neighbours.index, want.neighbours.index)
    assert not raised and hits >= 3, hits


# ---- test 7: align_points where align has nothing to hold on to ---------------------------------------------------------
@pytest.mark.parametrize("motion", MOTIONS)
def test_align_points_on_a_map_without_planes(motion):
    clouds, Q, T_true = lattice_scene(motion)
    g = _grid(clouds, leaf=16)
    # no leaf holds an accepted plane at max_variance 1e-6: align has no system to solve - the gap this closes
    planes = g.leaf_planes()
    assert not ((planes.count >= 8) & (planes.eigenvalues[:, 0] <= 1e-6)).any()
    assert g.registration_system(Q, max_variance=1e-6).n_used == 0
    with pytest.raises(ValueError, match="at least 6"):
        g.registration_system(Q, max_variance=1e-6).solve()
    no = g.align(Q, max_variance=1e-6)
    assert not no.converged and no.reason == "no correspondences" and np.array_equal(no.transform, np.eye(4))
    for delta in (None, 0.02):
        a = g.align_points(Q, max_distance=R_MAX, huber_delta=delta)
        ref = align_np(lambda T, c: point_registration_system_np(clouds, Q, T, c, max_distance=R_MAX,
                                                                 huber_delta=delta))
        assert a.converged and a.reason == "converged" and a.n_used == len(Q)
        assert np.abs(a.transform - T_true).max() <= 1e-9
        assert np.abs(a.transform - ref.transform).max() <= 1e-9 and a.iterations == ref.iterations
        print(f"motion {motion} delta {delta}: {a.iterations} iterations, |T - T_true| = "
              f"{np.abs(a.transform - T_true).max():.2e}, costs {a.costs}")
    one = g.align_points(Q, max_distance=R_MAX, pose_numbers=[1])
    assert one.n_used < len(Q)


# ---- test 8: untouched paths ---------------------------------------------------------------------------------------------
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
                                                 per_point=True)):
            fn()                        # (warm: the tables of the selection exist)
            a = _counter("octl_debug_launches")
            out.append(fn())
            launches.append(_counter("octl_debug_launches") - a)
        bits = [getattr(planes, k).tobytes() for k in ("node", "count", "mean", "covariance", "eigenvalues",
                                                       "eigenvectors")]
        bits += [getattr(nb, k).tobytes() for nb in out[:2] for k in FIELDS]
        bits += [sums28(out[2]).tobytes(), out[2].node.tobytes(), out[2].row.tobytes(), out[2].residual.tobytes()]
        return bits, launches

    before, launches_before = snapshot()
    assert launches_before == [1, 1, 2]
    g.point_registration_system(Q, T_SMALL, max_distance=0.3, huber_delta=0.02, per_point=True)
    g.point_registration_system(Q, T_SMALL, max_distance=0.2, pose_numbers=[1])
    g.align_points(Q[:-len(BAD)], max_distance=0.2, max_iterations=2)
    after, launches_after = snapshot()
    assert after == before and launches_after == launches_before
