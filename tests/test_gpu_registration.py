"""Scan-to-map normal equations on the device: octl_forest_registration_system (csrc/register.hip) and its Python
surface (Grid / OctreeManager / Octree: registration_system, align).

Contracts (eps = 2^-53):
 * per point: node, row and residual are the bits point_to_plane answers for transform_np(T, Q);
 * sums: every one of the 28 entries is within (D + 8) eps sum |term| of the np.longdouble sum over the terms the
   device itself selected (its per-point answers, the planes it returned), D = 16 + 6 + 3 + ceil(ceil(n / 4096) / 256)
   + 6 + 3 = the additions a term can pass through (lane, wave butterfly, four waves, fold thread, butterfly, four
   waves), 8 = the roundings of forming it (p - c, two per cross-product component, the weight's division, w J, the
   products); the two counts are exact;
 * the bits are a function of the call alone: the same call twice, and the host and the device form, agree."""

import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from octreelib_amd import MaxPoints, synthetic
from octreelib_amd import _native as nat
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree_manager import OctreeManager
from octreelib_amd.query import locate_np
from octreelib_amd.registration import (align_np, default_origin, registration_system_np, se3_exp,
                                        system_from_sums, transform_np)
from tests.test_cpu_registration import assert_recovers_motion, known_motion_scene, motion_errors
from tests.test_gpu_query import BAD, _counter, _DevBuf, _second_scan

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
CHUNK = 4096
LD = np.longdouble
_TRIU = np.triu_indices(6)


def _depth_bound(n):
    return 16 + 6 + 3 + math.ceil(math.ceil(n / CHUNK) / 256) + 6 + 3


def _sums28(s):
    return np.concatenate([np.asarray(s.H)[_TRIU], np.asarray(s.g), [s.cost]])


def _abs_term_sums(planes, p, c, row, r, max_distance, huber_delta):
    """sum |term| of each of the 28 sums in longdouble, over the points the per-point answers select."""
    used = (row >= 0) & np.isfinite(r)
    if max_distance is not None:
        used &= ~(np.abs(r) > max_distance)
    rr = r[used].astype(LD)
    nrm = planes.normal[row[used]].astype(LD).reshape(-1, 3)
    d = p[used].astype(LD) - np.asarray(c, dtype=np.float64).astype(LD)
    J = np.concatenate([np.cross(d, nrm).reshape(-1, 3), nrm], axis=1)
    w = np.ones(len(rr), dtype=LD)
    rho = rr * rr / 2
    if huber_delta is not None:
        tail = np.abs(rr) > LD(huber_delta)
        w[tail] = LD(huber_delta) / np.abs(rr[tail])
        rho[tail] = LD(huber_delta) * (np.abs(rr[tail]) - LD(huber_delta) / 2)
    out = [np.abs(w * J[:, a] * J[:, b]).sum() for a, b in zip(*_TRIU)]
    out += [np.abs(w * J[:, a] * rr).sum() for a in range(6)]
    out.append(np.abs(rho).sum())
    return np.array(out, dtype=LD), used


def _check_contract(s, Q, T, c, what, max_distance=None, huber_delta=None):
    """s: a RegistrationSystem with its per-point answers.  Counts exact, sums within the bound; returns the worst
    error / bound ratio."""
    n = len(Q)
    p = transform_np(T, Q)
    ref = registration_system_np(None, s.planes, Q, T, c, max_distance=max_distance, huber_delta=huber_delta,
                                 dtype=LD, answers=(s.node, s.row, s.residual))
    sabs, used = _abs_term_sums(s.planes, p, c, s.row, s.residual, max_distance, huber_delta)
    assert s.n_used == int(used.sum()) == ref.n_used and s.n_located == int((s.node >= 0).sum()), what
    got, want = _sums28(s).astype(LD), _sums28(ref)
    bound = (_depth_bound(n) + 8) * LD(EPS) * sabs
    err = np.abs(got - want)
    ratio = float((err / np.maximum(bound, np.finfo(LD).tiny)).max()) if n else 0.0
    print(f"{what}: n = {n}, used {s.n_used}, located {s.n_located}, worst sum error / bound = {ratio:.4f}")
    assert np.all(err <= bound), (what, n, np.nonzero(err > bound)[0], ratio)
    assert np.array_equal(s.H, s.H.T)
    return ratio


def _check_identity(obj, s, Q, T, what, **gates):
    """node, row, residual are the bits of the existing point_to_plane for the transformed scan."""
    ref = obj.point_to_plane(transform_np(T, Q), **gates)
    assert s.node.dtype == np.int32 and s.row.dtype == np.int32 and s.residual.dtype == np.float64
    assert np.array_equal(s.node, ref.node), what
    assert np.array_equal(s.row, ref.row), what
    assert np.array_equal(s.residual.view(np.uint64), ref.distance.view(np.uint64)), what


def _device_form(f, Q, T, c, per_point=False, **gates):
    """(28 sums, 2 counts[, node, row, residual]) of the device entry on uploaded points."""
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    n = len(Q)
    bufs = [_DevBuf(f.ctx, Q.nbytes), _DevBuf(f.ctx, 28 * 8), _DevBuf(f.ctx, 16)]
    if per_point:
        bufs += [_DevBuf(f.ctx, 4 * n), _DevBuf(f.ctx, 4 * n), _DevBuf(f.ctx, 8 * n)]
    try:
        if n:
            bufs[0].upload(Q)
        extra = [b.p for b in bufs[3:]] if per_point else [None, None, None]
        f.registration_system_device(bufs[0].p, n, T, c, bufs[1].p, bufs[2].p, *extra, **gates)
        out = [bufs[1].download(28, np.float64), bufs[2].download(2, np.int64)]
        if per_point:
            out += [bufs[3].download(n, np.int32), bufs[4].download(n, np.int32), bufs[5].download(n, np.float64)]
        return out
    finally:
        for b in bufs:
            b.free()


# ---- the scene of test_gpu_query.py::test_locate_planar_scene -------------------------------------------------------
T_SCENE = se3_exp([0.012, -0.02, 0.025, 0.01, -0.015, 0.005], [2.0, 2.0, 1.0])      # ~2 degrees and a small shift


@pytest.fixture(scope="module")
def scene():
    P = synthetic.planar_cloud(60000, (4, 4, 2), seed=3, sigma=0.001)
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P)
    g.subdivide([MaxPoints(64)])
    assert g._forest.nodes["depth"].max() >= 2
    S = _second_scan(P)
    # (a used point first - n = 1 is then a real term - and the rows no query may trip over right behind it)
    Q = np.concatenate([S[2000:2002], BAD, S])
    Q = np.ascontiguousarray(np.resize(Q, (70001, 3)))
    c = default_origin(T_SCENE, Q[8:20000])      # (the centroid of a scan without the 1e300 row)
    return g, Q, c


def test_per_point_identity_and_sums(scene):
    g, Q, c = scene
    n = 20008
    for gates, what in ((dict(), "plain"), (dict(max_distance=0.05), "gated"),
                        (dict(max_distance=0.2, huber_delta=0.01), "huber")):
        s = g.registration_system(Q[:n], T_SCENE, origin=c, per_point=True, **gates)
        _check_identity(g, s, Q[:n], T_SCENE, what)
        _check_contract(s, Q[:n], T_SCENE, c, what, **gates)
        assert 0.3 * n < s.n_used <= s.n_located < n, (what, s.n_used, s.n_located)
        assert np.all(s.node[2:2 + len(BAD)] == -1) and np.all(np.isfinite(s.H)) and np.isfinite(s.cost)
    plain = g.registration_system(Q[:n], T_SCENE, origin=c)
    gated = g.registration_system(Q[:n], T_SCENE, origin=c, max_distance=0.05)
    assert gated.n_used < plain.n_used and gated.n_located == plain.n_located and plain.node is None
    # min_points / max_variance gate as they do in point_to_plane
    s = g.registration_system(Q[:n], T_SCENE, origin=c, min_points=20, max_variance=1e-5, per_point=True)
    _check_identity(g, s, Q[:n], T_SCENE, "plane gates", min_points=20, max_variance=1e-5)
    _check_contract(s, Q[:n], T_SCENE, c, "plane gates")
    assert 0 < s.n_used < plain.n_used
    # the default origin is the centroid of the finite transformed points; f32 queries are widened exactly
    auto = g.registration_system(Q[8:n], T_SCENE)
    assert np.array_equal(auto.origin, default_origin(T_SCENE, Q[8:n]))
    q32 = Q[8:3000].astype(np.float32)
    a = g.registration_system(q32, T_SCENE, origin=c)
    b = g.registration_system(q32.astype(np.float64), T_SCENE, origin=c)
    assert _sums28(a).tobytes() == _sums28(b).tobytes()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193, 70001])
def test_shapes(scene, n):
    g, Q, c = scene
    s = g.registration_system(Q[:n], T_SCENE, origin=c, per_point=True)
    _check_contract(s, Q[:n], T_SCENE, c, "shape")
    dev = _device_form(g._forest, Q[:n], T_SCENE, c)
    assert dev[0].tobytes() == _sums28(s).tobytes() and dev[1].tolist() == [s.n_used, s.n_located]
    if n == 0:
        assert _sums28(s).tobytes() == np.zeros(28).tobytes() and (s.n_used, s.n_located) == (0, 0)   # (+0.0)
    if n == 1:
        # H is exactly w J J^T of that point: the device's arithmetic in exact rationals, rounded where it rounds
        assert s.n_used == 1 and s.row[0] >= 0
        fma = lambda a, b, acc: float(Fraction(a) * Fraction(b) + Fraction(acc))
        p = transform_np(T_SCENE, Q[:1])[0]
        nx, ny, nz = (float(v) for v in s.planes.normal[s.row[0]])
        dx, dy, dz = (float(v) for v in (p - c))
        J = [fma(dy, nz, -(dz * ny)), fma(dz, nx, -(dx * nz)), fma(dx, ny, -(dy * nx)), nx, ny, nz]
        r = float(s.residual[0])
        for a in range(6):
            for b in range(6):
                assert s.H[a, b] == fma(J[min(a, b)], J[max(a, b)], 0.0), (a, b)
            assert s.g[a] == fma(J[a], r, 0.0)
        assert s.cost == fma(0.5 * r, r, 0.0)


def test_fold_thread_takes_a_second_row(scene):
    g, Q, c = scene
    n = 256 * CHUNK + 1
    big = np.ascontiguousarray(np.resize(Q[:60000], (n, 3)))
    s = g.registration_system(big, T_SCENE, origin=c, max_distance=0.1, per_point=True)
    assert _depth_bound(n) == 36 and s.n_used > n // 3
    _check_contract(s, big, T_SCENE, c, "257 rows", max_distance=0.1)


def test_reproducible_and_forms_agree(scene):
    g, Q, c = scene
    n = 20008
    gates = dict(max_distance=0.1, huber_delta=0.02)
    a = g.registration_system(Q[:n], T_SCENE, origin=c, per_point=True, **gates)
    a2 = g.registration_system(Q[:n], T_SCENE, origin=c, per_point=True, **gates)
    assert _sums28(a2).tobytes() == _sums28(a).tobytes() and (a2.n_used, a2.n_located) == (a.n_used, a.n_located)
    b = g.registration_system(Q[:n], T_SCENE, origin=c, **gates)          # (the other template instance)
    assert _sums28(a).tobytes() == _sums28(b).tobytes() and (a.n_used, a.n_located) == (b.n_used, b.n_located)
    dev = _device_form(g._forest, Q[:n], T_SCENE, c, per_point=True, **gates)
    assert dev[0].tobytes() == _sums28(a).tobytes() and dev[1].tolist() == [a.n_used, a.n_located]
    assert np.array_equal(dev[2], a.node) and np.array_equal(dev[3], a.row)
    assert np.array_equal(dev[4].view(np.uint64), a.residual.view(np.uint64))
    again = system_from_sums(dev[0], dev[1], c)
    assert np.array_equal(again.H, a.H) and np.array_equal(again.g, a.g) and again.cost == a.cost


def test_multi_pose_subset_scheme_manager_and_octree():
    rng = np.random.default_rng(5)
    g = Grid(GridConfig(voxel_edge_length=2))
    clouds = [rng.uniform(-5.0, 5.0, (20000, 3)) * [1, 1, 0.02] + [0, 0, 0.5 * k] for k in range(2)]
    for p, P in enumerate(clouds):
        g.insert_points(p + 3, P)
    g.subdivide([MaxPoints(30)], pose_numbers=[3])
    T = se3_exp([0.0, 0.0, 0.035, 0.01, 0.02, 0.003], [0.0, 0.0, 0.0])
    Q = np.concatenate([_second_scan(np.vstack(clouds), 1), BAD])
    for sel in (None, [4]):
        c = default_origin(T, Q[:1000])
        s = g.registration_system(Q, T, pose_numbers=sel, origin=c, max_distance=0.3, per_point=True)
        _check_identity(g, s, Q, T, f"grid {sel}", pose_numbers=sel)
        _check_contract(s, Q, T, c, f"grid {sel}", max_distance=0.3)
        assert s.n_used > 1000 and s.planes is g.leaf_planes(sel)
    with pytest.raises(KeyError):
        g.registration_system(Q, T, pose_numbers=[9])
    # a manager and a single octree (one cube)
    m = OctreeManager(Octree, OctreeConfig(), np.array([-4.0, -4.0, -4.0]), 8.0)
    for p in (4, 9):
        m.insert_points(p, rng.uniform(-4.0, 4.0, (8000, 3)) * [1, 1, 0.01])
    m.subdivide([MaxPoints(25)])
    Qm = np.concatenate([rng.uniform(-4.5, 4.5, (6000, 3)) * [1, 1, 0.01], BAD])
    c = np.zeros(3)
    s = m.registration_system(Qm, T, pose_numbers=[9], origin=c, per_point=True)
    _check_identity(m, s, Qm, T, "manager", pose_numbers=[9])
    _check_contract(s, Qm, T, c, "manager")
    assert 0 < s.n_used and s.n_located < len(Qm)
    t = Octree(OctreeConfig(), np.zeros(3), 4.0)
    e = t.registration_system(np.ones((3, 3)))          # (no points yet: the cube is there, nothing is used)
    assert e.n_used == 0 and e.n_located == 3 and not e.H.any()
    t.insert_points(rng.random((5000, 3)) * [4.0, 4.0, 0.02] + [0, 0, 2.0])
    t.subdivide([MaxPoints(20)])
    Qt = np.concatenate([rng.random((3000, 3)) * [4.2, 4.2, 0.02] + [0, 0, 2.0], BAD])
    T1 = se3_exp([0.002, -0.001, 0.03, 0.0, 0.01, 0.002], [2.0, 2.0, 2.0])
    s = t.registration_system(Qt, T1, origin=[2.0, 2.0, 2.0], per_point=True)
    _check_identity(t, s, Qt, T1, "octree")
    _check_contract(s, Qt, T1, np.array([2.0, 2.0, 2.0]), "octree")
    assert s.n_used > 1000
    a = t.align(Qt[:-len(BAD)], T1, max_distance=0.1, max_iterations=3)
    assert a.iterations >= 1 and a.n_used > 1000 and np.all(np.isfinite(a.transform))
    # NaN and inf rows are skipped; a FINITE 1e300 drags the centroid - the origin - away: reported, not raised
    skipped = t.align(np.concatenate([Qt[:-len(BAD)], BAD[2:5]]), T1, max_distance=0.1, max_iterations=3)
    assert skipped.n_used == a.n_used
    wild = t.align(Qt, T1, max_distance=0.1)
    assert not wild.converged and wild.reason == "singular system" and np.array_equal(wild.transform, T1)


def test_launch_shape(scene):
    g, Q, c = scene
    f = g._forest
    g.leaf_planes()
    lib, h = f.lib, f.handle
    T12 = np.ascontiguousarray(T_SCENE[:3])
    cc = np.ascontiguousarray(c)
    sums, counts = np.empty(28), np.empty(2, dtype=np.int64)
    xin, s_out, c_out = _DevBuf(f.ctx, Q.nbytes), _DevBuf(f.ctx, 28 * 8), _DevBuf(f.ctx, 16)
    xin.upload(Q)
    calls = {
        "host": lambda n: lib.octl_forest_registration_system(h, nat.ptr(Q), n, nat.ptr(T12), nat.ptr(cc), 8, -1.0,
                                                              0.2, -1.0, nat.ptr(sums), nat.ptr(counts), None, None,
                                                              None),
        "device": lambda n: lib.octl_forest_registration_system_device(h, xin.p, n, nat.ptr(T12), nat.ptr(cc), 8,
                                                                       -1.0, 0.2, -1.0, s_out.p, c_out.p, None, None,
                                                                       None),
    }
    expect = {"host": (2, 1), "device": (2, 0)}
    try:
        for name, fn in calls.items():
            assert fn(len(Q)) == 0          # (warm: staging and scratch rows allocated, voxel codes on the device)
            f.ctx.sync()
            for n in (257, len(Q)):
                a, b = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
                assert fn(n) == 0
                got = (_counter("octl_debug_launches") - a, _counter("octl_debug_host_syncs") - b)
                assert got == expect[name], (name, n, got)
            f.ctx.sync()
        assert s_out.download(28, np.float64).tobytes() == sums.tobytes()
        assert c_out.download(2, np.int64).tolist() == counts.tolist()
    finally:
        for b in (xin, s_out, c_out):
            b.free()
    # one align iteration = the difference between a run of two and a run of one (tolerance 0: neither converges);
    # the scan without the rows that are finite and absurd (they would drag the centroid - the origin - to 1e296)
    clean = Q[np.all(np.abs(Q) < 100.0, axis=1)]
    assert len(clean) > 60000
    per_run = {}
    g.align(clean, T_SCENE, max_distance=0.2, max_iterations=2, tolerance=0.0)       # (warm)
    for n in (257, len(clean)):
        for iters in (1, 2):
            a, b = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
            res = g.align(clean[:n], T_SCENE, max_distance=0.2, max_iterations=iters, tolerance=0.0)
            assert res.iterations == iters and res.reason == "max_iterations"
            per_run[(n, iters)] = (_counter("octl_debug_launches") - a, _counter("octl_debug_host_syncs") - b)
        one = tuple(x - y for x, y in zip(per_run[(n, 2)], per_run[(n, 1)]))
        assert one == (2, 1), (n, per_run)
    assert per_run[(257, 1)] == per_run[(len(clean), 1)]


def test_state_and_errors():
    P = synthetic.planar_cloud(20000, (3, 3, 2), seed=3)
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P)
    g.subdivide([MaxPoints(64)])
    f = g._forest
    Q = np.ascontiguousarray(P[:1000] + 0.001)
    T12 = np.ascontiguousarray(np.eye(4)[:3])
    c = np.zeros(3)
    sums, counts = np.empty(28), np.empty(2, dtype=np.int64)
    where = g.locate(Q)

    def abi(T=T12, origin=c, n=1000):
        return f.lib.octl_forest_registration_system(f.handle, nat.ptr(Q), n, nat.ptr(T), nat.ptr(origin), 8, -1.0,
                                                     -1.0, -1.0, nat.ptr(sums), nat.ptr(counts), None,
                                                     None, None)

    def still_answers():
        assert np.array_equal(g.locate(Q), where)

    assert abi() == nat.OCTL_E_STATE and b"no pooled leaf planes" in f.lib.octl_last_error(f.ctx.handle)
    still_answers()
    g.leaf_planes()
    assert abi() == 0 and counts[0] > 500
    good = sums.copy()
    bad_T = T12.copy()
    bad_T[1, 2] = np.nan
    assert abi(T=bad_T) == nat.OCTL_E_INVALID
    still_answers()
    assert abi(origin=np.array([0.0, np.inf, 0.0])) == nat.OCTL_E_INVALID
    assert abi(n=-1) == nat.OCTL_E_INVALID and abi(n=1 << 31) == nat.OCTL_E_INVALID
    node = np.empty(1000, dtype=np.int32)        # (one per-point pointer without the other two)
    assert f.lib.octl_forest_registration_system(f.handle, nat.ptr(Q), 1000, nat.ptr(T12), nat.ptr(c), 8, -1.0, -1.0,
                                                 -1.0, nat.ptr(sums), nat.ptr(counts), nat.ptr(node), None,
                                                 None) == nat.OCTL_E_INVALID
    still_answers()
    assert abi() == 0 and sums.tobytes() == good.tobytes()
    with pytest.raises(ValueError):
        g.registration_system(Q, np.full((4, 4), np.nan))
    g.insert_points(1, P[:500] + 0.002)
    assert abi() == nat.OCTL_E_STATE and b"stale" in f.lib.octl_last_error(f.ctx.handle)
    assert len(g.locate(Q)) == 1000
    s = g.registration_system(Q)                      # (the method makes the planes again)
    assert s.n_used > 500 and abi() == 0


def test_allocation_failures_of_a_first_call():
    """The convention of tests/test_gpu_failures.py: every growth of a device buffer that a first registration_system
    call makes fails once; the call raises MemoryError with the library's message and, asked again, answers what an
    undisturbed grid answers."""
    P = synthetic.planar_cloud(20000, (3, 3, 2), seed=3)
    Q = np.ascontiguousarray(P[:9000] + 0.001)

    def arm(nth):
        seen = C.c_int64(0)
        nat.get_context().check(nat.load().octl_debug_fail_alloc(int(nth), C.byref(seen)))
        return seen.value

    def fresh():
        g = Grid(GridConfig(voxel_edge_length=1))
        g.insert_points(0, P)
        g.subdivide([MaxPoints(64)])
        g.leaf_planes()
        return g

    want = fresh().registration_system(Q, per_point=True)
    hits, nth = 0, 1
    while True:
        g = fresh()
        arm(nth)
        raised = False
        try:
            g.registration_system(Q, per_point=True)
        except MemoryError as e:
            raised = True
            assert "injected by octl_debug_fail_alloc" in str(e)
        finally:
            arm(0)
        if not raised:
            break
        hits += 1
        assert len(g.locate(Q)) == len(Q)
        got = g.registration_system(Q, per_point=True)
        assert _sums28(got).tobytes() == _sums28(want).tobytes() and got.n_used == want.n_used
        assert np.array_equal(got.residual.view(np.uint64), want.residual.view(np.uint64))
        nth += 1
        assert nth < 20
    assert hits >= 2, hits          # (the staging of the host form and the scratch rows)


# ---- align -----------------------------------------------------------------------------------------------------------
def test_align_recovers_a_known_motion_on_the_device():
    P, scan, M, centroid = known_motion_scene()
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P)
    a = g.align(scan, max_distance=0.2)
    assert_recovers_motion(a, M, centroid, len(scan))
    # the first iteration's system: the sums contract, and the host loop's first system
    f = g._forest
    planes = g.leaf_planes()
    c = default_origin(None, scan)
    first = g.registration_system(scan, None, origin=c, max_distance=0.2, per_point=True)
    assert np.abs(np.abs(first.residual[first.row >= 0]) - 0.2).min() > 1e-12      # (no point sits on the gate)
    _check_contract(first, scan, np.eye(4), c, "align, first system", max_distance=0.2)
    locate = lambda p: locate_np(f.nodes, f.voxels, f.mode, f._cube[1], p)
    seen = []

    def host_system(T, origin):
        seen.append(registration_system_np(locate, planes, scan, T, origin, max_distance=0.2))
        return seen[-1]

    host = align_np(host_system)
    assert (first.n_used, first.n_located) == (seen[0].n_used, seen[0].n_located)
    assert np.array_equal(seen[0].origin, c)
    # (both are f64 sums of ~20000 terms of one sign pattern: they agree far inside 1e-9 relative to the largest entry)
    assert np.abs(first.H - seen[0].H).max() <= 1e-9 * np.abs(seen[0].H).max()
    assert np.abs(first.g - seen[0].g).max() <= 1e-9 * np.abs(seen[0].g).max()
    assert abs(first.cost - seen[0].cost) <= 1e-9 * seen[0].cost
    assert host.converged and a.n_used == host.n_used and a.iterations == host.iterations
    assert np.abs(a.transform - host.transform).max() < 1e-7
    # everything gated out: not converged, the start comes back
    none = g.align(scan, max_distance=0.0)
    assert not none.converged and none.reason == "no correspondences" and np.array_equal(none.transform, np.eye(4))
    empty = g.align(np.empty((0, 3)))
    assert not empty.converged and empty.reason == "no correspondences" and empty.n_used == 0


def test_align_on_the_subdivided_map():
    P, scan, M, centroid = known_motion_scene()
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P)
    g.subdivide([MaxPoints(64)])
    a = g.align(scan, max_distance=0.2)
    rot0, cen0 = motion_errors(np.eye(4), M, centroid)
    rot1, cen1 = motion_errors(a.transform, M, centroid)
    print(f"subdivided map: rotation error {rot0:.4f} -> {rot1:.5f} deg, centroid error {cen0:.4f} -> {cen1:.6f}, "
          f"{a.iterations} iterations ({a.reason}), n_used {a.n_used}")
    assert a.converged
    assert rot1 < rot0 and cen1 < cen0
