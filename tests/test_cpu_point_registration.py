"""Point-to-point registration on the host: registration.point_registration_system_np (the definition of
octl_forest_point_registration_system), align_np over it, and the surface of HostMap and of the classes on the
caller's own plug types.

The scene of the recovery tests is the one the feature was proposed with: a 12^3 lattice at pitch 0.25, every point
jittered by +-0.05, stored as two poses - no leaf of it holds a plane - and a 700-point scan of it moved by a small
rigid motion (at most 0.02 rad and 0.03 m per component), max_distance 0.07."""

import re
from fractions import Fraction

import numpy as np
import pytest

import octreelib_amd
from octreelib_amd import registration as reg
from octreelib_amd.query import HostMap, Neighbours, nearest_np
from octreelib_amd.registration import (align_np, point_registration_system_np, se3_exp, system_from_sums,
                                        transform_np)

R_MAX = 0.07
LATTICE_ORIGIN = [1.375, 1.375, 1.375]
# three motions within 0.02 rad and 0.03 m per component
MOTIONS = [(0.02, -0.01, 0.015, 0.03, -0.02, 0.01), (-0.012, 0.02, 0.005, -0.03, 0.015, 0.02),
           (0.0, 0.0, 0.02, 0.01, 0.03, -0.03)]
_TRIU = np.triu_indices(6)


def lattice_scene(motion=MOTIONS[0], seed=0, n_scan=700, noise=0.0):
    """(clouds [(0, P0), (1, P1)], scan Q, T_true): transform_np(T_true, Q) lies on the stored points (up to `noise`)."""
    rng = np.random.default_rng(seed)
    t = np.arange(12) * 0.25
    P = np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(-1, 3) + rng.uniform(-0.05, 0.05, (1728, 3))
    clouds = [(0, np.ascontiguousarray(P[:900])), (1, np.ascontiguousarray(P[900:]))]
    T_true = se3_exp(motion, LATTICE_ORIGIN)
    S = P[rng.choice(len(P), n_scan, replace=False)]
    if noise:
        S = S + rng.normal(0.0, noise, S.shape)
    Q = transform_np(np.linalg.inv(T_true), S)
    return clouds, np.ascontiguousarray(Q), T_true


def sums28(s):
    return np.concatenate([np.asarray(s.H)[_TRIU], np.asarray(s.g), [s.cost]])


class _Leaf:
    def __init__(self, corner, edge, pts):
        self.corner_min, self.edge_length, self._p = np.asarray(corner, dtype=np.float64), float(edge), pts

    def get_points(self):
        return self._p


def host_map(clouds, edge=1.0):
    """A HostMap of whole voxels of `edge` as leaves, one per (voxel, pose) that holds points."""
    roots, leaves = {}, {}
    for p, P in clouds:
        v = np.floor(P / edge).astype(np.int64)
        leaves[p] = []
        for key in sorted(set(map(tuple, v.tolist()))):
            roots[key] = (np.array(key, dtype=np.float64) * edge, edge)
            leaves[p].append(_Leaf(np.array(key, dtype=np.float64) * edge, edge, P[np.all(v == key, axis=1)]))
    return HostMap(0, edge, [roots[k] for k in sorted(roots)], leaves)


# ---- exact at n = 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [None, 7.0 / 128.0])
def test_one_point_equals_the_hand_formed_system(delta):
    """n = 1: every sum has one term, so the definition must EQUAL J^T J, J^T e and rho formed by hand in rational
    arithmetic.  The inputs are dyadic with few bits, so that every f64 operation of the definition is exact: e =
    (2, 3, 6) / 64 has d2 = 49 / 4096 and sqrt(d2) = 7 / 64, and delta = 7 / 128 makes the Huber weight 1 / 2."""
    m = np.array([[0.5, 0.25, 0.75]])
    q = m + np.array([[2.0, 3.0, 6.0]]) / 64.0
    c = np.array([0.125, 0.5, 0.25])
    s = point_registration_system_np([(3, m)], q, None, c, max_distance=0.125, huber_delta=delta, per_point=True)
    assert s.n_used == 1 and s.n_located == 1 and s.neighbours.pose[0, 0] == 3 and s.neighbours.index[0, 0] == 0
    F = Fraction
    p = [F(x) for x in q[0].tolist()]
    e = [a - F(x) for a, x in zip(p, m[0].tolist())]
    d = [a - F(x) for a, x in zip(p, c.tolist())]
    d2 = sum(x * x for x in e)
    assert F(float(s.neighbours.distance2[0, 0])) == d2 == F(49, 4096)
    if delta is None:
        w, rho = F(1), d2 / 2
    else:
        assert d2 > F(delta) * F(delta)
        root = F(7, 64)
        w, rho = F(delta) / root, F(delta) * (root - F(delta) / 2)
        assert w == F(1, 2)
    J = [[F(0), d[2], -d[1], F(1), F(0), F(0)], [-d[2], F(0), d[0], F(0), F(1), F(0)],
         [d[1], -d[0], F(0), F(0), F(0), F(1)]]                     # -[d]x | I
    for a in range(6):
        for b in range(6):
            assert F(float(s.H[a, b])) == w * sum(J[k][a] * J[k][b] for k in range(3)), (a, b)
        assert F(float(s.g[a])) == w * sum(J[k][a] * e[k] for k in range(3)), a
    assert F(float(s.cost)) == rho
    assert not np.signbit(s.H[3:, 3:]).any() and not np.signbit(np.diag(s.H[:3, 3:])).any()     # (structural zeros: +0.0)


# ---- gradient, reference conditions ----------------------------------------------------------------------------------
def test_gradient_and_reference_conditions():
    clouds, Q, T_true = lattice_scene(noise=0.02, seed=2)
    delta = 0.03
    T = se3_exp([0.004, -0.003, 0.002, 0.004, 0.003, -0.005], LATTICE_ORIGIN) @ T_true
    c = np.array(LATTICE_ORIGIN)
    f = lambda X, **kw: point_registration_system_np(clouds, Q, X, c, max_distance=R_MAX, huber_delta=delta, **kw)
    s = f(T, per_point=True)
    nb = s.neighbours
    used = nb.count > 0
    d2 = nb.distance2[used, 0]
    # Huber is on and bites, and some points are beyond the gate
    assert 0 < (~used).sum() < len(Q) // 2 and (d2 > delta * delta).sum() > 20 and (d2 <= delta * delta).sum() > 20
    # reference conditions: nothing sits on a threshold, and H_vv is a multiple of the identity
    assert np.abs(d2 - R_MAX * R_MAX).min() > 1e-9 and np.abs(d2 - delta * delta).min() > 1e-9
    far = nearest_np(transform_np(T, Q), clouds, 1, max_distance=2 * R_MAX).distance2[~used, 0]
    assert np.all(far - R_MAX * R_MAX > 1e-9)
    assert s.H[3, 3] == s.H[4, 4] == s.H[5, 5] and np.all(s.H[3:, 3:][~np.eye(3, dtype=bool)] == 0.0)
    h = 1e-6
    for i in range(6):
        xi = np.zeros(6)
        xi[i] = h
        plus, minus = f(se3_exp(xi, c) @ T, per_point=True), f(se3_exp(-xi, c) @ T, per_point=True)
        # (the step moves no point across the gate: the cost is smooth between the two evaluations)
        assert np.array_equal(plus.neighbours.count, nb.count) and np.array_equal(minus.neighbours.count, nb.count)
        num = (plus.cost - minus.cost) / (2 * h)
        assert abs(num - s.g[i]) <= 1e-6 * np.abs(s.g).max(), (i, num, s.g[i])


# ---- align_np recovery ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", MOTIONS)
@pytest.mark.parametrize("delta", [None, 0.02])
def test_align_np_recovers_the_motion(motion, delta):
    clouds, Q, T_true = lattice_scene(motion)
    a = align_np(lambda T, c: point_registration_system_np(clouds, Q, T, c, max_distance=R_MAX, huber_delta=delta))
    assert a.converged and a.iterations <= 10 and a.n_used == len(Q), (a.iterations, a.reason, a.n_used)
    assert np.abs(a.transform - T_true).max() <= 1e-9
    assert a.costs[-1] <= 1e-12 * a.costs[0]


# ---- HostMap and the plug types ----------------------------------------------------------------------------------------
def test_host_map_equals_the_definition():
    clouds, Q, T_true = lattice_scene()
    hm = host_map(clouds)
    # (a HostMap knows a pose through its leaves: its clouds are the leaves' points in listing order)
    listed = hm.clouds()
    assert [p for p, _ in listed] == [0, 1] and sum(len(a) for _, a in listed) == 1728
    for sel in (None, [1]):
        got = hm.point_registration_system(Q, T_true, max_distance=R_MAX, pose_numbers=sel, huber_delta=0.02,
                                           per_point=True)
        ref = point_registration_system_np(hm.clouds(sel), Q, T_true, max_distance=R_MAX, huber_delta=0.02,
                                           per_point=True)
        assert sums28(got).tobytes() == sums28(ref).tobytes() and (got.n_used, got.n_located) == (ref.n_used,
                                                                                                  ref.n_located)
        assert isinstance(got.neighbours, Neighbours) and np.array_equal(got.neighbours.index, ref.neighbours.index)
        assert got.node is None and got.planes is None
    assert hm.point_registration_system(Q, T_true, max_distance=R_MAX, pose_numbers=[1]).n_used < len(Q)
    a = hm.align_points(Q, max_distance=R_MAX)
    assert a.converged and np.abs(a.transform - T_true).max() <= 1e-9


def test_plug_types_run_the_host_definition():
    from octreelib_amd.grid import Grid, GridConfig
    from octreelib_amd.octree.octree_base import OctreeConfigBase
    from tests.test_cpu_query import HostManager, HostOctree

    clouds, Q, T_true = lattice_scene()
    g = Grid(GridConfig(octree_manager_type=HostManager, octree_type=HostOctree, octree_config=OctreeConfigBase(),
                        voxel_edge_length=1))
    # (the voxel bucketing of the plug path's insert_points runs on the device: done in NumPy here, as
    #  tests/test_cpu_query.py does)
    for pose, P in clouds:
        vox = np.floor(P).astype(int)
        uniq, inv = np.unique(vox, axis=0, return_inverse=True)
        g._plug._pose_voxels[pose] = []
        for j, coords in enumerate(uniq):
            key = tuple(int(x) for x in coords)
            if key not in g._plug._managers:
                g._plug._managers[key] = HostManager(HostOctree, OctreeConfigBase(), np.array(coords), 1)
            g._plug._pose_voxels[pose].append(key)
            g._plug._managers[key].insert_points(pose, P[inv.reshape(-1) == j])
    s = g.point_registration_system(Q, T_true, max_distance=R_MAX, per_point=True)
    assert s.n_used == len(Q) and s.cost < 1e-25 and s.neighbours.count.sum() == len(Q)
    assert g.point_registration_system(Q, T_true, max_distance=R_MAX, pose_numbers=[1]).n_used < len(Q)
    a = g.align_points(Q, max_distance=R_MAX)
    assert a.converged and np.abs(a.transform - T_true).max() <= 1e-9
    with pytest.raises(KeyError):
        g.point_registration_system(Q, max_distance=R_MAX, pose_numbers=[9])
    with pytest.raises(TypeError):
        g.align_points(Q)


# ---- refusals, exports -----------------------------------------------------------------------------------------------
def test_refusals():
    clouds, Q, T_true = lattice_scene()
    hm = host_map(clouds)
    with pytest.raises(TypeError):
        point_registration_system_np(clouds, Q)
    with pytest.raises(TypeError):
        hm.point_registration_system(Q)
    with pytest.raises(TypeError):
        hm.align_points(Q)
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            point_registration_system_np(clouds, Q, max_distance=r)
        with pytest.raises(ValueError):
            hm.point_registration_system(Q, max_distance=r)
    with pytest.raises(ValueError, match="voxel edge"):
        hm.point_registration_system(Q, max_distance=2.5)
    with pytest.raises(ValueError, match="voxel edge"):
        hm.align_points(Q, max_distance=2.5)
    few = point_registration_system_np(clouds, Q[:5], T_true, max_distance=R_MAX)
    assert few.n_used == 5
    with pytest.raises(ValueError, match="at least 6"):
        few.solve()
    a = align_np(lambda T, c: point_registration_system_np(clouds, Q[:5], T, c, max_distance=R_MAX), T_true)
    assert not a.converged and a.reason == "no correspondences"
    # a query that is not finite is skipped, never weighted by zero
    bad = np.concatenate([Q[:50], [[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]]])
    s = point_registration_system_np(clouds, bad, T_true, np.array(LATTICE_ORIGIN), max_distance=R_MAX)
    assert s.n_used == 50 and s.n_located == 50 and np.all(np.isfinite(sums28(s)))
    e = point_registration_system_np(clouds, np.empty((0, 3)), max_distance=R_MAX)
    assert e.n_used == 0 and not sums28(e).any() and not np.signbit(sums28(e)).any()


def test_exports_and_abi_text():
    assert "point_registration_system_np" in octreelib_amd.__all__ and "point_registration_system_np" in reg.__all__
    assert octreelib_amd.point_registration_system_np is point_registration_system_np
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"\s+", " ", open(os.path.join(root, "include", "octreelib_hip.h")).read())
    for name in ("octl_forest_point_registration_system", "octl_forest_point_registration_system_device"):
        assert f"int {name}(octl_forest* f," in header
    assert "#define OCTL_ABI_VERSION 1" in header
    from octreelib_amd import _native as nat
    src = open(nat.__file__).read()
    assert '"octl_forest_point_registration_system"' in src and '"octl_forest_point_registration_system_device"' in src
    for cls in ("Grid", "OctreeManager", "Octree"):
        mod = {"Grid": "octreelib_amd.grid", "OctreeManager": "octreelib_amd.octree_manager",
               "Octree": "octreelib_amd.octree"}[cls]
        c = getattr(__import__(mod, fromlist=[cls]), cls)
        assert callable(c.point_registration_system) and callable(c.align_points)
    s = system_from_sums(np.zeros(28), (0, 0), np.zeros(3))
    assert s.neighbours is None
