"""CPU-only checks of the registration definition (octreelib_amd/registration.py): the sums of registration_system_np
against finite differences of its own residuals, the gates, align_np on a scene with a known motion, and the two new
C entries in the header and the signature table.

Finite differences.  r is affine in v and analytic in w with a third derivative bounded by |d| (d = p - origin, |n| =
1), so a central difference with step h has a truncation error of about h^2 |d| / 6 per residual derivative; the
rounding error of a difference of two f64 values of size s is about eps s / h.  With h = 1e-6, |d| <= 2 and
eps = 1.1e-16: truncation ~ 1e-12 and rounding ~ 1e-10 (s ~ 1 for the residual's terms, s = cost for the gradient)
against derivatives of order 1 - both far inside the asserted 1e-7 relative (to the largest entry of g, of H)."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from octreelib_amd import synthetic
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree.octree_base import OctreeConfigBase
from octreelib_amd.query import locate_np, node_table_from_leaves, pooled_leaf_statistics_np
from octreelib_amd.registration import (Alignment, RegistrationSystem, align_np, registration_system_np, se3_exp,
                                        transform_np)
from tests.test_cpu_query import HostManager, HostOctree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H_STEP = 1e-6
# (the non-finite and out-of-domain rows of tests/test_gpu_query.py)
BAD = np.array([[1e300, 0.0, 0.0], [0.0, -2.0 ** 31, 0.0], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5],
                [0.5, 0.5, -np.inf], [-777.5, 3.0, 3.0]])

ENTRIES = {
    "octl_forest_registration_system":
        "int octl_forest_registration_system(octl_forest* f, const double* xyz, int64_t n, const double T[12], "
        "const double origin[3], int32_t min_points, double max_variance, double max_distance, double huber_delta, "
        "double sys[28], int64_t counts[2], int32_t* node, int32_t* row, double* residual)",
    "octl_forest_registration_system_device":
        "int octl_forest_registration_system_device(octl_forest* f, const double* xyz_dev, int64_t n, "
        "const double T[12], const double origin[3], int32_t min_points, double max_variance, double max_distance, "
        "double huber_delta, double* sys_dev, int64_t* counts_dev, int32_t* node_dev, int32_t* row_dev, "
        "double* residual_dev)",
}


# ---- maps ------------------------------------------------------------------------------------------------------------
class _CubeMap:
    """One cube [0, 2)^3 holding one plane: the smallest map there is."""

    def __init__(self):
        rng = np.random.default_rng(4)
        xy = rng.uniform(0.2, 1.8, (400, 2))
        self.normal = np.array([0.2, -0.3, 1.0]) / np.linalg.norm([0.2, -0.3, 1.0])
        z = 1.0 - (self.normal[0] * (xy[:, 0] - 1.0) + self.normal[1] * (xy[:, 1] - 1.0)) / self.normal[2]
        self.points = np.column_stack([xy, z + rng.normal(0.0, 1e-3, 400)])
        self.nodes, _ = node_table_from_leaves([(np.zeros(3), 2.0)], [(np.zeros(3), 2.0)])
        self.planes = pooled_leaf_statistics_np([[(0, self.points)]])

    def locate(self, p):
        return locate_np(self.nodes, np.zeros((1, 3), dtype=int), 1, 2.0, p)

    def system(self, Q, T=None, origin=None, **kw):
        return registration_system_np(self.locate, self.planes, Q, T, origin, **kw)

    def scan(self, n=300, lift=0.03):
        """Points near the plane, well inside the cube, a few centimetres off it."""
        rng = np.random.default_rng(5)
        xy = rng.uniform(0.5, 1.5, (n, 2))
        z = 1.0 - (self.normal[0] * (xy[:, 0] - 1.0) + self.normal[1] * (xy[:, 1] - 1.0)) / self.normal[2]
        return np.column_stack([xy, z + lift + rng.normal(0.0, 0.02, n)])


def _plug_grid(clouds, L=1):
    """A Grid on the caller's own (host) octree types.  The one step of the plug path that runs on the device is the
    voxel bucketing of insert_points; here it is done in NumPy (as tests/test_cpu_query.py does)."""
    g = Grid(GridConfig(octree_manager_type=HostManager, octree_type=HostOctree, octree_config=OctreeConfigBase(),
                        voxel_edge_length=L))
    assert g._plug is not None
    for pose, P in clouds.items():
        vox = (np.floor_divide(P, float(L)) * L).astype(int)
        uniq, inv = np.unique(vox, axis=0, return_inverse=True)
        g._plug._pose_voxels[pose] = []
        for j, coords in enumerate(uniq):
            key = tuple(int(c) for c in coords)
            if key not in g._plug._managers:
                g._plug._managers[key] = HostManager(HostOctree, OctreeConfigBase(), np.array(coords), L)
            g._plug._pose_voxels[pose].append(key)
            g._plug._managers[key].insert_points(pose, P[inv.reshape(-1) == j])
    return g


# ---- derivatives -----------------------------------------------------------------------------------------------------
def _check_derivatives(system, Q, T, origin, **gates):
    """system(Q, T, origin, per_point=..., **gates) -> RegistrationSystem.  g against the central-difference gradient
    of the cost, and - without Huber weights - H against sum J J^T with J from differences of the residuals."""
    base = system(Q, T, origin, per_point=True, **gates)
    assert base.n_used > 50
    c = base.origin
    used = (base.row >= 0) & np.isfinite(base.residual)
    if gates.get("max_distance") is not None:
        used &= np.abs(base.residual) <= gates["max_distance"]
    assert used.sum() == base.n_used
    grad = np.zeros(6)
    J = np.zeros((int(used.sum()), 6))
    for k in range(6):
        e = np.zeros(6)
        e[k] = H_STEP
        plus = system(Q, se3_exp(e, c) @ T, c, per_point=True, **gates)
        minus = system(Q, se3_exp(-e, c) @ T, c, per_point=True, **gates)
        for s in (plus, minus):      # (the perturbation moves no point to another leaf or across a gate)
            assert np.array_equal(s.node, base.node) and np.array_equal(s.row, base.row) and s.n_used == base.n_used
        grad[k] = (plus.cost - minus.cost) / (2 * H_STEP)
        J[:, k] = (plus.residual[used] - minus.residual[used]) / (2 * H_STEP)
    assert np.abs(base.g).max() > 0
    assert np.abs(base.g - grad).max() <= 1e-7 * np.abs(base.g).max(), (base.g, grad)
    if gates.get("huber_delta") is None:
        Hfd = J.T @ J
        assert np.abs(base.H - Hfd).max() <= 1e-7 * np.abs(base.H).max()
        assert np.array_equal(base.H, base.H.T)
        assert np.isclose(base.cost, 0.5 * float((base.residual[used] ** 2).sum()), rtol=1e-13, atol=0)
    return base


def test_sums_against_finite_differences_one_cube():
    m = _CubeMap()
    Q = m.scan()
    T = se3_exp([0.01, -0.015, 0.02, 0.004, -0.003, 0.002], [1.0, 1.0, 1.0])
    base = _check_derivatives(m.system, Q, T, None)
    assert base.n_used == base.n_located == len(Q)
    assert np.allclose(base.origin, transform_np(T, Q).mean(axis=0), rtol=0, atol=1e-15)
    _check_derivatives(m.system, Q, T, [0.7, 1.2, 0.9])                        # another origin: another J, same rule
    _check_derivatives(m.system, Q, T, None, huber_delta=0.03)                 # g is the gradient of the Huber cost
    # r is affine in v: a shift of 0.05 along the normal moves every residual by 0.05 (to rounding)
    shifted = m.system(Q, se3_exp(np.concatenate([np.zeros(3), 0.05 * m.planes.normal[0]])) @ T, base.origin,
                       per_point=True)
    assert np.abs(shifted.residual - base.residual - 0.05).max() < 1e-15


def test_sums_against_finite_differences_plug_grid():
    P = synthetic.planar_cloud(8000, (2, 2, 1), seed=3, sigma=0.002, inlier_fraction=1.0)
    g = _plug_grid({0: P})
    hm = g._host_map()
    assert len(hm.voxels) == 4
    S = synthetic.planar_cloud(1500, (2, 2, 1), seed=3, stream=1, sigma=0.002, inlier_fraction=1.0)
    # (points within 2 mm of a voxel face could change voxel under the perturbation: the test is about derivatives)
    frac = S - np.floor(S)
    S = S[np.all((frac > 0.01) & (frac < 0.99), axis=1)]
    T = se3_exp([0.002, -0.001, 0.003, 0.004, -0.003, 0.005], S.mean(axis=0))
    fr = transform_np(T, S) - np.floor(transform_np(T, S))
    S = S[np.all((fr > 0.005) & (fr < 0.995), axis=1)]
    planes = hm.leaf_planes()

    def system(Q, T, origin, **kw):
        return registration_system_np(hm.locate, planes, Q, T, origin, **kw)

    base = _check_derivatives(system, S, T, None, max_distance=0.5)
    assert len(np.unique(base.node)) == 4
    # the class answers what the definition answers
    got = g.registration_system(S, T, max_distance=0.5, per_point=True)
    assert isinstance(got, RegistrationSystem) and np.array_equal(got.H, base.H) and np.array_equal(got.g, base.g)
    assert got.cost == base.cost and (got.n_used, got.n_located) == (base.n_used, base.n_located)
    assert np.array_equal(got.residual, base.residual, equal_nan=True) and got.planes is not None


# ---- gates -----------------------------------------------------------------------------------------------------------
def _same_sums(a: RegistrationSystem, b: RegistrationSystem):
    return (np.array_equal(a.H, b.H) and np.array_equal(a.g, b.g) and a.cost == b.cost and a.n_used == b.n_used
            and a.n_located == b.n_located)


def test_bad_queries_change_no_sum():
    m = _CubeMap()
    Q = m.scan(100)
    c = [1.0, 1.0, 1.0]
    clean = m.system(Q, None, c)
    mixed = m.system(np.concatenate([BAD[:3], Q[:50], BAD[3:], Q[50:]]), None, c, per_point=True)
    assert _same_sums(clean, mixed) and np.all(np.isfinite(mixed.H)) and np.isfinite(mixed.cost)
    assert np.all(mixed.node[:3] == -1) and np.all(np.isnan(mixed.residual[:3]))
    # a point outside the cube is not located; one inside a leaf without an accepted plane is located and unused
    out = m.system(np.concatenate([Q, [[2.5, 1.0, 1.0]]]), None, c)
    assert _same_sums(clean, out)
    thin = m.system(Q, None, c, min_points=401)
    assert thin.n_used == 0 and thin.n_located == len(Q)
    # the default origin is the centroid of the FINITE transformed points
    assert np.array_equal(m.system(np.concatenate([Q, BAD[2:5]])).origin, m.system(Q).origin)


def test_max_distance_and_huber_are_exact_at_the_threshold():
    m = _CubeMap()
    Q = m.scan(200)
    c = [1.0, 1.0, 1.0]
    full = m.system(Q, None, c, per_point=True)
    r = full.residual
    assert np.all(np.isfinite(r))
    order = np.argsort(np.abs(r))
    delta = float(np.abs(r[order[120]]))             # a residual of the scan IS the threshold
    inside = np.abs(r) <= delta
    assert inside.sum() == 121
    gated = m.system(Q, None, c, max_distance=delta)
    kept = m.system(Q[inside], None, c)                         # (the same terms in the same order)
    assert np.allclose(gated.H, kept.H, rtol=1e-13, atol=1e-15) and np.allclose(gated.g, kept.g, rtol=1e-13, atol=1e-15)
    assert np.isclose(gated.cost, kept.cost, rtol=1e-13, atol=0)
    assert gated.n_used == 121 and gated.n_located == 200
    assert m.system(Q, None, c, max_distance=np.nextafter(delta, 0.0)).n_used == 120
    # Huber: weight 1 up to and AT delta, delta / |r| beyond; cost r^2 / 2, delta (|r| - delta / 2) beyond
    hub = m.system(Q, None, c, huber_delta=delta)
    nrm = m.planes.normal[0]
    d = Q - np.asarray(c)
    J = np.concatenate([np.cross(d, nrm), np.tile(nrm, (len(Q), 1))], axis=1)
    w = np.where(inside, 1.0, delta / np.abs(r))
    rho = np.where(inside, r * r / 2, delta * (np.abs(r) - delta / 2))
    assert np.allclose(hub.H, (J * w[:, None]).T @ J, rtol=1e-13, atol=0)
    assert np.allclose(hub.g, (J * (w * r)[:, None]).sum(axis=0), rtol=1e-12, atol=1e-16)
    assert np.isclose(hub.cost, rho.sum(), rtol=1e-13, atol=0)
    at = order[120]
    one = m.system(Q[at:at + 1], None, c, huber_delta=delta)      # the point at the threshold alone: unit weight
    assert one.cost == r[at] * r[at] / 2 and np.array_equal(one.H, np.outer(J[at], J[at]))
    beyond = m.system(Q[order[121]:order[121] + 1], None, c, huber_delta=delta)
    rb = abs(r[order[121]])
    assert beyond.cost == delta * (rb - delta / 2) and beyond.cost < rb * rb / 2
    assert hub.n_used == 200


def test_everything_gated_out():
    m = _CubeMap()
    Q = m.scan(50)
    s = m.system(Q, None, None, max_distance=0.0)
    assert s.n_used == 0 and s.n_located == 50 and s.cost == 0
    assert not s.H.any() and not s.g.any() and s.H.shape == (6, 6) and s.g.shape == (6,)
    with pytest.raises(ValueError):
        s.solve()
    with pytest.raises(ValueError):
        m.system(Q[:5]).solve()           # five points do not determine six unknowns
    start = se3_exp([0.0, 0.0, 0.01, 0.1, 0.0, 0.0])
    a = align_np(lambda T, c: m.system(Q, T, c, max_distance=0.0), start)
    assert isinstance(a, Alignment) and not a.converged and a.reason == "no correspondences"
    assert a.iterations == 0 and a.n_used == 0 and a.costs == [] and np.array_equal(a.transform, start)
    e = m.system(np.empty((0, 3)))
    assert e.n_used == 0 and not e.H.any()
    for bad in (np.full((4, 4), np.nan), np.eye(3), np.ones((4, 4))):
        with pytest.raises(ValueError):
            m.system(Q, bad)


# ---- align_np recovers a known motion --------------------------------------------------------------------------------
def known_motion_scene():
    """(map cloud, moved scan, the motion M that was taken out of the scan, the scan's centroid before it moved)."""
    P = synthetic.planar_cloud(60000, (4, 4, 2), seed=3, sigma=0.002, inlier_fraction=1.0)
    S = synthetic.planar_cloud(20000, (4, 4, 2), seed=3, stream=1, sigma=0.002, inlier_fraction=1.0)
    centroid = S.mean(axis=0)
    axis = np.array([0.3, -0.5, 0.8])
    M = se3_exp(np.concatenate([np.deg2rad(1.0) * axis / np.linalg.norm(axis), [0.03, -0.02, 0.04]]), centroid)
    return P, transform_np(np.linalg.inv(M), S), M, centroid


def motion_errors(T, M, centroid):
    """(rotation error in degrees, centroid error) of the estimate T of the motion M."""
    E = np.asarray(T) @ np.linalg.inv(M)
    ang = np.degrees(np.arccos(np.clip((np.trace(E[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))
    return float(ang), float(np.linalg.norm(E[:3, :3] @ centroid + E[:3, 3] - centroid))


def assert_recovers_motion(a: Alignment, M, centroid, n):
    rot0, cen0 = motion_errors(np.eye(4), M, centroid)
    rot1, cen1 = motion_errors(a.transform, M, centroid)
    print(f"rotation error {rot0:.4f} -> {rot1:.5f} deg, centroid error {cen0:.4f} -> {cen1:.6f}, "
          f"{a.iterations} iterations, n_used {a.n_used}, costs {a.costs[0]:.4g} -> {a.costs[-1]:.4g}")
    assert a.converged and a.reason == "converged" and a.iterations <= 12
    assert a.costs[-1] < a.costs[0] and len(a.costs) == a.iterations
    assert rot1 * 50 <= rot0 and cen1 * 50 <= cen0
    assert a.n_used >= 0.95 * n


def test_align_recovers_a_known_motion():
    P, scan, M, centroid = known_motion_scene()
    assert abs(motion_errors(np.eye(4), M, centroid)[0] - 1.0) < 1e-9
    g = _plug_grid({0: P})
    a = g.align(scan, max_distance=0.2)
    assert_recovers_motion(a, M, centroid, len(scan))
    assert np.array_equal(a.transform[3], [0, 0, 0, 1])
    assert np.allclose(a.transform[:3, :3] @ a.transform[:3, :3].T, np.eye(3), rtol=0, atol=1e-12)
    # one iteration is one step: the loop stops where it is told to
    one = g.align(scan, max_distance=0.2, max_iterations=1)
    assert not one.converged and one.reason == "max_iterations" and one.iterations == 1 and len(one.costs) == 1


# ---- declarations and exports ----------------------------------------------------------------------------------------
def test_entries_declared_and_in_signature_table():
    from octreelib_amd import _native as nat

    text = open(os.path.join(ROOT, "include", "octreelib_hip.h")).read()
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    p, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    for name, decl in ENTRIES.items():
        assert decl + ";" in header, f"{name} is not declared as `{decl}`"
        res, args = nat.SIGNATURES[name]
        assert res is C.c_int and args == [p, p, i64, p, p, i32, f64, f64, f64, p, p, p, p, p]
    assert "#define OCTL_ABI_VERSION 1" in re.sub(r"\s+", " ", text)
    if os.path.exists(nat.lib_path()):
        lib = nat.load()
        for name in ENTRIES:
            assert getattr(lib, name).argtypes == nat.SIGNATURES[name][1]
        assert lib.octl_abi_version() == 1


def test_exported_from_the_package():
    import octreelib_amd
    from octreelib_amd.octree import Octree
    from octreelib_amd.octree_manager import OctreeManager

    for name in ("RegistrationSystem", "Alignment", "registration_system_np", "align_np", "se3_exp", "transform_np"):
        assert name in octreelib_amd.__all__ and hasattr(octreelib_amd, name)
    for cls in (Grid, OctreeManager, Octree):
        assert callable(getattr(cls, "registration_system")) and callable(getattr(cls, "align"))
    # se3_exp: a rotation about the origin it is given, and the identity at zero
    c = np.array([5.0e5, 4.0e6, 100.0])
    E = se3_exp([0.0, 0.0, np.pi / 2, 1.0, 2.0, 3.0], c)
    assert np.allclose(E @ np.append(c, 1.0), np.append(c + [1.0, 2.0, 3.0], 1.0), rtol=0, atol=1e-9)
    assert np.allclose(E[:3, :3] @ [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], rtol=0, atol=1e-15)
    assert np.array_equal(se3_exp(np.zeros(6), c), np.eye(4))
