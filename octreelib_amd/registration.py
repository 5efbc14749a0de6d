"""
Scan-to-map registration against the pooled leaf planes: the point-to-plane normal equations of a scan under a rigid
transform (registration_system), and the Gauss-Newton loop over them (align).  Further down the same against the
nearest stored points - classic ICP where the map has no planes to offer (point_registration_system, align_points:
point_registration_system_np is their definition), and the two combined: the correspondence of the nearest stored
point, the residual against the plane of that point's leaf (nearest_plane_registration_system, align_nearest_planes
in octreelib_amd/matching.py: nearest_plane_registration_system_np is their definition).

The device reduces a scan to the 6x6 system - 28 sums and two counts (octl_forest_registration_system, csrc/
register.hip); the solve, the pose update and the loop are NumPy on the host (one download of 240 bytes per iteration).
registration_system_np is the same on the host: the specification, the higher-precision reference of the tests, and
what the classes built on the caller's own plug types run through query.HostMap.

Per query q, with the transform T = (R, t) and an origin c:
  p_i  = ((R_i0 q_x + R_i1 q_y) + R_i2 q_z) + t_i        every product and sum rounded to f64 (transform_np)
  node = locate(p); row, r = point_to_plane(p)            the existing queries, same gates
  used = row >= 0 and r finite and (max_distance is None or |r| <= max_distance)
  d = p - c,  J = [d x n, n]                              dr/dxi under p <- Rot(w)(p - c) + c + v, xi = (w, v)
  w = 1, or with Huber: 1 if |r| <= delta else delta / |r|
  H = sum w J J^T,  g = sum w J r,  cost = sum rho(r)     rho = r^2 / 2, or delta (|r| - delta / 2) beyond delta
over the used points only (they are selected, not weighted by zero: a NaN query never reaches a sum).
"""

from dataclasses import dataclass, field
from typing import Callable, List, Optional

import numpy as np

from octreelib_amd.query import LeafPlanes, Neighbours, _as_queries, check_nearest_args, nearest_np, point_to_plane_np

__all__ = ["RegistrationSystem", "Alignment", "as_transform", "transform_np", "transform_rows_np",
           "as_transform_rows", "default_origin", "se3_exp",
           "system_from_sums", "registration_system_np", "point_registration_system_np",
           "nearest_plane_registration_system_np", "align_np"]

_TRIU = np.triu_indices(6)


@dataclass
class RegistrationSystem:
    """The normal equations of one transform.  node / row / residual / planes: the per-point answers (those of
    point_to_plane for the transformed scan) when they were asked for, None otherwise.  neighbours: the per-point
    answers of a point-to-point system (those of nearest with k = 1 for the transformed scan), likewise."""

    H: np.ndarray            # (6, 6) symmetric
    g: np.ndarray            # (6,)
    cost: float
    n_used: int
    n_located: int
    origin: np.ndarray       # (3,)
    node: Optional[np.ndarray] = None
    row: Optional[np.ndarray] = None
    residual: Optional[np.ndarray] = None
    planes: Optional[LeafPlanes] = None
    neighbours: Optional[Neighbours] = None

    def solve(self, damping: float = 0.0) -> np.ndarray:
        """xi = -(H + damping diag(H))^-1 g; ValueError when fewer than six points were used."""
        if self.n_used < 6:
            raise ValueError(f"registration system of {self.n_used} points: at least 6 are needed")
        H = np.asarray(self.H, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):     # (sums that overflowed give a non-finite step)
            A = H + float(damping) * np.diag(np.diag(H))
            return -np.linalg.solve(A, np.asarray(self.g, dtype=np.float64))


@dataclass
class Alignment:
    transform: np.ndarray    # (4, 4)
    iterations: int
    converged: bool
    costs: List[float] = field(default_factory=list)   # cost of every system that was solved
    n_used: int = 0          # points used by the last system
    reason: str = ""


def as_transform(transform):
    """(R (3, 3), t (3,)) f64 of a 4x4 or 3x4 rigid transform (None: the identity); ValueError otherwise."""
    if transform is None:
        return np.eye(3), np.zeros(3)
    a = np.asarray(transform, dtype=np.float64)
    if a.shape == (4, 4):
        if not np.array_equal(a[3], [0.0, 0.0, 0.0, 1.0]):
            raise ValueError("the last row of a 4x4 transform must be (0, 0, 0, 1)")
        a = a[:3]
    if a.shape != (3, 4):
        raise ValueError(f"expected a 4x4 or 3x4 transform, got shape {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError("the transform is not finite")
    return np.ascontiguousarray(a[:, :3]), np.ascontiguousarray(a[:, 3])


def _as_origin(origin) -> np.ndarray:
    c = np.asarray(origin, dtype=np.float64).reshape(-1)
    if c.shape != (3,) or not np.all(np.isfinite(c)):
        raise ValueError("the origin must be three finite numbers")
    return c


def _matrix(R, t) -> np.ndarray:
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def transform_np(transform, points) -> np.ndarray:
    """p_i = ((R_i0 q_x + R_i1 q_y) + R_i2 q_z) + t_i in f64, one rounding per product and per sum, in this order:
    the bits the device forms (no fused multiply-add on either side)."""
    R, t = as_transform(transform)
    q = _as_queries(points)
    with np.errstate(invalid="ignore", over="ignore"):
        cols = [((R[i, 0] * q[:, 0] + R[i, 1] * q[:, 1]) + R[i, 2] * q[:, 2]) + t[i] for i in range(3)]
    return np.ascontiguousarray(np.stack(cols, axis=1)) if len(q) else np.empty((0, 3))


XF_MAX_SEGMENTS = 1024   # OCTL_XF_MAX_SEGMENTS (include/octreelib_hip.h)


def as_transform_rows(transforms, segment, n: int):
    """(table (M, 12) f64 - the rows (R_i0 R_i1 R_i2 t_i) of every 3x4 -, segment uint16 (n,) or None) of the
    arguments of transform_rows_np, validated; ValueError otherwise."""
    a = np.asarray(transforms, dtype=np.float64)
    if a.ndim == 2:
        if segment is not None:
            raise ValueError("segment is given with a single transform: pass transforms of shape (M, 3, 4) or "
                             "(M, 4, 4)")
        R, t = as_transform(a)
        return np.ascontiguousarray(np.concatenate([R, t[:, None]], axis=1).reshape(1, 12)), None
    if a.ndim != 3:
        raise ValueError(f"expected a 4x4 or 3x4 transform or a stack of them, got shape {a.shape}")
    if segment is None:
        raise ValueError("a stack of transforms needs segment, the index of every row's transform")
    M = a.shape[0]
    if not 1 <= M <= XF_MAX_SEGMENTS:
        raise ValueError(f"{M} transforms: between 1 and {XF_MAX_SEGMENTS} are supported")
    table = np.empty((M, 12))
    for k in range(M):
        R, t = as_transform(a[k])
        table[k] = np.concatenate([R, t[:, None]], axis=1).reshape(12)
    s = np.asarray(segment)
    if not np.issubdtype(s.dtype, np.integer):
        raise ValueError(f"segment must have an integer dtype, got {s.dtype}")
    if s.shape != (n,):
        raise ValueError(f"segment must have shape ({n},), one index per point, got {s.shape}")
    if n and (int(s.min()) < 0 or int(s.max()) >= M):
        raise ValueError(f"segment entries must lie in [0, {M})")
    return table, np.ascontiguousarray(s, dtype=np.uint16)


def transform_rows_np(transforms, points, segment=None) -> np.ndarray:
    """transform_np with a transform per row ("piecewise rigid": the firing columns of a sweep, each with its pose).
    transforms (3, 4) or (4, 4) and segment None: transform_np(transforms, points).  transforms (M, 3, 4) or (M, 4, 4),
    1 <= M <= 1024, and segment (n,) of an integer dtype with entries in [0, M): row i is
    transform_np(transforms[segment[i]], points[i:i+1]) - the same formula, every product and sum rounded.  f32 points
    are widened first.  What insert_points(points, transform=transforms, segment=segment) stores."""
    q = points.astype(np.float64) if isinstance(points, np.ndarray) and points.dtype == np.float32 else points
    q = _as_queries(q)
    table, seg = as_transform_rows(transforms, segment, len(q))
    if seg is None:
        return transform_np(table.reshape(3, 4), q)
    m = table[seg]           # (n, 12)
    with np.errstate(invalid="ignore", over="ignore"):
        cols = [((m[:, 4 * i] * q[:, 0] + m[:, 4 * i + 1] * q[:, 1]) + m[:, 4 * i + 2] * q[:, 2]) + m[:, 4 * i + 3]
                for i in range(3)]
    return np.ascontiguousarray(np.stack(cols, axis=1)) if len(q) else np.empty((0, 3))


def host_transformed(points, transform, segment):
    """The cloud the caller's own plug types are fed for insert_points(points, transform=..., segment=...): moved on the
    host (transform_rows_np) before the plug sees it."""
    if transform is None:
        raise ValueError("segment is given without transforms")
    return transform_rows_np(transform, points, segment)


def default_origin(transform, points) -> np.ndarray:
    """Centroid of the transformed scan over its finite points (zeros when there is none): what align fixes as the
    origin at its first iteration.  At UTM magnitudes d = p would let the rotational block of H swamp the rest.  A
    finite but absurd coordinate (1e300) moves the centroid with it: such a scan wants cleaning, or an origin."""
    p = transform_np(transform, points)
    ok = np.all(np.isfinite(p), axis=1)
    return p[ok].mean(axis=0) if ok.any() else np.zeros(3)


def se3_exp(xi, origin=None) -> np.ndarray:
    """4x4 of the update p <- Rot(w)(p - c) + c + v for xi = (w, v): Rodrigues' formula about the origin c."""
    xi = np.asarray(xi, dtype=np.float64).reshape(6)
    c = np.zeros(3) if origin is None else _as_origin(origin)
    w, v = xi[:3], xi[3:]
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:     # (sin th / th and (1 - cos th) / th^2 by their series: exact to f64 below this angle)
        a, b = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th)
    R = np.eye(3) + a * K + b * (K @ K)
    return _matrix(R, c - R @ c + v)


def system_from_sums(sums, counts, origin) -> RegistrationSystem:
    """RegistrationSystem of the 28 sums (21 of H's upper triangle row-major, 6 of g, the cost) and the two counts."""
    s = np.asarray(sums).reshape(28)
    H = np.zeros((6, 6), dtype=s.dtype)
    H[_TRIU] = s[:21]
    H = H + np.triu(H, 1).T
    return RegistrationSystem(H, s[21:27].copy(), s[27], int(counts[0]), int(counts[1]),
                              np.array(origin, dtype=np.float64))


def registration_system_np(locate: Callable, planes: LeafPlanes, points, transform=None, origin=None,
                           min_points: int = 8, max_variance: Optional[float] = None,
                           max_distance: Optional[float] = None, huber_delta: Optional[float] = None,
                           dtype=np.float64, answers=None, per_point: bool = False) -> RegistrationSystem:
    """The definition (module docstring), on the host.  locate: points (n, 3) -> node ids (HostMap.locate, or
    locate_np over downloaded tables); planes: the pooled table.  origin None: default_origin.  The sums are formed in
    `dtype` (np.longdouble for a reference of higher precision) from p, r and the table's own bits.  answers = (node,
    row, residual): take these per-point answers as given instead of forming them here - the reference of a sum over
    exactly the terms another implementation selected."""
    R, t = as_transform(transform)
    T = _matrix(R, t)
    q = _as_queries(points)
    p = transform_np(T, q)
    c = default_origin(T, q) if origin is None else _as_origin(origin)
    if answers is None:
        node = np.asarray(locate(p), dtype=np.int32) if len(p) else np.empty(0, dtype=np.int32)
        row, r = point_to_plane_np(node, planes, p, min_points, max_variance)
    else:
        node, row, r = (np.asarray(a) for a in answers)
    with np.errstate(invalid="ignore"):
        used = (row >= 0) & np.isfinite(r)
        if max_distance is not None and max_distance >= 0:
            used &= ~(np.abs(r) > max_distance)
    with np.errstate(invalid="ignore", over="ignore"):      # (a wild origin overflows; the sums say so)
        rr = np.asarray(r, dtype=np.float64)[used].astype(dtype)
        nrm = (np.asarray(planes.normal, dtype=np.float64)[row[used]].astype(dtype) if used.any()
               else np.zeros((0, 3), dtype))
        d = p[used].astype(dtype) - c.astype(dtype)
        J = np.concatenate([np.cross(d, nrm).reshape(-1, 3), nrm], axis=1)
        ar = np.abs(rr)
        w = np.ones(len(rr), dtype=dtype)
        rho = rr * rr / 2
        if huber_delta is not None and huber_delta > 0:
            dl = dtype(huber_delta)
            tail = ar > dl
            w[tail] = dl / ar[tail]
            rho[tail] = dl * (ar[tail] - dl / 2)
        wJ = J * w[:, None]
        H = wJ.T @ J
        g = (wJ * rr[:, None]).sum(axis=0)
    out = RegistrationSystem(np.asarray(H, dtype=dtype).reshape(6, 6), g, rho.sum(dtype=dtype), int(used.sum()),
                             int((node >= 0).sum()), c)
    if per_point:
        out.node, out.row, out.residual, out.planes = node, row, r, planes
    return out


def point_registration_system_np(clouds, points, transform=None, origin=None, *, max_distance: float,
                                 huber_delta: Optional[float] = None, dtype=np.float64, answers=None,
                                 per_point: bool = False) -> RegistrationSystem:
    """The point-to-point normal equations of a scan against the nearest stored point of every transformed query, on
    the host: the definition of point_registration_system (octl_forest_point_registration_system, csrc/
    register_points.hip).  clouds: [(pose number, (m, 3) points)] of the selected poses in ascending slot order, as
    nearest_np takes them.  Per query q, with T = (R, t), the origin c, r = max_distance and delta = huber_delta:

      p = transform_np(T, q)                                   the bits of registration_system
      (pose, index, d2, count) = nearest_np(p, clouds, k=1, max_distance=r)
                                                               the total order (d2, slot, index), d2 <= fl(r r) inclusive
      used = count == 1; m = the stored point, bit for bit; e = p - m, one rounding per component (nearest's own dx,
      dy, dz; d2 is its d2); n_located = the queries whose p is finite (a query that is not is skipped by a branch)
      d = p - c; the residual under p <- Rot(w)(p - c) + c + v is e + w x d + v, so J = [-[d]x, I3]
      Huber, decided on d2: inlier iff d2 <= fl(delta delta): w = 1, rho = d2 / 2; otherwise s = sqrt(d2), w = delta / s,
      rho = delta (s - delta / 2)
      H = sum w J^T J, g = sum w J^T e, cost = sum rho:  H_ww = sum w (|d|^2 I - d d^T), H_wv = [sum w d]x,
      H_vv = (sum w) I, g_w = sum w d x e, g_v = sum w e - 17 distinct sums; the rest of system_from_sums' 28 numbers
      are copies, sign changes and structural zeros (+0.0).

    origin None: default_origin.  The sums are formed in `dtype` (np.longdouble for a reference of higher precision)
    from the f64 bits of p, e and d2.  answers = a Neighbours (k = 1) for the transformed scan: take these per-point
    answers as given instead of searching here - the reference of a sum over exactly the terms another
    implementation selected.  per_point: the Neighbours come back in .neighbours."""
    _, r = check_nearest_args(1, max_distance)
    R, t = as_transform(transform)
    T = _matrix(R, t)
    q = _as_queries(points)
    p = transform_np(T, q)
    c = default_origin(T, q) if origin is None else _as_origin(origin)
    clouds = [(int(k), np.asarray(a, dtype=np.float64).reshape(-1, 3)) for k, a in clouds]
    nb = nearest_np(p, clouds, 1, max_distance=r) if answers is None else answers
    used = np.asarray(nb.count).reshape(-1) > 0
    pose, index = np.asarray(nb.pose).reshape(-1)[used], np.asarray(nb.index).reshape(-1)[used]
    m = np.empty((int(used.sum()), 3))
    for k, a in clouds:
        of = pose == k
        m[of] = a[index[of]]
    with np.errstate(invalid="ignore", over="ignore"):      # (a wild origin overflows; the sums say so)
        n_located = int(np.all(np.isfinite(p), axis=1).sum())
        e = (p[used] - m).astype(dtype)
        d2_64 = np.asarray(nb.distance2, dtype=np.float64).reshape(-1)[used]
        d2 = d2_64.astype(dtype)
        d = p[used].astype(dtype) - c.astype(dtype)
        w = np.ones(len(d2), dtype=dtype)
        rho = d2 / 2
        if huber_delta is not None and huber_delta > 0:
            tail = d2_64 > np.float64(huber_delta) * np.float64(huber_delta)
            dl = dtype(huber_delta)
            s = np.sqrt(d2[tail])
            w[tail] = dl / s
            rho[tail] = dl * (s - dl / 2)
        wd, we = d * w[:, None], e * w[:, None]
        x, y, z = d[:, 0], d[:, 1], d[:, 2]
        sm = lambda a: a.sum(dtype=dtype) if len(a) else dtype(0)
        X, Y, Z, W = sm(wd[:, 0]), sm(wd[:, 1]), sm(wd[:, 2]), sm(w)
        gw = np.cross(wd, e).reshape(-1, 3)
        zero = dtype(0)
        sums = np.array([
            sm(wd[:, 1] * y + wd[:, 2] * z), sm(-wd[:, 0] * y), sm(-wd[:, 0] * z), zero, zero - Z, Y,
            sm(wd[:, 0] * x + wd[:, 2] * z), sm(-wd[:, 1] * z), Z, zero, zero - X,
            sm(wd[:, 0] * x + wd[:, 1] * y), zero - Y, X, zero,
            W, zero, zero,
            W, zero,
            W,
            sm(gw[:, 0]), sm(gw[:, 1]), sm(gw[:, 2]), sm(we[:, 0]), sm(we[:, 1]), sm(we[:, 2]),
            sm(rho)], dtype=dtype)
    out = system_from_sums(sums, (int(used.sum()), n_located), c)
    if per_point:
        out.neighbours = nb
    return out


def nearest_plane_registration_system_np(locate: Callable, planes: LeafPlanes, clouds, points, transform=None,
                                         origin=None, *, max_distance: float, min_points: int = 8,
                                         max_variance: Optional[float] = None, huber_delta: Optional[float] = None,
                                         dtype=np.float64, answers=None,
                                         per_point: bool = False) -> RegistrationSystem:
    """The nearest-point-to-plane normal equations of a scan, on the host: the definition of
    nearest_plane_registration_system (octl_forest_nearest_plane_registration_system, csrc/
    register_nearest_plane.hip).  The correspondence of point_registration_system_np, the residual of
    registration_system_np - a composition of the definitions above, with no arithmetic of its own.  locate: points
    (n, 3) -> node ids; planes: the pooled table; clouds: [(pose number, (m, 3) points)] in ascending slot order -
    planes and clouds over the SAME pose selection.  Per query q, with T = (R, t) and r = max_distance:

      p = transform_np(T, q)
      nb = nearest_np(p, clouds, 1, max_distance=r)            the correspondence of nearest(..., k=1): the same d2
                                                               bits, the same total order (d2, slot, index)
      m = the matched stored point, bit for bit; node = locate(m), the scheme leaf the MATCHED POINT lies in, -1
      where there is no match - not locate(p)
      row, residual = point_to_plane_np(node, planes, p, min_points, max_variance)
                                                               the signed distance of the QUERY p to the pooled plane
                                                               of the matched point's leaf; -1 and NaN where that
                                                               leaf has no accepted plane
      the system = registration_system_np(..., answers=(node, row, residual), max_distance=None,
      huber_delta=huber_delta): J, the Huber rule on |residual|, the 28 sums and n_used unchanged; n_located = the
      queries that found a correspondence (node >= 0).

    max_distance is the search radius only: there is no gate on |residual|.  answers = (Neighbours, node, row,
    residual): take these per-point answers as given - the reference of a sum over exactly the terms another
    implementation selected.  per_point: .neighbours, .node, .row, .residual and .planes come back."""
    _, r = check_nearest_args(1, max_distance)
    R, t = as_transform(transform)
    T = _matrix(R, t)
    q = _as_queries(points)
    if answers is None:
        p = transform_np(T, q)
        clouds = [(int(k), np.asarray(a, dtype=np.float64).reshape(-1, 3)) for k, a in clouds]
        nb = nearest_np(p, clouds, 1, max_distance=r)
        used = np.asarray(nb.count).reshape(-1) > 0
        pose, index = np.asarray(nb.pose).reshape(-1)[used], np.asarray(nb.index).reshape(-1)[used]
        m = np.empty((int(used.sum()), 3))
        for k, a in clouds:
            of = pose == k
            m[of] = a[index[of]]
        node = np.full(len(p), -1, dtype=np.int32)
        if len(m):
            node[used] = np.asarray(locate(m), dtype=np.int32)
        row, res = point_to_plane_np(node, planes, p, min_points, max_variance)
    else:
        nb, node, row, res = answers
    out = registration_system_np(None, planes, q, T, origin, min_points, max_variance, None, huber_delta, dtype,
                                 answers=(node, row, res), per_point=per_point)
    if per_point:
        out.neighbours = nb
    return out


def align_np(system: Callable, initial=None, max_iterations: int = 20, tolerance: float = 1e-9,
             damping: float = 0.0) -> Alignment:
    """Gauss-Newton over system(T (4, 4), origin or None) -> RegistrationSystem.  The first call passes origin None
    and the origin that system chose (RegistrationSystem.origin) is kept for the rest of the run.  Per iteration:
    xi = system.solve(damping), T <- se3_exp(xi, origin) T.  Ends converged when |xi| < tolerance; otherwise at
    max_iterations, or - with the last good transform - when fewer than six points are used ("no correspondences")
    or the system cannot be solved ("singular system")."""
    R, t = as_transform(initial)
    T = _matrix(R, t)
    costs, origin, n_used = [], None, 0
    for it in range(int(max_iterations)):
        s = system(T, origin)
        origin, n_used = s.origin, s.n_used
        if s.n_used < 6:
            return Alignment(T, it, False, costs, n_used, "no correspondences")
        try:
            xi = s.solve(damping)
        except np.linalg.LinAlgError:
            xi = None
        if xi is None or not np.all(np.isfinite(xi)):   # (also sums that overflowed: an origin at 1e300, say)
            return Alignment(T, it, False, costs, n_used, "singular system")
        costs.append(float(s.cost))
        T = se3_exp(xi, origin) @ T
        T[3] = [0.0, 0.0, 0.0, 1.0]
        if float(np.linalg.norm(xi)) < tolerance:
            return Alignment(T, it + 1, True, costs, n_used, "converged")
    return Alignment(T, int(max_iterations), False, costs, n_used, "max_iterations")
