"""
Neighbourhood statistics and point normals (no reference counterpart): what the surface looks like round a point - the
count, mean and covariance of the stored points within a radius, and the covariance's eigen-decomposition, whose
smallest eigenvalue's vector is the point's normal and whose surface_variation is its curvature.  What PCL's
NormalEstimation and Open3D's estimate_normals give, normal-space sampling, edge / planar feature selection and GICP
start from - without the walls of the subdivision that quantise leaf_planes.

  neighbourhood_statistics(map, points, radius)   one LeafStatistics row per query point;
  point_statistics(map, radius)                   the self-query: one row per alive stored point, with its (pose, index);
  orient_towards(normals, points, viewpoint)      flip normals to face the sensor.

They are module-level functions over a Grid, an OctreeManager or an Octree - on the device-resident map one kernel each
(octl_forest_neighbourhood_stats, octl_forest_point_stats: csrc/moments.hip, csrc/radius_moments.h), on
the caller's own plug types the host definitions below through query.HostMap.
"""

from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from octreelib_amd.leaf_stats import LeafStatistics, leaf_statistics_np
from octreelib_amd.query import _as_queries, check_radius_args

__all__ = ["PointStatistics", "neighbourhood_statistics_np", "point_statistics_np", "orient_towards",
           "neighbourhood_statistics", "point_statistics"]


@dataclass
class PointStatistics(LeafStatistics):
    """LeafStatistics of the neighbourhoods of n stored points; row i describes the point `index[i]` of pose
    `pose[i]`, rows ascending in (insertion order of the pose, index): the total order of Neighbours."""

    pose: np.ndarray = None    # (n,) int32 pose number
    index: np.ndarray = None   # (n,) int32 row of the point in that pose's cloud as inserted (Neighbours.index)


def _neighbour_lists(points, clouds, radius, what, chunk=256):
    r, _, _ = check_radius_args(radius, what=what)
    q = _as_queries(points)
    parts = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for _, c in clouds]
    P = np.concatenate(parts) if parts else np.empty((0, 3))
    out = [P[:0]] * len(q)
    if len(q) == 0 or len(P) == 0:
        return q, out
    r2 = np.float64(r) * np.float64(r)
    ok = np.all(np.isfinite(q), axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, len(q), chunk):
            qa = q[a: a + chunk]
            dx = qa[:, None, 0] - P[None, :, 0]
            dy = qa[:, None, 1] - P[None, :, 1]
            dz = qa[:, None, 2] - P[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            hit = (d2 <= r2) & ok[a: a + chunk, None]
            for i in np.nonzero(hit.any(axis=1))[0]:
                out[a + i] = P[hit[i]]
    return q, out


def neighbourhood_statistics_np(points, clouds, radius, *, dtype=np.float64, eigen: bool = True, chunk: int = 256,
                                what="neighbourhood_statistics") -> LeafStatistics:
    """Count, mean and population covariance (np.cov(..., bias=True)) of the stored points within `radius` of every
    query point, and the covariance's eigen-decomposition: the definition of neighbourhood_statistics.  clouds:
    [(pose number, (m, 3) points)] of the counted poses, as radius_count_np takes them.  The neighbours of q are
    selected by radius_count_np's own arithmetic in float64 - dx = q_x - p_x, d2 = (dx dx + dy dy) + dz dz with
    separate products and sums, p counts iff d2 <= radius * radius, inclusive - so count equals radius_count_np
    exactly, whatever `dtype`.  The moments are taken in two passes (mean, then the centred second moments) in `dtype`
    - np.longdouble for a reference of higher precision - and returned in it; eigenvalues (ascending) and eigenvectors
    (columns) are np.linalg.eigh's in float64 under the library's sign rule (orient_eigenvectors), None with
    eigen=False.  A query with a coordinate that is not finite, and one without a neighbour, has count 0 and NaN in
    every other field."""
    q, lists = _neighbour_lists(points, clouds, radius, what, chunk)
    st = leaf_statistics_np(lists, dtype=dtype, eigen=False)
    none = st.count == 0
    st.mean[none] = np.nan
    st.covariance[none] = np.nan
    if eigen:
        w = np.full((len(q), 3), np.nan)
        v = np.full((len(q), 3, 3), np.nan)
        some = np.nonzero(~none)[0]
        if len(some):
            full = leaf_statistics_np([lists[i] for i in some], dtype=dtype, eigen=True)
            w[some], v[some] = full.eigenvalues, full.eigenvectors
        st.eigenvalues, st.eigenvectors = w, v
    return st


def _tested_clouds(clouds, tested, what):
    """[(pose number, points)] of the judged poses: those of `clouds` that are tested, in their order, then the pairs."""
    names = [int(p) for p, _ in clouds]
    if tested is None:
        return [(p, c) for p, c in clouds]
    chosen, extra = set(), []
    for t in tested:
        if isinstance(t, (int, np.integer)):
            if int(t) not in names:
                raise ValueError(f"{what}: tested pose {t!r} is not among the counted clouds and brings no points")
            chosen.add(int(t))
        else:
            p, pts = t
            if int(p) in names:
                raise ValueError(f"{what}: tested pose {p!r} is among the counted clouds: name it by its number")
            extra.append((int(p), pts))
    return [(p, c) for p, c in clouds if int(p) in chosen] + extra


def point_statistics_np(clouds, tested, radius, *, dtype=np.float64, eigen: bool = True) -> PointStatistics:
    """The self-query, the definition of point_statistics: for every point x of a tested pose the row
    neighbourhood_statistics_np([x], clouds, radius) - the stored points of the COUNTED clouds within `radius` of x,
    x itself among them when its pose is counted (d2 = 0; PCL's convention, the opposite of sparse_keep_np's
    exclusion).  clouds and tested have the meaning they have in sparse_keep_np: tested names poses among `clouds`
    (None: all of them) and brings, for a tested pose that is not counted, a (pose number, points) pair.  Rows: the
    tested poses of `clouds` in their order, then the pairs in the order given; index = the row in the cloud."""
    check_radius_args(radius, what="point_statistics")
    judged = _tested_clouds(clouds, tested, "point_statistics")
    parts = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for _, c in judged]
    X = np.concatenate(parts) if parts else np.empty((0, 3))
    st = neighbourhood_statistics_np(X, clouds, radius, dtype=dtype, eigen=eigen, what="point_statistics")
    pose = np.repeat(np.asarray([p for p, _ in judged], dtype=np.int32), [len(c) for c in parts])
    index = (np.concatenate([np.arange(len(c), dtype=np.int32) for c in parts]) if parts
             else np.empty(0, dtype=np.int32))
    return PointStatistics(st.count, st.mean, st.covariance, st.eigenvalues, st.eigenvectors, pose.astype(np.int32),
                           index)


def orient_towards(normals, points, viewpoint) -> np.ndarray:
    """The normals (n, 3) of the points (n, 3), each flipped to face `viewpoint` ((3,), or (n, 3): one per point):
    normal . (viewpoint - point) >= 0 afterwards.  A new array."""
    n = np.array(normals, dtype=np.float64).reshape(-1, 3)
    away = np.einsum("ij,ij->i", n, np.asarray(viewpoint, dtype=np.float64) - np.asarray(points, dtype=np.float64)) < 0
    n[away] = -n[away]
    return n


def neighbourhood_statistics(map, points, radius, *, pose_numbers: Optional[List[int]] = None,
                             eigen: bool = True) -> LeafStatistics:
    """What the surface looks like round every query point: a LeafStatistics whose row i describes the stored points
    of the given poses (None: all) within `radius` of query i - count, mean, population covariance and, with eigen,
    eigenvalues (ascending) and eigenvectors under the sign rule of leaf_statistics; .normal is the point's normal (up
    to sign: orient_towards), .surface_variation its curvature.  map: a Grid, an OctreeManager or an Octree.  The
    neighbours are exactly the points radius_count counts: count[i] == radius_count(points, radius,
    pose_numbers=...)[i], distance2 <= radius^2 inclusive; what a mask, a filter, carve, remove_sparse, thin or
    remove_poses took out never counts.  A query that is not finite, and one without a neighbour, has count 0 and NaN
    in every other field; a single neighbour has covariance 0.  points: any (n, 3) array-like, or a DeviceCloud of
    float64 points, read where it lies.  One kernel once the block index of the selection exists
    (neighbourhood_statistics_np is the definition).  With n neighbours within R = max |p - q|_inf of the query the mean
    is within 2 g R + 2^-53 |mean| and every covariance entry within 4 g R^2 of the exact value, g = (n + 16) 2^-53:
    the magnitude of the coordinates does not enter.  The same map and the same query bits give the same row bits - from
    a host array, a DeviceCloud, any batch, or as a stored point of point_statistics with the same selection; two maps
    with the same points but another subdivision visit the neighbours in another order and may differ within the
    bound.  ValueError for a radius that is not finite and positive or, on a Grid, above twice the voxel edge (one cube
    has no cap on the radius), for a float32 DeviceCloud and for an Octree with pose_numbers; RuntimeError after
    map_leaf_points moved rows outside their leaves; KeyError for an unknown pose; TypeError for another kind of map."""
    from octreelib_amd._map_ops import _resolve

    forest, host, sel, _ = _resolve(map, pose_numbers, "neighbourhood_statistics")
    if host is not None:
        return host.neighbourhood_statistics(points, radius, pose_numbers=sel, eigen=eigen)
    return forest.neighbourhood_stats(points, radius, sel, eigen)


def point_statistics(map, radius, *, pose_numbers: Optional[List[int]] = None, among: Optional[List[int]] = None,
                     eigen: bool = True) -> PointStatistics:
    """Normals, curvature and covariances of the map's own points: a PointStatistics with one row per alive stored
    point of the given poses (None: all) describing the stored points of the poses of `among` (None: all) within
    `radius` of it - pose_numbers=[newest] describes a new scan against the whole map.  map: a Grid, an OctreeManager
    or an Octree.  The point itself is among its neighbours when its pose is counted - PCL's convention, and the
    opposite of remove_sparse, which never counts a point for itself - so such a row has count >= 1; a tested pose
    that is not counted is described by the counted ones only.  pose[i], index[i] name the point of row i (index: its
    row in the cloud as inserted, Neighbours.index); rows ascend in (insertion order of the pose, index).  What a mask,
    a filter, carve, remove_sparse, thin or remove_poses took out has no row and is not counted; points that a pending
    RANSAC mask is about to drop still have rows and still count, as in remove_sparse - apply_mask first avoids it.
    The map is not changed and no cached table is dropped.  One kernel once the block index of `among` exists
    (point_statistics_np is the definition); a row is, bit for bit, the row neighbourhood_statistics gives for the
    stored point under pose_numbers=among, and is bounded as that one is.  ValueError for a radius that
    neighbourhood_statistics refuses and for an Octree with pose_numbers or among; RuntimeError after map_leaf_points
    moved rows outside their leaves; KeyError for an unknown pose; TypeError for another kind of map."""
    from octreelib_amd._map_ops import MapOperations, _resolve

    forest, host, sel, names = _resolve(map, pose_numbers, "point_statistics")
    asel = None
    if isinstance(map, MapOperations):
        asel = map._query_slots(among)
    elif among is not None:
        raise ValueError("point_statistics: an Octree holds a single pose and takes no among")
    if host is not None:
        return host.point_statistics(radius, pose_numbers=sel, among=asel, eigen=eigen)
    return forest.point_stats(radius, sel, asel, eigen, names)
