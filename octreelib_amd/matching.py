"""
Nearest-point-to-plane scan-to-map registration (no reference counterpart): the correspondence from the nearest
stored point, the residual against the pooled plane of the leaf THAT point lies in - what LiDAR odometry uses.

  align / registration_system            score a point against the plane of the leaf the point itself falls into: the
                                         basin of convergence is a fraction of a leaf;
  align_points / point_registration_system  find the nearest stored point across leaf and voxel walls (the basin is
                                         max_distance), but the residual is point-to-point: on planes the fixed point
                                         is biased by the sampling;
  the two functions below                the basin of the second with the residual of the first.

They are module-level functions over a Grid, an OctreeManager or an Octree - on the device-resident map three
kernels and a 240-byte download per system (octl_forest_nearest_plane_registration_system, csrc/
register_nearest_plane.hip), on the caller's own plug types the host definition through
query.HostMap (octreelib_amd/registration.py: nearest_plane_registration_system_np).
"""

from typing import List, Optional

from octreelib_amd._map_ops import _resolve
from octreelib_amd.registration import Alignment, RegistrationSystem

__all__ = ["nearest_plane_registration_system", "align_nearest_planes"]


def nearest_plane_registration_system(map, points, transform=None, *, max_distance: float,
                                      pose_numbers: Optional[List[int]] = None, min_points: int = 8,
                                      max_variance: Optional[float] = None, huber_delta: Optional[float] = None,
                                      origin=None, per_point: bool = False) -> RegistrationSystem:
    """The point-to-plane normal equations of a scan under `transform` (4x4 or 3x4, None: identity), every point
    scored against the pooled plane of the leaf its NEAREST STORED POINT lies in: a RegistrationSystem (H 6x6, g,
    cost, n_used, n_located, origin) for the left update p <- Rot(w)(p - origin) + origin + v; .solve() is the
    Gauss-Newton step.  map: a Grid, an OctreeManager or an Octree.  The correspondence is that of
    nearest(transform_np(transform, points), k=1, max_distance=..., pose_numbers=...) exactly; the plane is the one of
    leaf_planes(pose_numbers) for the leaf the matched point lies in, under point_to_plane's gates min_points and
    max_variance - not the leaf of the query.  A point is used when it has a correspondence and that leaf an accepted
    plane; n_located counts the correspondences.  max_distance is the search radius alone: there is no gate on the
    residual.  huber_delta: Huber weights on |residual|; origin None: the centroid of the transformed scan;
    per_point: .neighbours (a Neighbours), .node, .row, .residual and .planes come back too.  Three kernels once the
    tables of the selection exist, one host wait (octreelib_amd/registration.py:
    nearest_plane_registration_system_np is the definition).  ValueError for a max_distance that is not finite and
    positive or, as for nearest, above twice the voxel edge on a Grid, and for an Octree with pose_numbers;
    RuntimeError after map_leaf_points moved rows outside their leaves; KeyError for an unknown pose; TypeError for
    another kind of map."""
    forest, host, sel, names = _resolve(map, pose_numbers, "nearest_plane_registration_system")
    if host is not None:
        return host.nearest_plane_registration_system(points, transform, max_distance=max_distance, pose_numbers=sel,
                                                      min_points=min_points, max_variance=max_variance,
                                                      huber_delta=huber_delta, origin=origin, per_point=per_point)
    return forest.nearest_plane_registration_system(points, transform, origin, sel, max_distance, min_points,
                                                    max_variance, huber_delta, per_point, names)


def align_nearest_planes(map, points, initial=None, *, max_distance: float, pose_numbers: Optional[List[int]] = None,
                         min_points: int = 8, max_variance: Optional[float] = None,
                         huber_delta: Optional[float] = None, max_iterations: int = 20, tolerance: float = 1e-9,
                         damping: float = 0.0) -> Alignment:
    """Gauss-Newton alignment of a scan to the map over nearest_plane_registration_system, from `initial` (None:
    identity): an Alignment (transform 4x4, iterations, converged, costs, n_used, reason).  A first guess that is off
    by several leaves - up to max_distance - still finds its planes, and the scan slides along them.  The planes and
    the block index are made once and the scan is uploaded once (or is a DeviceCloud of f64 points); an iteration is
    three kernels, a 240-byte download and a 6x6 solve on the host.  Ends when |xi| < tolerance, at max_iterations,
    or - not converged, last good transform - when fewer than six points are used.  Errors as
    nearest_plane_registration_system."""
    forest, host, sel, _ = _resolve(map, pose_numbers, "align_nearest_planes")
    if host is not None:
        return host.align_nearest_planes(points, initial, max_distance=max_distance, pose_numbers=sel,
                                         min_points=min_points, max_variance=max_variance, huber_delta=huber_delta,
                                         max_iterations=max_iterations, tolerance=tolerance, damping=damping)
    return forest.align_nearest_planes(points, initial, sel, max_distance, min_points, max_variance, huber_delta,
                                       max_iterations, tolerance, damping)
