"""
Grid of top-level voxels, multi-pose (reference: grid/grid.py:21-362), device resident.

insert_points uploads a pose; the voxel bucketing, the synchronised count-driven subdivision,
the leaf ordering, the per-leaf RANSAC and the mask application all run as HIP kernels behind
the C ABI (include/octreelib_hip.h).
"""

import os
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

import numpy as np

from octreelib_amd import _views
from octreelib_amd._engine import Forest
from octreelib_amd.criteria import try_count_threshold, try_planar_threshold
from octreelib_amd.grid.grid_base import GridBase, GridConfigBase, VisualizationConfig
from octreelib_amd.internal.voxel import Voxel
from octreelib_amd.leaf_stats import LeafStatistics, leaf_statistics_of_leaves
from octreelib_amd.query import HostMap, LeafPlanes, Neighbours, PlaneSegments, PointToPlane, RayEvidence, RayHits
from octreelib_amd.adjustment import Adjustment, AdjustmentSystem
from octreelib_amd.registration import Alignment, RegistrationSystem, host_transformed as _host_transformed

__all__ = ["Grid", "GridConfig"]

RANSAC_MAX_HYPOTHESES = 1024  # the reference's CUDA_THREADS (ransac/cuda_ransac.py:15)
_CHECKS = os.environ.get("OCTREELIB_AMD_CHECKS", "0") not in ("", "0")   # invariants asserted (the GPU tests set it)


@dataclass
class GridConfig(GridConfigBase):
    pass


class Grid(GridBase):
    def __init__(self, grid_config: GridConfig):
        super().__init__(grid_config)
        L = grid_config.voxel_edge_length
        corner = np.asarray(grid_config.corner, dtype=np.float64).reshape(3)
        if np.any(corner != 0.0):
            raise NotImplementedError(
                "GridConfig.corner != 0 is outside the parity domain: the reference stores voxel "
                "corners relative to the grid corner but its octrees subtract them from absolute "
                "points (grid.py:96-105 vs octree.py:74) and fail on subdivide"
            )
        if float(L) <= 0 or float(L) != int(L):
            raise NotImplementedError(
                "voxel_edge_length must be a positive integer value: the reference truncates "
                "voxel coordinates with astype(int) (grid.py:72-76), merging fractional voxels"
            )
        # the reference's plug seam (grid_base.py:66-87, grid.py:100-106): it instantiates
        # octree_manager_type(octree_type, octree_config, corner, L) per top-level voxel.  With the package's own
        # types the whole grid is ONE device-resident forest.
        from octreelib_amd.octree import Octree
        from octreelib_amd.octree_manager import OctreeManager

        self._slots: Dict[int, int] = {}  # pose number -> slot
        self._plug = None
        self._forest = None
        if grid_config.octree_manager_type is not OctreeManager or grid_config.octree_type is not Octree:
            # the caller's own types: served on the host, one manager_type(octree_type, config, corner, L) per
            # top-level voxel as the reference instantiates them (grid/_plugged.py) - slow and correct
            from octreelib_amd.grid._plugged import PluggedGrid

            self._plug = PluggedGrid(grid_config)
        else:
            self._forest = Forest(0, corner, float(L))

    # grid.py:58-109
    def insert_points(self, pose_number: int, points, *, transform=None, segment=None):
        """transform (no reference counterpart): a 3x4 or 4x4 - Alignment.transform goes straight in - under which
        the cloud is stored, moved by the ingest kernel on its way into the map: exactly what
        insert_points(pose_number, transform_rows_np(transform, points, segment)) leaves, without the host pass.  A
        stack (M, 3, 4) or (M, 4, 4), M <= 1024, with segment (n,), the index of every row's transform, deskews a
        sweep in the same pass.  points may be a host array (f64 or f32) or a DeviceCloud."""
        if self._plug is not None:
            if transform is not None or segment is not None:
                points = _host_transformed(points, transform, segment)
            return self._plug.insert_points(pose_number, points)
        if pose_number in self._slots:
            raise ValueError(f"Cannot insert points to existing pose {pose_number}")
        self._slots[pose_number] = self._forest.add_pose(points, transform, segment)

    # grid.py:244-258
    def subdivide(self, subdivision_criteria: List[Callable], pose_numbers: Optional[List[int]] = None):
        if self._plug is not None:
            return self._plug.subdivide(subdivision_criteria, pose_numbers)
        scheme = None if pose_numbers is None else [self._slots[p] for p in pose_numbers]
        rule = try_planar_threshold(subdivision_criteria)
        if rule is not None:
            return self._forest.subdivide_planar(rule, scheme)
        k = try_count_threshold(subdivision_criteria)
        if k is None:
            self._forest.subdivide_callable(subdivision_criteria, scheme)
        else:
            self._forest.subdivide(k, scheme)

    # grid.py:217-232
    def get_leaf_points(self, pose_number: int, non_empty: bool = True) -> List[Voxel]:
        if self._plug is not None:
            return self._plug.get_leaf_points(pose_number, non_empty)
        return _views.leaf_views(self._forest, self._slots[pose_number], non_empty)

    def leaf_statistics(self, pose_number: int) -> LeafStatistics:
        """Count, mean, covariance and its eigen-decomposition (least-squares plane) of every non-empty leaf of a
        pose: row i describes get_leaf_points(pose_number)[i].  One device call over the pose's blocks; a grid on
        the caller's own plug types computes it on the host from get_leaf_points.  KeyError for an unknown pose."""
        if self._plug is not None:
            return leaf_statistics_of_leaves(self._plug.get_leaf_points(pose_number, True))
        slot = self._slots[pose_number]
        self._forest.ensure_built()
        return self._forest.leaf_stats(self._forest.slot_blocks(slot))

    # -- queries: no reference counterpart (octreelib_amd/query.py holds the host definitions) ----------------------
    def _host_map(self) -> HostMap:
        plug = self._plug
        keys = sorted(plug._managers)
        roots = [(np.array(k, dtype=np.float64), float(plug._L)) for k in keys]
        leaves = {p: plug.get_leaf_points(p, False) for p in plug._pose_voxels}
        return HostMap(0, float(plug._L), roots, leaves)

    def _query_slots(self, pose_numbers):
        if self._plug is not None:
            for p in pose_numbers or ():
                self._plug._pose_voxels[p]   # KeyError for an unknown pose
            return pose_numbers
        return None if pose_numbers is None else [self._slots[p] for p in pose_numbers]

    def locate(self, points) -> np.ndarray:
        """int32 node id of the scheme leaf that every query point falls into - the leaf a point inserted as a late
        pose would land in; LeafView.node of get_leaf_points is the id to match against - or -1: no top-level voxel
        there, outside the voxel domain, not finite.  Read-only, one kernel.  Any (n, 3) array-like."""
        if self._plug is not None:
            return self._host_map().locate(points)
        return self._forest.locate(points)

    def nearest(self, points, k: int = 1, *, max_distance: float,
                pose_numbers: Optional[List[int]] = None) -> Neighbours:
        """The k <= 8 stored points of the given poses (None: all) nearest to every query point, within max_distance:
        exact neighbours across leaf and voxel walls.  A Neighbours (pose, index, distance2 (n, k), count (n,)): rows
        in ascending (distance2, insertion order of the pose, index), index = the point's row in the cloud that was
        inserted as that pose (masks and filters do not renumber it; removed points are never returned), pads -1 /
        -1 / +inf.  distance2 <= max_distance^2 inclusive; a query that is not finite finds nothing.  One kernel once
        the block index of the selection exists (octreelib_amd/query.py: nearest_np is the definition, bit for bit).
        ValueError for k outside 1 .. 8, a max_distance that is not finite and positive or above twice the voxel
        edge; RuntimeError after map_leaf_points moved rows outside their leaves; KeyError for an unknown pose."""
        sel = self._query_slots(pose_numbers)
        if self._plug is not None:
            return self._host_map().nearest(points, k, max_distance=max_distance, pose_numbers=sel)
        names = [p for p, _ in sorted(self._slots.items(), key=lambda kv: kv[1])]
        return self._forest.neighbours(points, k, max_distance, sel, names)

    def raycast(self, origins, directions, max_range, *, min_range=0.0, pose_numbers: Optional[List[int]] = None,
                surface: str = "cube", min_points: Optional[int] = None,
                max_variance: Optional[float] = None) -> RayHits:
        """What every ray hits first: for n rays from `origins` (n, 3) along `directions` (n, 3; normalised here, any
        length; a zero vector hits nothing) between min_range and max_range (scalars or (n,)), the first occupied
        leaf (surface="cube": at least min_points, default 1, alive points of the given poses - None: all - and t
        where the ray enters its cube) or the first accepted leaf plane (surface="plane": the pooled plane of
        leaf_planes(pose_numbers) under point_to_plane's gates, min_points default 8 and max_variance, where the ray
        meets it inside the leaf's cube).  A RayHits (node, t, row (n,); .hit, .points(origins, directions)): node -1,
        t +inf, row -1 where nothing is hit or the ray is dead (a value that is not finite, max_range < min_range);
        ties in t go to the smaller node id.  One kernel once the tables of the selection exist
        (octreelib_amd/query.py: raycast_np is the definition, bit for bit).  ValueError for shapes that do not fit, an
        unknown surface, a ray that spans more than 256 voxel edges; RuntimeError after map_leaf_points moved rows
        outside their leaves; KeyError for an unknown pose."""
        sel = self._query_slots(pose_numbers)
        if self._plug is not None:
            return self._host_map().raycast(origins, directions, max_range, min_range=min_range, pose_numbers=sel,
                                            surface=surface, min_points=min_points, max_variance=max_variance)
        return self._forest.raycast(origins, directions, max_range, min_range, sel, surface, min_points, max_variance)

    def ray_evidence(self, origins, directions, ranges, margin, min_range=0.0, returned=None) -> RayEvidence:
        """Free-space evidence of a scan: for n rays from `origins` (n, 3) along `directions` (n, 3; normalised here)
        with measured `ranges` (scalar or (n,)), how many rays END in every leaf of the scheme and how many only pass
        THROUGH it.  A ray is free over [min_range, range - margin] and ends in [range - margin, range + margin]
        (margin finite and >= 0: the range noise plus what the surface may have moved); a leaf the end interval
        crosses gets a hit, a leaf only the free interval crosses gets a through; rays with returned == False (no
        echo) are free up to range - margin and end nowhere.  A RayEvidence (through, hits (n_nodes,) uint32 over the
        rows of node_cubes(); `+` adds the evidence of two scans; .free(min_through, max_hits) the nodes carve would
        empty).  The scheme and the rays alone decide - no occupancy, no pose selection; a dead ray (a value that is
        not finite) adds nothing.  One kernel (octreelib_amd/query.py: ray_evidence_np is the definition, count for
        count).  ValueError for shapes that do not fit, a bad margin, a ray that spans more than 256 voxel edges."""
        if self._plug is not None:
            return self._host_map().ray_evidence(origins, directions, ranges, margin, min_range, returned)
        return self._forest.ray_evidence(origins, directions, ranges, margin, min_range, returned)

    def carve(self, evidence: RayEvidence, min_through: int = 2, max_hits: int = 0,
              pose_numbers: Optional[List[int]] = None) -> int:
        """Remove what rays saw through: every leaf of the given poses (None: all) that at least min_through rays
        passed through and at most max_hits rays ended in loses its points of those poses - things that have moved
        away since the poses were taken.  Evidence belongs to the scheme it was taken on (ray_evidence of this map as
        it is subdivided now; several scans summed with `+`).  The scheme stays, a pending RANSAC mask is applied in
        the same compaction, every cached table is dropped.  Returns the number of points removed.  ValueError when
        the evidence is not over this map's nodes, min_through < 1 or max_hits < 0; KeyError for an unknown pose;
        NotImplementedError on the caller's own plug types."""
        if self._plug is not None:
            raise NotImplementedError(
                "carve removes points of the device-resident map: a Grid on the caller's own plug types keeps its "
                "points in those types on the host, and there is no host path for them")
        sel = None if pose_numbers is None else [self._slots[p] for p in pose_numbers]
        return self._forest.carve(evidence, min_through, max_hits, sel)

    def carve_rays(self, origins, directions, ranges, margin, min_range=0.0, returned=None, min_through: int = 2,
                   max_hits: int = 0, pose_numbers: Optional[List[int]] = None) -> int:
        """carve(ray_evidence(...)) in one go on the device: the counters are never downloaded.  Returns the number
        of points removed."""
        if self._plug is not None:
            raise NotImplementedError(
                "carve_rays removes points of the device-resident map: a Grid on the caller's own plug types keeps "
                "its points in those types on the host, and there is no host path for them")
        sel = None if pose_numbers is None else [self._slots[p] for p in pose_numbers]
        return self._forest.carve_rays(origins, directions, ranges, margin, min_range, returned, min_through,
                                       max_hits, sel)

    def radius_count(self, points, radius, *, max_count: Optional[int] = None,
                     pose_numbers: Optional[List[int]] = None) -> np.ndarray:
        """How many stored points of the given poses (None: all) lie within `radius` of every query point: (n,) int32,
        min(count, max_count) with max_count None: uncapped - density gates, occupancy tests for new scan points,
        adaptive radii.  The counted points are exactly the candidates of nearest (distance2 <= radius^2 inclusive;
        what a mask, a filter, carve or remove_poses took out never counts) without its limit of 8; a query that is
        not finite counts 0; a capped query stops searching at the cap.  points: any (n, 3) array-like, or a
        DeviceCloud of float64 points, read where it lies.  One kernel once the block index of the selection exists
        (octreelib_amd/query.py: radius_count_np is the definition, count for count).  ValueError for a radius that
        is not finite and positive or above twice the voxel edge, or a max_count that is not an integer in
        1 .. 2^31 - 1; RuntimeError after map_leaf_points moved rows outside their leaves; KeyError for an unknown
        pose."""
        sel = self._query_slots(pose_numbers)
        if self._plug is not None:
            return self._host_map().radius_count(points, radius, max_count=max_count, pose_numbers=sel)
        return self._forest.radius_count(points, radius, max_count, sel)

    def remove_sparse(self, radius, min_neighbours: int, *, pose_numbers: Optional[List[int]] = None,
                      among: Optional[List[int]] = None) -> int:
        """Radius outlier removal: every stored point of the given poses (None: all) that has fewer than
        min_neighbours OTHER stored points of the poses of `among` (None: all) within `radius` leaves the map - sensor
        speckle, the halo carve leaves round a removed object, single returns from rain, dust and glass.
        pose_numbers=[newest], among=None cleans a new scan against the whole map.  A point never counts itself, a
        duplicate at the same coordinates does; every decision is made on the map as it is before the call (one
        simultaneous round: a second call may remove more); points a pending RANSAC mask is about to drop still count
        and are judged, and that mask is applied in the same compaction.  The scheme stays (prune() afterwards drops
        what became empty), every cached table is dropped, Neighbours.index of the surviving rows is unchanged.  One
        kernel and the compaction (octreelib_amd/query.py: sparse_keep_np is the rule).  Returns the number of points
        removed.  ValueError for a radius that is not finite and positive or above twice the voxel edge, or a
        min_neighbours that is not an integer in 1 .. 2^31 - 1; RuntimeError after map_leaf_points moved rows outside
        their leaves; KeyError for an unknown pose; NotImplementedError on the caller's own plug types."""
        if self._plug is not None:
            raise NotImplementedError(
                "remove_sparse removes points of the device-resident map: a Grid on the caller's own plug types keeps "
                "its points in those types on the host (HostMap.remove_sparse gives the decision)")
        sel = None if pose_numbers is None else [self._slots[p] for p in pose_numbers]
        asel = None if among is None else [self._slots[p] for p in among]
        return self._forest.remove_sparse(radius, min_neighbours, sel, asel)

    def leaf_planes(self, pose_numbers: Optional[List[int]] = None) -> LeafPlanes:
        """One least-squares plane per leaf over the given poses (None: all), all their points pooled: a LeafPlanes in
        ascending node id.  KeyError for an unknown pose."""
        sel = self._query_slots(pose_numbers)
        if self._plug is not None:
            return self._host_map().leaf_planes(sel)
        return self._forest.leaf_planes(sel)

    def plane_segments(self, pose_numbers: Optional[List[int]] = None, min_points: int = 8,
                       max_variance: Optional[float] = None, max_angle: float = 0.1,
                       max_offset: float = 0.05) -> PlaneSegments:
        """The leaves of leaf_planes(pose_numbers) merged across their faces into connected coplanar segments - plane
        landmarks (a floor, a wall) instead of hundreds of leaves: a PlaneSegments (planes, neighbour (rows, 6) node
        ids behind the faces -x +x -y +y -z +z, label (rows,) segment of a row or -1, segments = one merged plane per
        segment with root and n_leaves).  A row takes part with at least min_points points and a smallest eigenvalue
        that is finite and at most max_variance; two face neighbours are joined when their normals are within
        max_angle and each plane passes within max_offset of the other's mean.  Computed on the device and cached
        until the map changes (octreelib_amd/query.py: plane_segments_np is the definition; neighbour, label, root
        and n_leaves equal it exactly).  ValueError for max_angle outside [0, pi/2], a max_offset that is negative or
        not finite, min_points < 1; KeyError for an unknown pose."""
        sel = self._query_slots(pose_numbers)
        if self._plug is not None:
            return self._host_map().plane_segments(sel, min_points, max_variance, max_angle, max_offset)
        return self._forest.plane_segments(sel, min_points, max_variance, max_angle, max_offset)

    def point_to_plane(self, points, pose_numbers: Optional[List[int]] = None, min_points: int = 8,
                       max_variance: Optional[float] = None) -> PointToPlane:
        """Leaf, plane row and signed distance to the pooled plane of its own leaf for every query point; row -1 and
        distance NaN where the point has no leaf or the leaf no accepted plane (fewer than min_points pooled points,
        smallest eigenvalue above max_variance).  One fused kernel; the pooled planes are recomputed only when the
        grid has changed or the pose selection is another one."""
        sel = self._query_slots(pose_numbers)
        if self._plug is not None:
            return self._host_map().point_to_plane(points, sel, min_points, max_variance)
        return self._forest.point_to_plane(points, sel, min_points, max_variance)

    def registration_system(self, points, transform=None, pose_numbers: Optional[List[int]] = None,
                            min_points: int = 8, max_variance: Optional[float] = None,
                            max_distance: Optional[float] = None, huber_delta: Optional[float] = None, origin=None,
                            per_point: bool = False) -> RegistrationSystem:
        """The point-to-plane normal equations of a scan under `transform` (4x4 or 3x4, None: identity) against the
        pooled leaf planes: a RegistrationSystem (H 6x6, g, cost, n_used, n_located, origin) for the left update
        p <- Rot(w)(p - origin) + origin + v; .solve() is the Gauss-Newton step.  Gates as point_to_plane, plus
        max_distance (points with a larger |residual| are not used) and huber_delta (Huber weights); origin None: the
        centroid of the transformed scan; per_point: node / row / residual of every point come back too.  Two kernels
        and one host wait (octreelib_amd/registration.py has the definition)."""
        sel = self._query_slots(pose_numbers)
        if self._plug is not None:
            return self._host_map().registration_system(points, transform, sel, min_points, max_variance,
                                                        max_distance, huber_delta, origin, per_point)
        return self._forest.registration_system(points, transform, origin, sel, min_points, max_variance,
                                                max_distance, huber_delta, per_point)

    def align(self, points, initial=None, pose_numbers: Optional[List[int]] = None, min_points: int = 8,
              max_variance: Optional[float] = None, max_distance: Optional[float] = None,
              huber_delta: Optional[float] = None, max_iterations: int = 20, tolerance: float = 1e-9,
              damping: float = 0.0) -> Alignment:
        """Gauss-Newton alignment of a scan to the map, from `initial` (None: identity): an Alignment (transform 4x4,
        iterations, converged, costs, n_used, reason).  The planes are made once and the scan is uploaded once; an
        iteration is two kernels, a 240-byte download and a 6x6 solve on the host.  Ends when |xi| < tolerance, at
        max_iterations, or - not converged, last good transform - when fewer than six points are used."""
        sel = self._query_slots(pose_numbers)
        if self._plug is not None:
            return self._host_map().align(points, initial, sel, min_points, max_variance, max_distance, huber_delta,
                                          max_iterations, tolerance, damping)
        return self._forest.align(points, initial, sel, min_points, max_variance, max_distance, huber_delta,
                                  max_iterations, tolerance, damping)

    def point_registration_system(self, points, transform=None, *, max_distance: float,
                                  pose_numbers: Optional[List[int]] = None, huber_delta: Optional[float] = None,
                                  origin=None, per_point: bool = False) -> RegistrationSystem:
        """The point-to-point normal equations of a scan under `transform` (4x4 or 3x4, None: identity) against the
        NEAREST STORED POINT of the given poses (None: all) within max_distance - classic ICP for maps without planes
        (vegetation, rubble, a sparse first scan): a RegistrationSystem (H 6x6, g, cost, n_used, n_located, origin)
        for the left update p <- Rot(w)(p - origin) + origin + v; .solve() is the Gauss-Newton step.  The
        correspondences are those of nearest(transform_np(transform, points), k=1, max_distance=...) exactly; a point
        without one is not used; huber_delta: Huber weights on the distance; origin None: the centroid of the
        transformed scan; per_point: the Neighbours come back in .neighbours.  Three kernels once the block index of
        the selection exists, one host wait (octreelib_amd/registration.py: point_registration_system_np is the
        definition).  ValueError for a max_distance that is not finite and positive or above twice the voxel edge;
        RuntimeError after map_leaf_points moved rows outside their leaves; KeyError for an unknown pose."""
        sel = self._query_slots(pose_numbers)
        if self._plug is not None:
            return self._host_map().point_registration_system(points, transform, max_distance=max_distance,
                                                              pose_numbers=sel, huber_delta=huber_delta,
                                                              origin=origin, per_point=per_point)
        names = [p for p, _ in sorted(self._slots.items(), key=lambda kv: kv[1])]
        return self._forest.point_registration_system(points, transform, origin, sel, max_distance, huber_delta,
                                                      per_point, names)

    def align_points(self, points, initial=None, *, max_distance: float, pose_numbers: Optional[List[int]] = None,
                     huber_delta: Optional[float] = None, max_iterations: int = 20, tolerance: float = 1e-9,
                     damping: float = 0.0) -> Alignment:
        """Gauss-Newton alignment of a scan to the nearest stored points, from `initial` (None: identity): an
        Alignment (transform 4x4, iterations, converged, costs, n_used, reason).  The block index is made once and the
        scan is uploaded once (or is a DeviceCloud of f64 points); an iteration is three kernels, a 240-byte download
        and a 6x6 solve on the host.  Ends when |xi| < tolerance, at max_iterations, or - not converged, last good
        transform - when fewer than six points are used."""
        sel = self._query_slots(pose_numbers)
        if self._plug is not None:
            return self._host_map().align_points(points, initial, max_distance=max_distance, pose_numbers=sel,
                                                 huber_delta=huber_delta, max_iterations=max_iterations,
                                                 tolerance=tolerance, damping=damping)
        return self._forest.align_points(points, initial, sel, max_distance, huber_delta, max_iterations, tolerance,
                                         damping)

    def adjustment_system(self, transforms=None, pose_numbers: Optional[List[int]] = None, origin=None,
                          min_points: int = 8, min_poses: int = 2, max_variance: Optional[float] = None,
                          leaves: bool = False) -> AdjustmentSystem:
        """The plane-adjustment systems of the given poses (None: all) at one rigid transform per pose (4x4 or 3x4,
        increments applied to the points as they were inserted; None: identities, in the order the poses were
        inserted): an AdjustmentSystem (H (S, 6, 6), g, cost per pose, total_cost, n_points, n_blocks, n_leaves,
        origin) against the leaf planes pooled AT those transforms; .solve() is one block-Jacobi step.  A leaf is used
        with at least min_points pooled points, min_poses poses that see it and a smallest eigenvalue of at most
        max_variance; origin None: the centre of the box of the top-level voxels; leaves: the leaf table and the
        block moments come back too.  The map is reduced to 80 bytes per (leaf, pose) block once; a call reads no
        point: three kernels and one host wait (octreelib_amd/adjustment.py has the definition)."""
        sel = self._query_slots(pose_numbers)
        if self._plug is not None:
            return self._host_map().adjustment_system(transforms, sel, origin, min_points, min_poses, max_variance,
                                                      leaves)
        return self._forest.adjustment_system(transforms, sel, origin, min_points, min_poses, max_variance, leaves,
                                              self._adjust_names(pose_numbers))

    def adjust(self, initial=None, pose_numbers: Optional[List[int]] = None, origin=None, min_points: int = 8,
               min_poses: int = 2, max_variance: Optional[float] = None, fixed=None, max_iterations: int = 200,
               tolerance: float = 1e-9, damping: float = 0.0) -> Adjustment:
        """Block-Jacobi plane adjustment of the given poses from `initial` (None: identities): an Adjustment
        (transforms (S, 4, 4), iterations, converged, costs, reason).  `fixed` (pose numbers; None: the first selected
        pose) stay where they are.  Per iteration T_p <- se3_exp(xi_p, origin) T_p; ends when max |xi_p| < tolerance,
        at max_iterations, or - not converged, last good transforms - when a free pose has fewer than six used
        points.  The transforms are returned; transform_poses writes them back into the map."""
        sel = self._query_slots(pose_numbers)
        if self._plug is not None:
            return self._host_map().adjust(initial, sel, origin, min_points, min_poses, max_variance, fixed,
                                           max_iterations, tolerance, damping)
        return self._forest.adjust(initial, sel, origin, min_points, min_poses, max_variance, fixed, max_iterations,
                                   tolerance, damping, self._adjust_names(pose_numbers))

    def transform_poses(self, transforms, pose_numbers: Optional[List[int]] = None) -> None:
        """Write poses back into the map: move the stored points of the given poses (None: all) by one rigid transform
        each (4x4 or 3x4, in the order the poses were inserted - Adjustment.transforms of the same pose_numbers can be
        passed straight in), in place on the device.  A point p of a selected pose becomes transform_np(T, p), bit for
        bit; the points of the other poses keep their bits; points that a mask or filter removed stay removed.
        Afterwards the map is what a fresh Grid would be after inserting every pose again with its surviving points
        as moved: no subdivision, the top-level voxels the moved points fall into, every cached table dropped -
        subdivide, fit planes and adjust again - except that Neighbours.index still names rows of the clouds as they
        were first inserted.  Transactional: DomainError (a moved point is not finite or falls outside the voxel
        domain) leaves the map exactly as it was.  One kernel over the stored points and one host wait
        (octl_forest_transform_poses).  ValueError for transforms that are not one valid transform per selected pose;
        KeyError for an unknown pose; NotImplementedError on the caller's own plug types."""
        if self._plug is not None:
            raise NotImplementedError(
                "transform_poses moves the points of the device-resident map: a Grid on the caller's own plug types "
                "keeps its points in those types on the host, and there is no host path for them")
        sel = None if pose_numbers is None else [self._slots[p] for p in pose_numbers]
        self._forest.transform_poses(transforms, sel)

    def remove_poses(self, pose_numbers: List[int]) -> int:
        """Let go of poses: afterwards the map is the map as it was with those poses absent.  The subdivision, the
        voxels and their creation order stay, as after carve (voxels and leaves only a removed pose populated stay,
        empty; ray evidence stays valid); every remaining pose reads back the same bits from get_points,
        get_leaf_points, leaf_statistics and the counters, and its rows keep their Neighbours.index; a query over
        every pose answers what it answered over the remaining poses before.  The pose numbers are free again -
        insert_points with one of them adds a new pose, which inherits the subdivision as any late pose does - and
        the point store on the device shrinks to the remaining poses' rows with its voxel box folded again, so a
        sliding window holds bounded memory and does not carry the box of everywhere it has been.  A pending RANSAC
        mask is applied in the same compaction; every cached table is dropped.  Launches and host waits do not depend
        on the number of points (octl_forest_remove_poses).  Returns the number of stored points that left.  KeyError
        for an unknown pose; ValueError on the caller's own plug types."""
        if self._plug is not None:
            raise ValueError(
                "remove_poses removes points of the device-resident map: a Grid on the caller's own plug types keeps "
                "its points in those types on the host, and there is no host path for them")
        slots = [self._slots[p] for p in pose_numbers]   # KeyError for an unknown pose, before anything changes
        gone = set(pose_numbers)
        new_slot, removed = self._forest.remove_slots(slots)
        self._slots = {p: int(new_slot[s]) for p, s in self._slots.items() if p not in gone}
        return removed

    def prune(self):
        """Make the subdivision follow the points again, on the device: top-level voxels that hold no point of any
        pose any more (after carve, filter, a RANSAC mask that was applied, remove_poses) leave the map with their
        whole subtree, and an internal node below which no point is left becomes a leaf; an internal node that stays
        keeps all eight children, empty ones included.  Nothing calls this implicitly.  Every read of every pose
        gives the same points, leaves and statistics as before, minus the empty leaves that are gone; points, their
        order and a pending RANSAC mask are not touched (prune after the mask is applied: what a pending mask will
        empty still counts as occupied).  Node ids change: the PruneResult returned maps them (node_map, old_node),
        and RayEvidence.remapped(result) carries evidence over.  A pose that no longer has a voxel it was inserted
        into no longer lists that voxel's (empty) leaves.  A later scan that falls into a dropped voxel creates it
        anew, as any voxel seen for the first time: an unsplit root at the END of the creation order, until the next
        subdivide.  Launches and host waits do not depend on the number of points, nodes or levels
        (octl_forest_prune).  ValueError on the caller's own plug types."""
        if self._plug is not None:
            raise ValueError(
                "prune renumbers the scheme of the device-resident map: a Grid on the caller's own plug types keeps "
                "its points in those types on the host, and there is no host path for them")
        return self._forest.prune()

    def _adjust_names(self, pose_numbers):
        """The selected pose numbers in ascending slot order: the order of the transforms and of every result row."""
        chosen = self._slots if pose_numbers is None else set(pose_numbers)
        return [p for p, _ in sorted(self._slots.items(), key=lambda kv: kv[1]) if p in chosen]

    def node_cubes(self):
        """(corner (N, 3), edge (N,)) of every node id that locate / leaf_planes can name."""
        nd = self._host_map().nodes if self._plug is not None else self._forest.nodes
        return nd["corner"].copy(), nd["edge"].copy()

    # grid.py:234-242: all managers in first-creation order, DFS order inside a manager
    def get_points(self, pose_number: int):
        if self._plug is not None:
            return self._plug.get_points(pose_number)
        f = self._forest
        slot = self._slots[pose_number]
        blk = f.blocks
        sel = np.nonzero(blk["slot"] == slot)[0]
        if len(sel) == 0:
            return np.empty((0, 3), dtype=float)
        vox_rank = f.nodes["voxel"][blk["node"][sel]]
        creation = f.creation_ranks(f.voxels)[vox_rank]
        # managers in creation order, storage order inside one (= the DFS order of octree.get_points); a grid whose
        # voxels were created in voxel order - one pose, or poses over the same voxels - is in that order already.
        # INVARIANT the shortcut relies on: the block table is in storage order - `start` strictly ascending over the
        # non-empty blocks (forest.h: "block table of non-empty (leaf, pose) runs in storage order") - so that equal
        # creation ranks are already ordered by start.  OCTREELIB_AMD_CHECKS=1 verifies it.
        if _CHECKS and len(sel) > 1:
            assert np.all(np.diff(blk["start"][sel].astype(np.int64)) > 0), "block table out of storage order"
        if len(sel) > 1 and np.any(creation[1:] < creation[:-1]):
            sel = sel[np.lexsort((blk["start"][sel], creation))]
        return f.gather_blocks(sel)

    # grid.py:260-267
    def filter(self, filtering_criteria: List[Callable]):
        if self._plug is not None:
            return self._plug.filter(filtering_criteria)
        _views.filter_slots(self._forest, list(self._slots.values()), filtering_criteria)

    # grid.py:111-122
    def map_leaf_points(self, function: Callable, pose_numbers: Optional[List[int]] = None):
        if self._plug is not None:
            return self._plug.map_leaf_points(function, pose_numbers)
        if pose_numbers is None:
            slots = list(self._slots.values())
        else:
            slots = [self._slots[p] for p in pose_numbers if p in self._slots]
        _views.map_slots(self._forest, slots, function)

    # grid.py:124-215
    def map_leaf_points_cuda_ransac(
        self,
        poses_per_batch: int = 10,
        threshold: float = 0.01,
        hypotheses_number: int = 1024,
        initial_points_number: int = 6,
        *,
        hypotheses=None,
    ):
        """`hypotheses` (extension, keyword only): the (H, k) table itself instead of one drawn from NumPy's global
        generator - for callers that fit scans from several threads (octreelib_amd.ScanPipeline) and want every
        scan to see the same table without serialising on the generator."""
        if hypotheses is not None:
            hypotheses = np.ascontiguousarray(hypotheses, dtype=np.float64)
            if hypotheses.ndim != 2:
                raise ValueError("hypotheses must be an (H, k) table")
            hypotheses_number, initial_points_number = hypotheses.shape
        if threshold <= 0:
            raise ValueError("Threshold must be positive")
        if hypotheses_number < 1:
            raise ValueError("Number of RANSAC hypotheses must be positive")
        if hypotheses_number > RANSAC_MAX_HYPOTHESES:
            raise ValueError(
                "Number of RANSAC hypotheses must be <= 1024 "
                "because of the CUDA thread limit."
            )
        if self._plug is not None:
            return self._plug.ransac(poses_per_batch, threshold, min(hypotheses_number, RANSAC_MAX_HYPOTHESES),
                                     initial_points_number, hypotheses)
        f = self._forest
        n_poses = len(self._slots)
        if n_poses == 0:
            return
        # the hypothesis table: ONE draw from NumPy's global generator, shared by all leaves
        # and batches (ransac/cuda_ransac.py:39-41)
        if hypotheses is not None:
            table = hypotheses
        else:
            table = np.random.random((min(hypotheses_number, RANSAC_MAX_HYPOTHESES), initial_points_number))
        # batches are ranges of pose INDICES used as pose numbers (grid.py:149-157)
        for p in range(n_poses):
            if p not in self._slots:
                raise KeyError(p)
        if all(self._slots[p] == p for p in range(n_poses)):
            f.ransac_all(poses_per_batch, table, threshold)  # order + kernel on the device
        else:
            for i in range(0, n_poses, poses_per_batch):
                batch = range(i, min(i + poses_per_batch, n_poses))
                order = np.concatenate([f.slot_blocks(self._slots[p]) for p in batch])
                f.ransac_blocks(order, table, threshold)
        f.apply_device_mask()  # grid.py:203-215 -> apply_mask: outliers leave the tree

    def visualize(self, config: VisualizationConfig = VisualizationConfig()) -> None:
        raise NotImplementedError("Grid.visualize (k3d HTML export) is out of scope of this build")

    # grid.py:343-362
    def n_leaves(self, pose_number: int) -> int:
        if self._plug is not None:
            return self._plug.count("n_leaves", pose_number)
        return self._forest.n_leaves(self._slots[pose_number])

    def n_points(self, pose_number: int) -> int:
        if self._plug is not None:
            return self._plug.count("n_points", pose_number)
        return self._forest.n_points(self._slots[pose_number])

    def n_nodes(self, pose_number: int) -> int:
        if self._plug is not None:
            return self._plug.count("n_nodes", pose_number)
        return self._forest.n_nodes(self._slots[pose_number])
