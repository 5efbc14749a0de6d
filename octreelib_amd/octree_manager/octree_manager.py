"""
One cube, many poses, one shared subdivision scheme (reference: octree_manager/
octree_manager.py:12-180).  The scheme is built on the device from the union of the selected
poses' points and every pose is placed in it (octreelib_amd/csrc/build.hip).
"""

from typing import Callable, Dict, List, Optional, Type

import numpy as np

from octreelib_amd import _views
from octreelib_amd._engine import Forest
from octreelib_amd.criteria import try_count_threshold, try_planar_threshold
from octreelib_amd.internal.voxel import Voxel, VoxelBase
from octreelib_amd.leaf_stats import LeafStatistics, leaf_statistics_of_leaves
from octreelib_amd.octree.octree_base import OctreeBase, OctreeConfigBase
from octreelib_amd.query import HostMap, LeafPlanes, Neighbours, PlaneSegments, PointToPlane, RayEvidence, RayHits
from octreelib_amd.adjustment import Adjustment, AdjustmentSystem
from octreelib_amd.registration import Alignment, RegistrationSystem, host_transformed as _host_transformed

__all__ = ["OctreeManager"]


class OctreeManager(VoxelBase):
    def __init__(
        self,
        octree_type: Type[OctreeBase],
        octree_config: OctreeConfigBase,
        corner_min,
        edge_length: float,
    ):
        super().__init__(corner_min, edge_length)
        self._octree_type = octree_type
        self._octree_config = octree_config
        self._slots: Dict[int, int] = {}  # pose number -> slot (insertion order)
        # the plug seam (grid_base.py:66-68): a caller's OWN octree type is instantiated per pose and driven through
        # its public interface on the host (octree_manager/_plugged.py); octreelib_amd's Octree means "one forest"
        from octreelib_amd.octree import Octree

        self._plug = None
        self._forest = None
        if octree_type is not Octree:
            from octreelib_amd.octree_manager._plugged import PluggedPoses

            self._plug = PluggedPoses(octree_type, octree_config, corner_min, edge_length)
        else:
            self._forest = Forest(1, np.asarray(corner_min, dtype=np.float64), float(edge_length))

    # octree_manager.py:161-171
    def insert_points(self, pose_number: int, points, *, transform=None, segment=None):
        """transform / segment (no reference counterpart): the cloud is stored under the transform(s), as
        Grid.insert_points describes; a second call on a pose extends it."""
        if self._plug is not None:
            if transform is not None or segment is not None:
                points = _host_transformed(points, transform, segment)
            return self._plug.insert_points(pose_number, points)
        if pose_number not in self._slots:
            self._slots[pose_number] = self._forest.add_pose(points, transform, segment)
        else:
            self._forest.extend_pose(self._slots[pose_number], points, transform, segment)

    # octree_manager.py:36-66
    def subdivide(self, subdivision_criteria: List[Callable], pose_numbers: Optional[List[int]] = None):
        if self._plug is not None:
            return self._plug.subdivide(subdivision_criteria, pose_numbers)
        rule = try_planar_threshold(subdivision_criteria)
        k = None if rule is not None else try_count_threshold(subdivision_criteria)
        if pose_numbers is None:
            scheme = None
        else:
            scheme = [self._slots[p] for p in pose_numbers]  # KeyError for an unknown pose, as upstream
        if rule is not None:
            self._forest.subdivide_planar(rule, scheme)
        elif k is None:
            self._forest.subdivide_callable(subdivision_criteria, scheme)
        else:
            self._forest.subdivide(k, scheme)

    def _selected(self, pose_numbers):
        if pose_numbers is None:
            return list(self._slots.values())
        return [self._slots[p] for p in pose_numbers if p in self._slots]

    def map_leaf_points(self, function: Callable, pose_numbers: Optional[List[int]] = None):
        if self._plug is not None:
            return self._plug.map_leaf_points(function, pose_numbers)
        _views.map_slots(self._forest, self._selected(pose_numbers), function)

    def filter(self, filtering_criteria: List[Callable], pose_numbers: Optional[List[int]] = None):
        if self._plug is not None:
            return self._plug.filter(filtering_criteria, pose_numbers)
        slots = list(self._slots.values()) if pose_numbers is None else [self._slots[p] for p in pose_numbers]
        _views.filter_slots(self._forest, slots, filtering_criteria)

    # octree_manager.py:101-119 (note the argument order)
    def get_leaf_points(self, non_empty: bool = True, pose_number: Optional[int] = None) -> List[Voxel]:
        if self._plug is not None:
            return self._plug.get_leaf_points(non_empty, pose_number)
        if pose_number is None:
            return sum((_views.leaf_views(self._forest, s, non_empty) for s in self._slots.values()), [])
        if pose_number in self._slots:
            return _views.leaf_views(self._forest, self._slots[pose_number], non_empty)
        return []

    def leaf_statistics(self, pose_number: int) -> LeafStatistics:
        """Count, mean, covariance and its eigen-decomposition (least-squares plane) of every non-empty leaf of a
        pose: row i describes get_leaf_points(True, pose_number)[i].  One device call over the pose's blocks; a
        manager on the caller's own octree type computes it on the host.  KeyError for an unknown pose."""
        if self._plug is not None:
            if pose_number not in self._plug.octrees:
                raise KeyError(pose_number)
            return leaf_statistics_of_leaves(self._plug.get_leaf_points(True, pose_number))
        slot = self._slots[pose_number]
        self._forest.ensure_built()
        return self._forest.leaf_stats(self._forest.slot_blocks(slot))

    # -- queries: no reference counterpart (octreelib_amd/query.py holds the host definitions) ----------------------
    def _host_map(self) -> HostMap:
        roots = [(np.asarray(self.corner_min, dtype=np.float64), float(self.edge_length))]
        leaves = {p: self._plug.get_leaf_points(False, p) for p in self._plug.octrees}
        return HostMap(1, float(self.edge_length), roots, leaves)

    def _query_slots(self, pose_numbers):
        if self._plug is not None:
            for p in pose_numbers or ():
                self._plug.octrees[p]   # KeyError for an unknown pose
            return pose_numbers
        return None if pose_numbers is None else [self._slots[p] for p in pose_numbers]

    def locate(self, points) -> np.ndarray:
        """int32 node id of the scheme leaf every query point falls into (LeafView.node), -1 outside the cube or
        for a point that is not finite.  Read-only, one kernel."""
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
        ValueError for k outside 1 .. 8 or a max_distance that is not finite and positive; RuntimeError after
        map_leaf_points moved rows outside their leaves; KeyError for an unknown pose."""
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
        (octreelib_amd/query.py: raycast_np is the definition, bit for bit).  ValueError for shapes that do not fit or an
        unknown surface (one cube has no cap on the range); RuntimeError after map_leaf_points moved rows
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
        count).  ValueError for shapes that do not fit, a bad margin (one cube has no cap on the range)."""
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
                "carve removes points of the device-resident map: an OctreeManager on the caller's own plug types keeps its "
                "points in those types on the host, and there is no host path for them")
        sel = None if pose_numbers is None else [self._slots[p] for p in pose_numbers]
        return self._forest.carve(evidence, min_through, max_hits, sel)

    def carve_rays(self, origins, directions, ranges, margin, min_range=0.0, returned=None, min_through: int = 2,
                   max_hits: int = 0, pose_numbers: Optional[List[int]] = None) -> int:
        """carve(ray_evidence(...)) in one go on the device: the counters are never downloaded.  Returns the number
        of points removed."""
        if self._plug is not None:
            raise NotImplementedError(
                "carve_rays removes points of the device-resident map: an OctreeManager on the caller's own plug types keeps "
                "its points in those types on the host, and there is no host path for them")
        sel = None if pose_numbers is None else [self._slots[p] for p in pose_numbers]
        return self._forest.carve_rays(origins, directions, ranges, margin, min_range, returned, min_through,
                                       max_hits, sel)

    def radius_count(self, points, radius, *, max_count: Optional[int] = None,
                     pose_numbers: Optional[List[int]] = None) -> np.ndarray:
        """How many stored points of the given poses (None: all) lie within `radius` of every query point, capped at
        max_count (None: uncapped): (n,) int32; Grid.radius_count describes it (one cube has no cap on the radius).
        ValueError for a radius that is not finite and positive or a max_count that is not an integer in 1 .. 2^31 - 1;
        RuntimeError after map_leaf_points moved rows outside their leaves; KeyError for an unknown pose."""
        sel = self._query_slots(pose_numbers)
        if self._plug is not None:
            return self._host_map().radius_count(points, radius, max_count=max_count, pose_numbers=sel)
        return self._forest.radius_count(points, radius, max_count, sel)

    def remove_sparse(self, radius, min_neighbours: int, *, pose_numbers: Optional[List[int]] = None,
                      among: Optional[List[int]] = None) -> int:
        """Radius outlier removal: every point of the given poses (None: all) with fewer than min_neighbours other
        points of the poses of `among` (None: all) within `radius` leaves the map; Grid.remove_sparse describes it.
        Returns the number of points removed.  NotImplementedError on the caller's own plug types."""
        if self._plug is not None:
            raise NotImplementedError(
                "remove_sparse removes points of the device-resident map: an OctreeManager on the caller's own plug "
                "types keeps its points in those types on the host (HostMap.remove_sparse gives the decision)")
        sel = None if pose_numbers is None else [self._slots[p] for p in pose_numbers]
        asel = None if among is None else [self._slots[p] for p in among]
        return self._forest.remove_sparse(radius, min_neighbours, sel, asel)

    def leaf_planes(self, pose_numbers: Optional[List[int]] = None) -> LeafPlanes:
        """One least-squares plane per leaf over the given poses (None: all), their points pooled; ascending node id.
        KeyError for an unknown pose."""
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
        """Leaf, plane row and signed distance to the pooled plane of its own leaf for every query point."""
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
        max_variance; origin None: the centre of the cube; leaves: the leaf table and the
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
        Afterwards the map is what a fresh OctreeManager would be after inserting every pose again with its surviving
        points as moved: no subdivision, every cached table dropped - subdivide, fit planes and adjust again - except that
        Neighbours.index still names rows of the clouds as they were first inserted.  Transactional: DomainError (a
        moved point is not finite or lies outside the cube) leaves the map exactly as it was.  One kernel over the
        stored points and one host wait (octl_forest_transform_poses).  ValueError for transforms that are not one
        valid transform per selected pose; KeyError for an unknown pose; NotImplementedError on the caller's own plug
        types."""
        if self._plug is not None:
            raise NotImplementedError(
                "transform_poses moves the points of the device-resident map: an OctreeManager on the caller's own plug "
                "types keeps its points in those types on the host, and there is no host path for them")
        sel = None if pose_numbers is None else [self._slots[p] for p in pose_numbers]
        self._forest.transform_poses(transforms, sel)

    def remove_poses(self, pose_numbers: List[int]) -> int:
        """Let go of poses: afterwards the map is the map as it was with those poses absent.  The subdivision stays,
        as after carve (leaves only a removed pose populated stay, empty; ray evidence stays valid); every remaining
        pose reads back the same bits from get_points, get_leaf_points, leaf_statistics and the counters, and its rows
        keep their Neighbours.index; a query over every pose answers what it answered over the remaining poses
        before.  The pose numbers are free again - insert_points with one of them adds a new pose - and the point
        store on the device shrinks to the remaining poses' rows, so a sliding window holds bounded memory.  A pending
        RANSAC mask is applied in the same compaction; every cached table is dropped.  Launches and host waits do
        not depend on the number of points (octl_forest_remove_poses).  Returns the number of stored points that
        left.  KeyError for an unknown pose; ValueError on the caller's own plug types."""
        if self._plug is not None:
            raise ValueError(
                "remove_poses removes points of the device-resident map: an OctreeManager on the caller's own plug "
                "types keeps its points in those types on the host, and there is no host path for them")
        slots = [self._slots[p] for p in pose_numbers]   # KeyError for an unknown pose, before anything changes
        gone = set(pose_numbers)
        new_slot, removed = self._forest.remove_slots(slots)
        self._slots = {p: int(new_slot[s]) for p, s in self._slots.items() if p not in gone}
        return removed

    def prune(self):
        """Collapse the subtrees below which no point of any pose is left into leaves (a PruneResult; Grid.prune
        describes it).  The root always stays: an empty manager becomes its bare root.  ValueError on the caller's
        own plug types."""
        if self._plug is not None:
            raise ValueError(
                "prune renumbers the scheme of the device-resident map: an OctreeManager on the caller's own plug "
                "types keeps its points in those types on the host, and there is no host path for them")
        return self._forest.prune()

    def _adjust_names(self, pose_numbers):
        """The selected pose numbers in ascending slot order: the order of the transforms and of every result row."""
        chosen = self._slots if pose_numbers is None else set(pose_numbers)
        return [p for p, _ in sorted(self._slots.items(), key=lambda kv: kv[1]) if p in chosen]

    def node_cubes(self):
        """(corner (N, 3), edge (N,)) of every node id that locate / leaf_planes can name."""
        nd = self._host_map().nodes if self._plug is not None else self._forest.nodes
        return nd["corner"].copy(), nd["edge"].copy()

    def get_points(self, pose_number: Optional[int] = None):
        if self._plug is not None:
            return self._plug.get_points(pose_number)
        f = self._forest
        if pose_number is None:
            parts = [self.get_points(p) for p in self._slots]
            return np.vstack(parts) if parts else np.empty((0, 3), dtype=float)
        if pose_number not in self._slots:
            return np.empty((0, 3), dtype=float)
        # octree.get_points(): DFS order of the leaves = storage order
        blk = f.blocks
        sel = np.nonzero(blk["slot"] == self._slots[pose_number])[0]
        return f.gather_blocks(sel)

    def n_points(self, pose_number: Optional[int] = None) -> int:
        if self._plug is not None:
            return self._plug.count("n_points", pose_number)
        if pose_number is None:
            return sum(self._forest.n_points(s) for s in self._slots.values())
        if pose_number in self._slots:
            return self._forest.n_points(self._slots[pose_number])
        return 0

    def n_leaves(self, pose_number: int) -> int:
        if self._plug is not None:
            return self._plug.count("n_leaves", pose_number)
        if pose_number in self._slots:
            return self._forest.n_leaves(self._slots[pose_number])
        return 0

    def n_nodes(self, pose_number: int) -> int:
        if self._plug is not None:
            return self._plug.count("n_nodes", pose_number)
        if pose_number in self._slots:
            self._forest.ensure_built()
            return 1 + 8 * int(self._forest.info.n_internal)
        return 0

    # octree_manager.py:173-180
    def apply_mask(self, mask, pose_number: int):
        if self._plug is not None:
            return self._plug.apply_mask(mask, pose_number)
        if pose_number in self._slots:
            _views.apply_mask_slot(self._forest, self._slots[pose_number], mask)
