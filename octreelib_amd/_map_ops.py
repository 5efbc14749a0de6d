"""
The map operations that Grid and OctreeManager share (no reference counterpart): queries, registration, adjustment
and the edits that remove or move stored points.  Each is defined once here, over the device-resident forest
(_engine.Forest) or, on the caller's own plug types, over the host definitions (query.HostMap).

A new map operation goes into Forest (device path), HostMap (host definition) and, once, into MapOperations.

The inheriting class provides
  _forest, _plug, _slots   the forest or the plug (the other is None); pose number -> slot of the forest
  _host_map()              the HostMap of the plug: the two kinds of map build it differently
  _plug_poses()            the plug's table that is keyed by pose number
  _noun                    "a Grid" / "an OctreeManager", for the refusals on the caller's own plug types

The module-level map functions (matching.py, thinning.py, neighbourhood.py, clustering.py) take any of the three classes and start with _resolve below.

Octree is not served from here: its operations take no pose_numbers, so every signature differs, and each is already
two lines over Forest.
"""

from typing import List, Optional

import numpy as np

from octreelib_amd.adjustment import Adjustment, AdjustmentSystem
from octreelib_amd.query import LeafPlanes, Neighbours, PlaneSegments, PointToPlane, RayEvidence, RayHits
from octreelib_amd.registration import Alignment, RegistrationSystem

__all__ = ["MapOperations"]


def _resolve(map, pose_numbers, what):
    """What the module-level map functions (matching.py, thinning.py, neighbourhood.py, clustering.py) start with: (forest or None, HostMap or None,
    selection, pose numbers in slot order) of a Grid, an OctreeManager or an Octree; TypeError for anything else,
    ValueError for an Octree with pose_numbers, KeyError for an unknown pose."""
    from octreelib_amd.octree import Octree

    if isinstance(map, Octree):
        if pose_numbers is not None:
            raise ValueError(f"{what}: an Octree holds a single pose and takes no pose_numbers")
        map._query_ready()
        return map._forest, None, None, [0] * map._forest.n_slots
    if not isinstance(map, MapOperations):
        raise TypeError(f"{what}: expected a Grid, an OctreeManager or an Octree, got {type(map).__name__}")
    sel = map._query_slots(pose_numbers)
    if map._plug is not None:
        return None, map._host_map(), sel, None
    return map._forest, None, sel, map._adjust_names(None)


class MapOperations:
    def _query_slots(self, pose_numbers):
        if self._plug is not None:
            poses = self._plug_poses()
            for p in pose_numbers or ():
                poses[p]   # KeyError for an unknown pose
            return pose_numbers
        return None if pose_numbers is None else [self._slots[p] for p in pose_numbers]

    def _adjust_names(self, pose_numbers):
        """The selected pose numbers (None: all) in ascending slot order: the order of the transforms and of every
        result row."""
        chosen = self._slots if pose_numbers is None else set(pose_numbers)
        return [p for p, _ in sorted(self._slots.items(), key=lambda kv: kv[1]) if p in chosen]

    def locate(self, points) -> np.ndarray:
        """int32 node id of the scheme leaf that every query point falls into - the leaf a point inserted as a late
        pose would land in; LeafView.node of get_leaf_points is the id to match against - or -1: not finite, on a Grid
        no top-level voxel there or outside the voxel domain, on an OctreeManager outside the cube.  Read-only, one
        kernel.  Any (n, 3) array-like."""
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
        ValueError for k outside 1 .. 8, a max_distance that is not finite and positive or, on a Grid, above twice the
        voxel edge (one cube has no cap); RuntimeError after map_leaf_points moved rows outside their leaves; KeyError
        for an unknown pose."""
        sel = self._query_slots(pose_numbers)
        if self._plug is not None:
            return self._host_map().nearest(points, k, max_distance=max_distance, pose_numbers=sel)
        return self._forest.neighbours(points, k, max_distance, sel, self._adjust_names(None))

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
        (octreelib_amd/query.py: raycast_np is the definition, bit for bit).  ValueError for shapes that do not fit,
        an unknown surface or, on a Grid, a ray that spans more than 256 voxel edges (one cube has no cap on the
        range); RuntimeError after map_leaf_points moved rows outside their leaves; KeyError for an unknown pose."""
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
        count).  ValueError for shapes that do not fit, a bad margin or, on a Grid, a ray that spans more than 256
        voxel edges (one cube has no cap on the range)."""
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
                f"carve removes points of the device-resident map: {self._noun} on the caller's own plug types keeps "
                "its points in those types on the host, and there is no host path for them")
        return self._forest.carve(evidence, min_through, max_hits, self._query_slots(pose_numbers))

    def carve_rays(self, origins, directions, ranges, margin, min_range=0.0, returned=None, min_through: int = 2,
                   max_hits: int = 0, pose_numbers: Optional[List[int]] = None) -> int:
        """carve(ray_evidence(...)) in one go on the device: the counters are never downloaded.  Returns the number
        of points removed."""
        if self._plug is not None:
            raise NotImplementedError(
                f"carve_rays removes points of the device-resident map: {self._noun} on the caller's own plug types "
                "keeps its points in those types on the host, and there is no host path for them")
        return self._forest.carve_rays(origins, directions, ranges, margin, min_range, returned, min_through,
                                       max_hits, self._query_slots(pose_numbers))

    def radius_count(self, points, radius, *, max_count: Optional[int] = None,
                     pose_numbers: Optional[List[int]] = None) -> np.ndarray:
        """How many stored points of the given poses (None: all) lie within `radius` of every query point: (n,) int32,
        min(count, max_count) with max_count None: uncapped - density gates, occupancy tests for new scan points,
        adaptive radii.  The counted points are exactly the candidates of nearest (distance2 <= radius^2 inclusive;
        what a mask, a filter, carve or remove_poses took out never counts) without its limit of 8; a query that is
        not finite counts 0; a capped query stops searching at the cap.  points: any (n, 3) array-like, or a
        DeviceCloud of float64 points, read where it lies.  One kernel once the block index of the selection exists
        (octreelib_amd/query.py: radius_count_np is the definition, count for count).  ValueError for a radius that
        is not finite and positive or, on a Grid, above twice the voxel edge (one cube has no cap on the radius), or
        a max_count that is not an integer in 1 .. 2^31 - 1; RuntimeError after map_leaf_points moved rows outside
        their leaves; KeyError for an unknown pose."""
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
        removed.  ValueError for a radius that is not finite and positive or, on a Grid, above twice the voxel edge
        (one cube has no cap on the radius), or a min_neighbours that is not an integer in 1 .. 2^31 - 1; RuntimeError
        after map_leaf_points moved rows outside their leaves; KeyError for an unknown pose; NotImplementedError on
        the caller's own plug types."""
        if self._plug is not None:
            raise NotImplementedError(
                f"remove_sparse removes points of the device-resident map: {self._noun} on the caller's own plug "
                "types keeps its points in those types on the host (HostMap.remove_sparse gives the decision)")
        return self._forest.remove_sparse(radius, min_neighbours, self._query_slots(pose_numbers),
                                          self._query_slots(among))

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
        map has changed or the pose selection is another one."""
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
        definition).  ValueError for a max_distance that is not finite and positive or, as for nearest, above twice
        the voxel edge on a Grid; RuntimeError after map_leaf_points moved rows outside their leaves; KeyError for an
        unknown pose."""
        sel = self._query_slots(pose_numbers)
        if self._plug is not None:
            return self._host_map().point_registration_system(points, transform, max_distance=max_distance,
                                                              pose_numbers=sel, huber_delta=huber_delta,
                                                              origin=origin, per_point=per_point)
        return self._forest.point_registration_system(points, transform, origin, sel, max_distance, huber_delta,
                                                      per_point, self._adjust_names(None))

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
        max_variance; origin None: the centre of the box of the top-level voxels on a Grid, the centre of the cube on
        an OctreeManager; leaves: the leaf table and the block moments come back too.  The map is reduced to 80 bytes
        per (leaf, pose) block once; a call reads no point: three kernels and one host wait
        (octreelib_amd/adjustment.py has the definition)."""
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
        Afterwards the map is what a fresh Grid or OctreeManager would be after inserting every pose again with its
        surviving points as moved: no subdivision, on a Grid the top-level voxels the moved points fall into, every
        cached table dropped - subdivide, fit planes and adjust again - except that Neighbours.index still names rows
        of the clouds as they were first inserted.  Transactional: DomainError (a moved point is not finite or, on a
        Grid, falls outside the voxel domain, on an OctreeManager, lies outside the cube) leaves the map exactly as it
        was.  One kernel over the stored points and one host wait (octl_forest_transform_poses).  ValueError for
        transforms that are not one valid transform per selected pose; KeyError for an unknown pose;
        NotImplementedError on the caller's own plug types."""
        if self._plug is not None:
            raise NotImplementedError(
                f"transform_poses moves the points of the device-resident map: {self._noun} on the caller's own plug "
                "types keeps its points in those types on the host, and there is no host path for them")
        self._forest.transform_poses(transforms, self._query_slots(pose_numbers))

    def remove_poses(self, pose_numbers: List[int]) -> int:
        """Let go of poses: afterwards the map is the map as it was with those poses absent.  The subdivision and, on
        a Grid, the voxels and their creation order stay, as after carve (leaves and, on a Grid, voxels only a removed
        pose populated stay, empty; ray evidence stays valid); every remaining pose reads back the same bits from
        get_points, get_leaf_points, leaf_statistics and the counters, and its rows keep their Neighbours.index; a
        query over every pose answers what it answered over the remaining poses before.  The pose numbers are free
        again - insert_points with one of them adds a new pose, which inherits the subdivision as any late pose does -
        and the point store on the device shrinks to the remaining poses' rows, on a Grid with its voxel box folded
        again, so a sliding window holds bounded memory and, on a Grid, does not carry the box of everywhere it has
        been.  A pending RANSAC mask is applied in the same compaction; every cached table is dropped.  Launches and
        host waits do not depend on the number of points (octl_forest_remove_poses).  Returns the number of stored
        points that left.  KeyError for an unknown pose; ValueError on the caller's own plug types."""
        if self._plug is not None:
            raise ValueError(
                f"remove_poses removes points of the device-resident map: {self._noun} on the caller's own plug "
                "types keeps its points in those types on the host, and there is no host path for them")
        slots = [self._slots[p] for p in pose_numbers]   # KeyError for an unknown pose, before anything changes
        gone = set(pose_numbers)
        new_slot, removed = self._forest.remove_slots(slots)
        self._slots = {p: int(new_slot[s]) for p, s in self._slots.items() if p not in gone}
        return removed

    def prune(self):
        """Make the subdivision follow the points again, on the device: an internal node below which no point of any
        pose is left (after carve, filter, a RANSAC mask that was applied, remove_poses) becomes a leaf; an internal
        node that stays keeps all eight children, empty ones included.  On a Grid, top-level voxels that hold no point
        of any pose any more leave the map with their whole subtree; on an OctreeManager the root always stays: an
        empty manager becomes its bare root.  Nothing calls this implicitly.  Every read of every pose gives the same
        points, leaves and statistics as before, minus the empty leaves that are gone; points, their order and a
        pending RANSAC mask are not touched (prune after the mask is applied: what a pending mask will empty still
        counts as occupied).  Node ids change: the PruneResult returned maps them (node_map, old_node), and
        RayEvidence.remapped(result) carries evidence over.  On a Grid, a pose that no longer has a voxel it was
        inserted into no longer lists that voxel's (empty) leaves, and a later scan that falls into a dropped voxel
        creates it anew, as any voxel seen for the first time: an unsplit root at the END of the creation order,
        until the next subdivide.  Launches and host waits do not depend on the number of points, nodes or levels
        (octl_forest_prune).  ValueError on the caller's own plug types."""
        if self._plug is not None:
            raise ValueError(
                f"prune renumbers the scheme of the device-resident map: {self._noun} on the caller's own plug types "
                "keeps its points in those types on the host, and there is no host path for them")
        return self._forest.prune()

    def node_cubes(self):
        """(corner (N, 3), edge (N,)) of every node id that locate / leaf_planes can name."""
        nd = self._host_map().nodes if self._plug is not None else self._forest.nodes
        return nd["corner"].copy(), nd["edge"].copy()
