"""
Single-pose octree over one cube (reference: octree/octree.py:14-295), device resident.

The tree is a flat scheme-node table + a leaf-ordered point permutation produced by HIP kernels
(octreelib_amd/csrc/build.hip); this class only maps the reference's methods onto it.
"""

from dataclasses import dataclass
from typing import Callable, Generic, List

import numpy as np

from octreelib_amd import _views
from octreelib_amd._engine import Forest
from octreelib_amd.criteria import try_count_threshold, try_planar_threshold
from octreelib_amd.internal import T, Voxel
from octreelib_amd.leaf_stats import LeafStatistics, leaf_statistics_np
from octreelib_amd.octree.octree_base import OctreeBase, OctreeConfigBase, OctreeNodeBase

__all__ = ["OctreeNode", "Octree", "OctreeConfig"]


@dataclass
class OctreeConfig(OctreeConfigBase):
    pass


class Octree(OctreeBase, Generic[T]):
    """Octree(octree_config, corner_min, edge_length) - points of a single pose."""

    def __init__(self, octree_config: OctreeConfigBase, corner_min, edge_length):
        Voxel.__init__(self, corner_min, edge_length)
        self._config = octree_config
        self._forest = Forest(1, np.asarray(corner_min, dtype=np.float64), float(edge_length))
        self._slot = None

    # -- construction -------------------------------------------------------------------
    def insert_points(self, points, *, transform=None, segment=None):
        """octree.py:235-239.  Points added to an already subdivided tree descend the existing
        structure (octree.py:67-98) without triggering new splits.  transform / segment (no reference counterpart):
        the cloud is stored under the transform(s), as Grid.insert_points describes."""
        if self._slot is None:
            self._slot = self._forest.add_pose(points, transform, segment)
        else:
            self._forest.extend_pose(self._slot, points, transform, segment)

    def subdivide(self, subdivision_criteria: List[Callable]):
        """octree.py:214-220 / 20-32.  A root that is already split holds no points itself, so
        a count criterion is false on it and the call changes nothing (upstream behaviour)."""
        rule = try_planar_threshold(subdivision_criteria)
        k = None if rule is not None else try_count_threshold(subdivision_criteria)
        f = self._forest
        if self._slot is None:
            self._slot = f.add_pose(np.empty((0, 3)))
        if f.has_scheme and f.nodes["first_child"][0] >= 0:
            # upstream evaluates the criteria on the (empty) point array of the split root
            if not any([c(np.empty((0, 3), dtype=float)) for c in subdivision_criteria]):
                return
        if rule is not None:
            f.subdivide_planar(rule)
        elif k is None:
            f.subdivide_callable(subdivision_criteria)
        else:
            f.subdivide(k)

    def subdivide_as(self, other_octree: "Octree"):
        """octree.py:222-227: split this octree wherever `other_octree` is split (the operation an
        OctreeManager applies to every pose).  The scheme is copied on the host, every point is
        placed on the device."""
        f = self._forest
        if self._slot is None:
            self._slot = f.add_pose(np.empty((0, 3)))
        f.adopt_scheme(other_octree._forest)

    # -- queries ------------------------------------------------------------------------
    def get_points(self):
        """octree.py:229-233: DFS order of the leaves = storage order."""
        if self._slot is None:
            return np.empty((0, 3), dtype=float)
        return self._forest.xyz.copy()

    def get_leaf_points(self, non_empty: bool = True) -> List[Voxel]:
        if self._slot is None:
            self._slot = self._forest.add_pose(np.empty((0, 3)))
        return _views.leaf_views(self._forest, self._slot, non_empty)

    def leaf_statistics(self) -> LeafStatistics:
        """Count, mean, covariance and its eigen-decomposition (least-squares plane) of every non-empty leaf: row i
        describes get_leaf_points()[i].  One device call."""
        if self._slot is None:
            return leaf_statistics_np([])
        self._forest.ensure_built()
        return self._forest.leaf_stats(self._forest.slot_blocks(self._slot))

    # -- queries: no reference counterpart (octreelib_amd/query.py holds the host definitions) ------------------
    def _query_ready(self):
        if self._slot is None:
            self._slot = self._forest.add_pose(np.empty((0, 3)))

    def locate(self, points) -> np.ndarray:
        """int32 node id of the leaf every query point falls into (LeafView.node), -1 outside the cube or for a
        point that is not finite.  Read-only, one kernel."""
        self._query_ready()
        return self._forest.locate(points)

    def nearest(self, points, k: int = 1, *, max_distance: float):
        """The k <= 8 stored points nearest to every query point within max_distance (a Neighbours whose pose column
        is 0; Grid.nearest describes it)."""
        self._query_ready()
        return self._forest.neighbours(points, k, max_distance, None, [0] * self._forest.n_slots)

    def raycast(self, origins, directions, max_range, *, min_range=0.0, surface: str = "cube", min_points=None,
                max_variance=None):
        """What every ray hits first between min_range and max_range: the first occupied leaf ("cube") or the first
        accepted leaf plane ("plane") - a RayHits; Grid.raycast describes it.  One cube has no cap on the range."""
        self._query_ready()
        return self._forest.raycast(origins, directions, max_range, min_range, None, surface, min_points, max_variance)

    def ray_evidence(self, origins, directions, ranges, margin, min_range=0.0, returned=None):
        """How many rays end in every leaf and how many only pass through it (a RayEvidence; Grid.ray_evidence
        describes it).  One cube has no cap on the range."""
        self._query_ready()
        return self._forest.ray_evidence(origins, directions, ranges, margin, min_range, returned)

    def carve(self, evidence, min_through: int = 2, max_hits: int = 0) -> int:
        """Empty every leaf that at least min_through rays passed through and at most max_hits ended in (Grid.carve
        describes it; evidence belongs to the scheme it was taken on).  Returns the number of points removed."""
        self._query_ready()
        return self._forest.carve(evidence, min_through, max_hits, None)

    def carve_rays(self, origins, directions, ranges, margin, min_range=0.0, returned=None, min_through: int = 2,
                   max_hits: int = 0) -> int:
        """carve(ray_evidence(...)) in one go on the device.  Returns the number of points removed."""
        self._query_ready()
        return self._forest.carve_rays(origins, directions, ranges, margin, min_range, returned, min_through,
                                       max_hits, None)

    def radius_count(self, points, radius, *, max_count=None) -> np.ndarray:
        """How many stored points lie within `radius` of every query point, capped at max_count ((n,) int32;
        Grid.radius_count describes it).  One cube has no cap on the radius."""
        self._query_ready()
        return self._forest.radius_count(points, radius, max_count, None)

    def remove_sparse(self, radius, min_neighbours) -> int:
        """Radius outlier removal: every point with fewer than min_neighbours other points within `radius` leaves
        the octree (Grid.remove_sparse describes it).  Returns the number of points removed."""
        self._query_ready()
        return self._forest.remove_sparse(radius, min_neighbours, None, None)

    def prune(self):
        """Collapse the subtrees below which no point is left into leaves (a PruneResult; Grid.prune describes it).
        The root always stays: an empty octree becomes its bare root."""
        self._query_ready()
        return self._forest.prune()

    def leaf_planes(self):
        """One least-squares plane per non-empty leaf, in ascending node id (a LeafPlanes)."""
        self._query_ready()
        return self._forest.leaf_planes(None)

    def plane_segments(self, min_points: int = 8, max_variance=None, max_angle: float = 0.1,
                       max_offset: float = 0.05):
        """The leaves of leaf_planes() merged across their faces into connected coplanar segments (a PlaneSegments;
        Grid.plane_segments describes it)."""
        self._query_ready()
        return self._forest.plane_segments(None, min_points, max_variance, max_angle, max_offset)

    def point_to_plane(self, points, min_points: int = 8, max_variance=None):
        """Leaf, plane row and signed distance to the plane of its own leaf for every query point."""
        self._query_ready()
        return self._forest.point_to_plane(points, None, min_points, max_variance)

    def registration_system(self, points, transform=None, min_points: int = 8, max_variance=None, max_distance=None,
                            huber_delta=None, origin=None, per_point: bool = False):
        """The point-to-plane normal equations of a scan under `transform` against the leaf planes (a
        RegistrationSystem; Grid.registration_system describes it)."""
        self._query_ready()
        return self._forest.registration_system(points, transform, origin, None, min_points, max_variance,
                                                max_distance, huber_delta, per_point)

    def align(self, points, initial=None, min_points: int = 8, max_variance=None, max_distance=None, huber_delta=None,
              max_iterations: int = 20, tolerance: float = 1e-9, damping: float = 0.0):
        """Gauss-Newton alignment of a scan to the leaf planes (an Alignment; Grid.align describes it)."""
        self._query_ready()
        return self._forest.align(points, initial, None, min_points, max_variance, max_distance, huber_delta,
                                  max_iterations, tolerance, damping)

    def point_registration_system(self, points, transform=None, *, max_distance: float, huber_delta=None, origin=None,
                                  per_point: bool = False):
        """The point-to-point normal equations of a scan under `transform` against the nearest stored points within
        max_distance (a RegistrationSystem; Grid.point_registration_system describes it).  One cube has no cap on
        max_distance."""
        self._query_ready()
        return self._forest.point_registration_system(points, transform, origin, None, max_distance, huber_delta,
                                                      per_point, [0] * self._forest.n_slots)

    def align_points(self, points, initial=None, *, max_distance: float, huber_delta=None, max_iterations: int = 20,
                     tolerance: float = 1e-9, damping: float = 0.0):
        """Gauss-Newton alignment of a scan to the nearest stored points (an Alignment; Grid.align_points describes
        it)."""
        self._query_ready()
        return self._forest.align_points(points, initial, None, max_distance, huber_delta, max_iterations, tolerance,
                                         damping)

    def node_cubes(self):
        """(corner (N, 3), edge (N,)) of every node id that locate / leaf_planes can name."""
        self._query_ready()
        nd = self._forest.nodes
        return nd["corner"].copy(), nd["edge"].copy()

    @property
    def n_points(self):
        return 0 if self._slot is None else self._forest.n_points(self._slot)

    @property
    def n_leaves(self):
        return 0 if self._slot is None else self._forest.n_leaves(self._slot)

    @property
    def n_nodes(self):
        if self._slot is None:
            return 1
        self._forest.ensure_built()
        return 1 + 8 * int(self._forest.info.n_internal)

    # -- callable driven ----------------------------------------------------------------
    def filter(self, filtering_criteria: List[Callable]):
        if self._slot is not None:
            _views.filter_slots(self._forest, [self._slot], filtering_criteria)

    def map_leaf_points(self, function: Callable):
        if self._slot is not None:
            _views.map_slots(self._forest, [self._slot], function)

    def apply_mask(self, mask):
        if self._slot is not None:
            _views.apply_mask_slot(self._forest, self._slot, mask)


class OctreeNode(OctreeNodeBase):
    """Stand-alone node (reference: OctreeNode(corner_min, edge_length, octree_cached_leaves),
    octree_base.py:36-49).  It owns a device octree rooted at itself; the caller's
    `octree_cached_leaves` list is refreshed with the current leaves (empty ones included) after
    every structural change, like the list the reference nodes append themselves to."""

    def __init__(self, corner_min, edge_length, octree_cached_leaves: list):
        Voxel.__init__(self, corner_min, edge_length)
        self._tree = Octree(OctreeConfig(), corner_min, edge_length)
        self._cached_leaves = octree_cached_leaves
        self._cached_leaves.append(self)

    def _refresh_cache(self):
        self._cached_leaves[:] = self._tree.get_leaf_points(non_empty=False)

    def insert_points(self, points):
        self._tree.insert_points(points)

    def subdivide(self, subdivision_criteria):
        self._tree.subdivide(subdivision_criteria)
        self._refresh_cache()

    def subdivide_as(self, other):
        """octree.py:34-53: `other` is a node (or an Octree) over the same cube."""
        self._tree.subdivide_as(other._tree if isinstance(other, OctreeNode) else other)
        self._refresh_cache()

    def get_points(self):
        return self._tree.get_points()

    def get_leaf_points(self):
        """octree.py:125-135: fresh Voxel copies of the non-empty leaves, DFS order."""
        leaves = self._tree.get_leaf_points()
        leaves.sort(key=lambda v: v._start)
        return [Voxel(v.corner_min, v.edge_length, v.get_points()) for v in leaves]

    def filter(self, filtering_criteria):
        self._tree.filter(filtering_criteria)
        self._refresh_cache()

    def map_leaf_points(self, function):
        self._tree.map_leaf_points(function)
        self._refresh_cache()

    def apply_mask(self, mask):
        self._tree.apply_mask(mask)
        self._refresh_cache()

    @property
    def n_points(self):
        return self._tree.n_points

    @property
    def n_leaves(self):
        return self._tree.n_leaves

    @property
    def n_nodes(self):
        return self._tree.n_nodes
