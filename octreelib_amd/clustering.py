"""
Euclidean cluster extraction (no reference counterpart): which stored points form one object - the connected components
of "two stored points are within `radius` of each other", what PCL's EuclideanClusterExtraction and Open3D's
cluster_dbscan give after ground and plane removal: the things that stand on the floor, dynamic objects to track or
drop, clumps of speckle to throw away.

  cluster(map, radius, min_points, max_points)     one label per alive stored point, the clusters' sizes and smallest
                                                   members;
  remove_small_clusters(map, radius, min_points)   every point of a component of fewer than min_points members leaves
                                                   the map - remove_sparse judges a point by its own neighbour count and
                                                   keeps a clump of five, each of whose points has four neighbours.

They are module-level functions over a Grid, an OctreeManager or an Octree - on the device-resident map a lock-free
union-find over the walk of radius_count (octl_forest_cluster_points, octl_forest_remove_small_clusters:
csrc/cluster.hip, csrc/cluster_link.h, csrc/union_find.h), on the caller's own plug types the host
definitions below through query.HostMap.  The answer consists of integers only: the device equals the definitions
exactly.  The definitions hash the points into cells instead of comparing every pair, so they check maps of 10^5 points.
"""

from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from octreelib_amd.query import _count_arg, check_radius_args

__all__ = ["Clusters", "cluster_labels_np", "small_cluster_keep_np", "check_cluster_args", "cluster",
           "remove_small_clusters"]

_PAIRS = 1 << 22      # candidate pairs examined at a time


@dataclass
class Clusters:
    """The clusters of n stored points; row i is the point `index[i]` of pose `pose[i]`, rows ascending in (insertion
    order of the pose, index): the total order of Neighbours.  Cluster c has sizes[c] members, the smallest of which in
    that order is the point first_index[c] of pose first_pose[c]; the clusters are numbered in ascending order of that
    member."""

    pose: np.ndarray          # (n,) int32 pose number
    index: np.ndarray         # (n,) int32 row of the point in that pose's cloud as inserted (Neighbours.index)
    label: np.ndarray         # (n,) int32 cluster of the point, -1: its component's size is outside [min_points, max_points]
    sizes: np.ndarray         # (n_clusters,) int64
    first_pose: np.ndarray    # (n_clusters,) int32
    first_index: np.ndarray   # (n_clusters,) int32

    def __len__(self):
        return len(self.sizes)

    def members(self, c: int) -> np.ndarray:
        """The rows of cluster c, ascending."""
        if not 0 <= int(c) < len(self.sizes):
            raise IndexError(f"cluster {c!r} of {len(self.sizes)}")
        return np.nonzero(self.label == int(c))[0]


def check_cluster_args(radius, min_points=1, max_points=None, what="cluster"):
    """(radius, min_points, max_points) as (float, int, int or None); ValueError for what cluster and
    remove_small_clusters refuse whatever the map: a radius that is not finite and positive (check_radius_args), a
    min_points or a given max_points that is not an integer in 1 .. 2^31 - 1, max_points < min_points (max_points None:
    no upper limit)."""
    r, _, _ = check_radius_args(radius, what=what)
    lo = _count_arg("min_points", min_points, what)
    hi = None if max_points is None else _count_arg("max_points", max_points, what)
    if hi is not None and hi < lo:
        raise ValueError(f"{what}: max_points = {hi} is below min_points = {lo}")
    return r, lo, hi


def _join(lab, ei, ej):
    """The labelling `lab` (lab[x] = the smallest member of x's component so far) after the edges (ei, ej): min-label
    propagation over the contracted edge list - every root takes the smallest root an edge joins it to - with pointer
    jumping until every label is a root again.  Only local minima among the roots survive a round, so the rounds are
    logarithmic in the number of components joined."""
    a, b = lab[ei], lab[ej]
    while True:
        differ = a != b
        if not differ.any():
            return lab
        a, b = a[differ], b[differ]
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        key = np.unique(hi * np.int64(len(lab)) + lo)        # (each joined pair of roots once)
        hi, lo = key // len(lab), key % len(lab)
        new = lab.copy()
        np.minimum.at(new, hi, lo)                            # (lab[x] <= x stays: the larger root goes under the smaller)
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        lab = new
        a, b = lab[a], lab[b]


def _cell_ranks(col):
    """Integer cell index of every entry of one axis, compressed: equal indices stay equal, indices one apart stay one
    apart, a gap of two or more becomes two - adjacency is kept and the range is at most twice the number of points."""
    u, inv = np.unique(col, return_inverse=True)
    step = np.minimum(np.diff(u), 2.0) if len(u) > 1 else np.empty(0)
    rank = np.concatenate([[0.0], np.cumsum(step)]).astype(np.int64)
    return rank[np.asarray(inv).reshape(-1)]


def _roots(P, r):
    """Smallest member of the connected component of every row of P (n, 3) under "d2 <= r2": (n,) int64."""
    n = len(P)
    lab = np.arange(n, dtype=np.int64)
    ok = np.nonzero(np.all(np.isfinite(P), axis=1))[0]       # (a row that is not finite is within r of nothing)
    if len(ok) < 2:
        return lab
    r2 = np.float64(r) * np.float64(r)
    X = P[ok]
    # cells a hair wider than the radius: fl(dx dx) <= fl(r r) does not exclude |dx| one ulp above r, and the quotient
    # is rounded too; with 2^-20 to spare two points within the radius are at most one cell apart on every axis
    with np.errstate(over="ignore", invalid="ignore"):
        cells = np.floor(X / (np.float64(r) * (1.0 + 2.0 ** -20)))
    held = np.all(np.isfinite(cells), axis=1)
    ok, X, cells = ok[held], X[held], cells[held]
    if len(ok) < 2:
        return lab
    c = np.stack([_cell_ranks(cells[:, a]) for a in range(3)], axis=1) + 1
    ext = c.max(axis=0) + 2
    key = (c[:, 0] * ext[1] + c[:, 1]) * ext[2] + c[:, 2]
    order = np.argsort(key, kind="stable")
    ukey, start, count = np.unique(key[order], return_index=True, return_counts=True)
    # every pair of cells at most one apart, each once: the cell itself and the 13 offsets that are positive in
    # lexicographic order
    offsets = [(dx, dy, dz) for dx in (0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) >= (0, 0, 0)]
    for dx, dy, dz in offsets:
        other = ukey + ((dx * ext[1] + dy) * ext[2] + dz)
        at = np.searchsorted(ukey, other)
        hit = (at < len(ukey)) & (ukey[np.minimum(at, len(ukey) - 1)] == other)
        A, B = np.nonzero(hit)[0], at[hit]
        pairs = count[A] * count[B]
        done = 0
        while done < len(A):
            # as many cell pairs as hold about _PAIRS point pairs (one at least)
            upto = done + max(1, int(np.searchsorted(np.cumsum(pairs[done:]), _PAIRS, side="right")))
            a, b, m = A[done:upto], B[done:upto], pairs[done:upto]
            done = upto
            which = np.repeat(np.arange(len(a)), m)
            local = np.arange(int(m.sum()), dtype=np.int64) - np.repeat(np.cumsum(m) - m, m)
            i = order[start[a][which] + local // count[b][which]]
            j = order[start[b][which] + local % count[b][which]]
            if (dx, dy, dz) == (0, 0, 0):
                once = i < j
                i, j = i[once], j[once]
            with np.errstate(over="ignore", invalid="ignore"):
                ex, ey, ez = X[i, 0] - X[j, 0], X[i, 1] - X[j, 1], X[i, 2] - X[j, 2]
                near = (ex * ex + ey * ey) + ez * ez <= r2
            lab = _join(lab, ok[i[near]], ok[j[near]])
    return lab


def _parts(clouds):
    return [np.asarray(c, dtype=np.float64).reshape(-1, 3) for _, c in clouds]


def _split(a, parts):
    return np.split(a, np.cumsum([len(p) for p in parts])[:-1]) if parts else []


def _number(first_key, size, lo, hi):
    """Cluster numbering from one (key of the smallest member, size of the component) pair per point: (label (n,)
    int32, keys of the clusters ascending, their sizes int64) - the components whose size lies in [lo, hi] (hi None: no
    upper limit) numbered 0, 1, ... in ascending order of the key, every other point -1."""
    first_key = np.asarray(first_key, dtype=np.int64)
    size = np.asarray(size, dtype=np.int64)
    inside = size >= lo if hi is None else (size >= lo) & (size <= hi)
    keys, at = np.unique(first_key[inside], return_index=True)
    label = np.full(len(first_key), -1, dtype=np.int32)
    label[inside] = np.searchsorted(keys, first_key[inside]).astype(np.int32)
    return label, keys, size[inside][at]


def cluster_labels_np(clouds, radius, min_points=1, max_points=None):
    """Euclidean clusters by their definition.  clouds: [(pose number, (m, 3) points)] in slot order, as radius_count_np
    takes them; the vertices are all their rows.  Two vertices are joined iff d2 <= r2 in radius_count_np's own
    expression - dx = q_x - p_x, d2 = (dx dx + dy dy) + dz dz in float64 with separate products and sums, r2 = radius *
    radius formed once, inclusive - which is symmetric bit for bit and so defines an undirected graph; a duplicate at
    the same coordinates is a neighbour, a point is trivially in its own cluster, a row that is not finite is joined
    to nothing.  The id of a point is (position of its pose in `clouds`, row): the total order of Neighbours.  A
    cluster is a connected component; the clusters whose size lies in [min_points, max_points] (None: no upper limit)
    are numbered 0, 1, ... in ascending order of their smallest id, every other point gets label -1.  Returns (labels:
    one int32 array per cloud, sizes (n_clusters,) int64, first (n_clusters, 2) int64 = position in clouds, row of the
    smallest member).  The points are hashed into cells of the radius and only the 27 cells round each are compared;
    the components are taken by min-label propagation with pointer jumping over the edge list."""
    r, lo, hi = check_cluster_args(radius, min_points, max_points, what="cluster")
    parts = _parts(clouds)
    P = np.concatenate(parts) if parts else np.empty((0, 3))
    root = _roots(P, r)
    size = np.bincount(root, minlength=len(P))[root] if len(P) else np.empty(0, dtype=np.int64)
    label, keys, sizes = _number(root, size, lo, hi)
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    where = np.searchsorted(off, keys, side="right") - 1
    first = np.stack([where, keys - off[where]], axis=1).astype(np.int64).reshape(-1, 2)
    return _split(label, parts), sizes, first


def small_cluster_keep_np(clouds, radius, min_points):
    """The rule of remove_small_clusters: one bool array per cloud of `clouds` ([(pose number, (m, 3) points)] in slot
    order), true iff the row's connected component (cluster_labels_np: the graph over all rows of `clouds`) has at
    least min_points members.  One simultaneous round, after which a second round removes nothing: what stays keeps
    its whole component."""
    r, lo, _ = check_cluster_args(radius, min_points, what="remove_small_clusters")
    parts = _parts(clouds)
    P = np.concatenate(parts) if parts else np.empty((0, 3))
    root = _roots(P, r)
    keep = np.bincount(root, minlength=len(P))[root] >= lo if len(P) else np.empty(0, dtype=bool)
    return _split(keep, parts)


def cluster(map, radius, *, min_points: int = 1, max_points: Optional[int] = None,
            pose_numbers: Optional[List[int]] = None) -> Clusters:
    """Euclidean cluster extraction over the stored points: a Clusters with one row per alive stored point of the given
    poses (None: all) in the order of Neighbours - pose, index, label - and per cluster its size and smallest member
    (sizes, first_pose, first_index; .members(c) the rows of cluster c).  map: a Grid, an OctreeManager or an Octree.
    Two points belong to one cluster iff a chain of stored points of the given poses joins them, each within `radius`
    of the next (distance2 <= radius^2 inclusive, the test of radius_count; a duplicate at the same coordinates is a
    neighbour).  The selected poses are the whole graph: points of other poses are neither labelled nor used as
    bridges.  The clusters whose size lies in [min_points, max_points] (None: no upper limit) are numbered 0, 1, ... in
    ascending order of their smallest member, every other point has label -1.  What a mask, a filter, carve,
    remove_sparse, thin or remove_poses took out has no row and connects nothing; points that a pending RANSAC mask is
    about to drop still have rows and still connect, as in remove_sparse - apply_mask first avoids it.  The map is only
    read and no cached table is dropped.  Four kernels once the block index of the selection exists and one host wait,
    whatever the number of points or clusters (cluster_labels_np is the definition; the answer equals it exactly and
    does not depend on the subdivision).  ValueError for a radius that is not finite and positive or, on a Grid, above
    twice the voxel edge (one cube has no cap on the radius), a min_points or max_points that is not an integer in
    1 .. 2^31 - 1, max_points < min_points and an Octree with pose_numbers; RuntimeError after map_leaf_points moved
    rows outside their leaves; KeyError for an unknown pose; TypeError for another kind of map."""
    from octreelib_amd._map_ops import _resolve

    forest, host, sel, names = _resolve(map, pose_numbers, "cluster")
    r, lo, hi = check_cluster_args(radius, min_points, max_points, what="cluster")
    if host is not None:
        return host.cluster(r, min_points=lo, max_points=hi, pose_numbers=sel)
    return forest.cluster_points(r, sel, lo, hi, names)


def remove_small_clusters(map, radius, min_points: int, *, pose_numbers: Optional[List[int]] = None) -> int:
    """Remove clumps: every stored point of the given poses (None: all) whose cluster - cluster(map, radius,
    pose_numbers=...), taken over the given poses - has fewer than min_points members leaves the map: rain, the halo
    carve leaves round a removed car, whatever remove_sparse keeps because its points have each other for neighbours.
    map: a Grid, an OctreeManager or an Octree.  Every decision is made on the map as it is before the call (one
    simultaneous round; what stays keeps its whole cluster, so a second call removes nothing); points a pending RANSAC
    mask is about to drop still connect and are judged, and that mask is applied in the same compaction.  The scheme
    stays (prune() afterwards drops what became empty), every cached table is dropped, Neighbours.index of the
    surviving rows is unchanged.  Four kernels and the compaction (small_cluster_keep_np is the rule).  Returns the
    number of points removed.  ValueError for a radius that cluster refuses, a min_points that is not an integer in
    1 .. 2^31 - 1 and an Octree with pose_numbers; RuntimeError after map_leaf_points moved rows outside their leaves;
    KeyError for an unknown pose; TypeError for another kind of map; NotImplementedError on the caller's own plug types
    (HostMap.remove_small_clusters gives the decision)."""
    from octreelib_amd._map_ops import MapOperations, _resolve

    if isinstance(map, MapOperations) and map._plug is not None:
        raise NotImplementedError(
            f"remove_small_clusters removes points of the device-resident map: {map._noun} on the caller's own plug "
            "types keeps its points in those types on the host (HostMap.remove_small_clusters gives the decision)")
    forest, _, sel, _ = _resolve(map, pose_numbers, "remove_small_clusters")
    r, lo, _ = check_cluster_args(radius, min_points, what="remove_small_clusters")
    return forest.remove_small_clusters(r, lo, sel)
