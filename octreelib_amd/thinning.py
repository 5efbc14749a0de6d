"""
Voxel-grid thinning (no reference counterpart): dropping stored points by redundancy - the first thing a LiDAR pipeline
does to its map.  A regular lattice of edge `cell` is laid over space (absolute: origin 0, nothing to do with the
subdivision) and only the first max_per_cell points that fall into each of its cells stay.

  cell_count(map, points, cell)    how many stored points lie in the lattice cell of every query point: the gate "only
                                   insert what is new" that a pipeline applies to a scan before insert_points;
  thin(map, cell, max_per_cell)    remove every stored point that has max_per_cell or more stored points of its cell
                                   before it in insertion order.

They are module-level functions over a Grid, an OctreeManager or an Octree - on the device-resident map one kernel each
(octl_forest_cell_count, octl_forest_thin: csrc/cell.hip, csrc/cell_walk.h), on the caller's own plug
types the host definitions below through query.HostMap.  The definitions hash the cell indices instead of comparing
every pair, so they check maps of 10^5 points.
"""

from typing import List, Optional

import numpy as np

from octreelib_amd.query import _as_queries, _count_arg

__all__ = ["cell_index_np", "cell_count_np", "thin_keep_np", "thin_ranks_np", "check_cell_args", "cell_count", "thin"]


def check_cell_args(cell, max_count=None, max_per_cell=None, what="cell_count"):
    """(cell, max_count, max_per_cell) as (float, int or None, int or None); ValueError for what cell_count and thin
    refuse whatever the map: a cell that is not finite and positive, a max_count or max_per_cell that is given and not
    an integer in 1 .. 2^31 - 1 (max_count None: uncapped)."""
    try:
        c = float(cell)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: cell must be finite and positive, got {cell!r}") from None
    if not (np.isfinite(c) and c > 0.0):
        raise ValueError(f"{what}: cell must be finite and positive, got {cell!r}")
    if max_count is not None:
        max_count = _count_arg("max_count", max_count, what)
    if max_per_cell is not None:
        max_per_cell = _count_arg("max_per_cell", max_per_cell, what)
    return c, max_count, max_per_cell


def _required(max_per_cell):
    if max_per_cell is None:
        raise ValueError("thin: max_per_cell = None is not an integer in 1 .. 2^31 - 1")
    return max_per_cell


def cell_index_np(points, cell) -> np.ndarray:
    """The lattice cell of every point: (n, 3) float64, np.floor_divide(p, cell) per axis - NumPy takes the floor of
    the TRUE quotient, and that is the definition.  The lattice is absolute (origin 0).  Two points share a cell iff
    the three indices are equal; a coordinate that is not finite has an index that equals none."""
    c, _, _ = check_cell_args(cell)
    p = _as_queries(points)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor_divide(p, c) + 0.0       # (+ 0.0: the index of -0.0 is 0.0 in the bits too)


def _labels(parts, cell):
    """One integer label per row of every array of `parts` - equal labels iff equal cell indices across all of them -
    and -1 for a row with a coordinate, or an index, that is not finite: it shares its cell with nothing."""
    sizes = [len(p) for p in parts]
    allp = np.concatenate(parts) if parts else np.empty((0, 3))
    label = np.full(len(allp), -1, dtype=np.int64)
    idx = cell_index_np(allp, cell)
    ok = np.all(np.isfinite(allp), axis=1) & np.all(np.isfinite(idx), axis=1)
    if ok.any():
        _, inverse = np.unique(idx[ok], axis=0, return_inverse=True)
        label[ok] = np.asarray(inverse).reshape(-1)
    return np.split(label, np.cumsum(sizes)[:-1]) if sizes else []


def cell_count_np(points, clouds, cell, *, max_count=None) -> np.ndarray:
    """How many stored points lie in the lattice cell of every query point: the definition of cell_count.  clouds:
    [(pose number, (m, 3) points)] of the counted poses, as radius_count_np takes them.  The answer, (n,) int32, is
    min(number of stored points whose cell index (cell_index_np) equals the query's, max_count); max_count None:
    uncapped.  A query with a coordinate that is not finite counts 0."""
    c, max_count, _ = check_cell_args(cell, max_count)
    q = _as_queries(points)
    parts = [np.asarray(x, dtype=np.float64).reshape(-1, 3) for _, x in clouds]
    stored = np.concatenate(parts) if parts else np.empty((0, 3))
    if len(q) == 0 or len(stored) == 0:
        return np.zeros(len(q), dtype=np.int32)
    lq, ls = _labels([q, stored], c)
    per_cell = np.bincount(ls[ls >= 0], minlength=int(max(lq.max(), ls.max(), 0)) + 1)
    count = np.where(lq >= 0, per_cell[np.maximum(lq, 0)], 0).astype(np.int64)
    if max_count is not None:
        count = np.minimum(count, max_count)
    return count.astype(np.int32)


def thin_ranks_np(clouds, tested, cell):
    """rank(x) of thin_keep_np for every judged point: a list of (m,) int64 arrays in the order of thin_keep_np's
    answer (an untested cloud's entry is None)."""
    c, _, _ = check_cell_args(cell, what="thin")
    names = [int(p) for p, _ in clouds]
    parts = [np.asarray(x, dtype=np.float64).reshape(-1, 3) for _, x in clouds]
    chosen, extra = (set(names), []) if tested is None else (set(), [])
    for t in (() if tested is None else tested):
        if isinstance(t, (int, np.integer)):
            if int(t) not in names:
                raise ValueError(f"thin: tested pose {t!r} is not among the counted clouds and brings no points")
            chosen.add(int(t))
        else:
            p, pts = t[0], t[1]
            before = len(clouds) if len(t) < 3 else int(t[2])
            if int(p) in names:
                raise ValueError(f"thin: tested pose {p!r} is among the counted clouds: name it by its number")
            if not 0 <= before <= len(clouds):
                raise ValueError(f"thin: tested pose {p!r} cannot come after {before} of {len(clouds)} counted clouds")
            extra.append((np.asarray(pts, dtype=np.float64).reshape(-1, 3), before))
    labels = _labels(parts + [x for x, _ in extra], c)
    off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
    M = int(off[-1])
    ls = np.concatenate(labels[:len(parts)]) if parts else np.empty(0, dtype=np.int64)
    gid = np.arange(M, dtype=np.int64)
    held = ls >= 0
    # the stored points as sorted keys (cell, id): the points of a cell before id g are those with a key in
    # [cell (M + 1), cell (M + 1) + g)
    keys = np.sort(ls[held] * (M + 1) + gid[held])

    def ranks(label, g):
        r = np.searchsorted(keys, label * (M + 1) + g) - np.searchsorted(keys, label * (M + 1))
        return np.where(label >= 0, r, 0).astype(np.int64)

    out = [ranks(labels[i], off[i] + np.arange(len(parts[i]), dtype=np.int64)) if names[i] in chosen else None
           for i in range(len(parts))]
    for j, (x, before) in enumerate(extra):
        out.append(ranks(labels[len(parts) + j], np.full(len(x), off[before], dtype=np.int64)))
    return out


def thin_keep_np(clouds, tested, cell, max_per_cell=1):
    """The rule of thin (voxel-grid downsampling): which stored points stay.  clouds: [(pose number, (m, 3) points)] of
    the COUNTED poses in ascending slot order; tested: the poses whose points are judged - pose numbers among `clouds`
    (None: all of them) and, for a tested pose that is not counted, a (pose number, points) pair - it comes after
    every counted cloud, as a new scan does - or a (pose number, points, before) triple for one that comes after the
    first `before` counted clouds.  The id of a stored point is (position of its pose in slot order, row in the cloud as
    inserted): the total order of Neighbours.  For a point x of a tested pose, rank(x) = the number of points y of the
    counted clouds with cell(y) == cell(x) (cell_index_np) and id(y) < id(x) - strict, so x never counts itself, while
    a duplicate at the same coordinates with a smaller id does; a tested pose that is not counted is judged against the
    counted ones only.  keep(x) iff rank(x) < max_per_cell; a point with a coordinate that is not finite shares no
    cell and stays.  Every decision is made on the clouds as given: one simultaneous round.  With every cloud tested
    and counted it keeps exactly the first max_per_cell points of every cell in insertion order, and is then idempotent:
    a second round removes nothing.  Answer: one bool array per cloud in the order of `clouds` (all True for a cloud
    that is not tested), then one per pair or triple in the order given."""
    _, _, m = check_cell_args(cell, None, _required(max_per_cell), what="thin")
    rs = thin_ranks_np(clouds, tested, cell)
    sizes = [len(np.asarray(c).reshape(-1, 3)) for _, c in clouds]
    return [np.ones(sizes[i], dtype=bool) if r is None else r < m for i, r in enumerate(rs)]


def cell_count(map, points, cell, *, max_count: Optional[int] = None,
               pose_numbers: Optional[List[int]] = None) -> np.ndarray:
    """How many stored points of the given poses (None: all) lie in the lattice cell of every query point: (n,) int32,
    min(count, max_count) with max_count None: uncapped.  map: a Grid, an OctreeManager or an Octree.  The cell of a
    point is floor(p / cell) per axis on an absolute lattice (cell_index_np); what a mask, a filter, carve,
    remove_sparse, thin or remove_poses took out never counts; a query that is not finite counts 0; a capped query
    stops searching at the cap - cell_count(scan, cell, max_count=1) == 0 is "this scan point is new to the map".
    points: any (n, 3) array-like, or a DeviceCloud of float64 points, read where it lies.  One kernel once the block
    index of the selection exists (cell_count_np is the definition, count for count).  ValueError for a cell that is
    not finite and positive, on a Grid above the voxel edge L or below L 2^-20, on one cube below 2^-50 of
    max(|corner|, |corner + edge|) (every cell index of the map stays an exact double), for a max_count that is not an
    integer in 1 .. 2^31 - 1 and for an Octree with pose_numbers; RuntimeError after map_leaf_points moved rows outside
    their leaves; KeyError for an unknown pose; TypeError for another kind of map."""
    from octreelib_amd._map_ops import _resolve

    forest, host, sel, _ = _resolve(map, pose_numbers, "cell_count")
    if host is not None:
        return host.cell_count(points, cell, max_count=max_count, pose_numbers=sel)
    return forest.cell_count(points, cell, max_count, sel)


def thin(map, cell, max_per_cell: int = 1, *, pose_numbers: Optional[List[int]] = None,
         among: Optional[List[int]] = None) -> int:
    """Voxel-grid downsampling of the stored points: of the points that share a lattice cell of edge `cell`
    (cell_index_np) only the first max_per_cell stay, first in the order of Neighbours - the poses in the order they
    were inserted, the rows of a pose in the order of its cloud.  map: a Grid, an OctreeManager or an Octree.
    pose_numbers names the poses that may lose points (None: all), `among` the poses whose points occupy cells (None:
    all): pose_numbers=[newest] thins a new scan against the whole map.  A point never counts itself, an earlier
    duplicate at the same coordinates does; a tested pose that is not among the counted ones is judged against those
    only.  Every decision is made on the map as it is before the call (one simultaneous round); with the defaults a
    second call removes nothing.  Points that a pending RANSAC mask is about to drop still occupy cells and are judged,
    and that mask is applied in the same compaction - apply_mask first avoids it.  The scheme stays (prune() afterwards
    drops what became empty), every cached table is dropped, Neighbours.index of the surviving points is unchanged.
    One kernel and the compaction (thin_keep_np is the rule).  Returns the number of points removed.  ValueError for
    a cell that cell_count refuses, a max_per_cell that is not an integer in 1 .. 2^31 - 1 and an Octree with
    pose_numbers or among; RuntimeError after map_leaf_points moved rows outside their leaves; KeyError for an unknown
    pose; TypeError for another kind of map; NotImplementedError on the caller's own plug types (HostMap.thin gives
    the decision)."""
    from octreelib_amd._map_ops import MapOperations, _resolve

    if isinstance(map, MapOperations) and map._plug is not None:
        raise NotImplementedError(
            f"thin removes points of the device-resident map: {map._noun} on the caller's own plug types keeps its "
            "points in those types on the host (HostMap.thin gives the decision)")
    forest, _, sel, _ = _resolve(map, pose_numbers, "thin")
    asel = None
    if isinstance(map, MapOperations):
        asel = map._query_slots(among)
    elif among is not None:
        raise ValueError("thin: an Octree holds a single pose and takes no among")
    return forest.thin(cell, max_per_cell, sel, asel)
