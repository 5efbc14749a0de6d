"""
Seeded random operation sequences over the whole API, drawn with the oracle in the loop (no GPU needed).

generate(seed) returns a Sequence: the LOG - a list of plain dicts that fully determines the sequence (clouds by
generator parameters, RANSAC tables by their np.random.seed, criteria by their parameters, map functions by name) -
and, per step, the oracle-side expected observation (per pose: leaf table in list order with an order-independent
64-bit digest of every leaf's rows, and the counters) plus what the model knows about the library's own state (is
the pooled plane table of the device still valid, what split_stats must show).  Model.replay(container, log) builds a
fresh model from a log; this is how a model is forked (the oracle's trees cannot be deep-copied).

The container, the first subdivision kind and one "motif" (a transition that must occur with nothing mutating in
between) are fixed by the seed's number so that the seed set covers them; everything else is drawn.

Domain guard (INTEGRATION.md "Limits of the parity domain").  Preconditions that follow from the
container and the state alone decide which kinds can be drawn at all (an Octree has no poses, RANSAC needs pose
numbers 0..n-1, nothing re-keys points after rows were displaced, ...).  A drawn operation is then applied to the
model and REJECTED - the model is rebuilt by replaying the log, the draw is counted - when
  * a re-subdivide is not equal-or-finer (an internal node of the old scheme is a leaf of the new one),
  * a NotPlanar rule evaluated a node within 1e-9 e^2 of its threshold (tests/_util._oracle_nodes),
  * points are no longer distinct within a pose or across the poses that drive a scheme,
  * an in-place transforming map moved a row out of its leaf's cube.
An opaque filter that empties nothing stays in: the library evaluates it on the host and then makes no device call, so
the pooled plane table stays valid, which the model books (a point-count filter always runs on the device and always
invalidates it).
K of a count-driven re-subdivide is drawn below the smallest count the scheme poses have in any internal node of the
current scheme, which makes it equal-or-finer by construction.
The second generation (SEEDS2, _Generator2) adds the map queries - nearest, raycast, plane_segments,
registration_system, adjustment_system - and transform_poses with its refused form; SEEDS keep the logs they had.
Every parameter is still in the record: rigid motions as {"xi", "origin"} (motion()), queries, rays and scans by seed.
transform_poses rebuilds the model as a fresh one with every pose's surviving rows inserted again in store order, so
the model carries, per row, its number in the cloud as first inserted (Model.identity(): what Neighbours.index names);
a motion that takes a row out of the cube or the voxel domain is Rejected - or, for the refused form, required.
Not drawn at all: map functions that reorder a leaf's own rows (the library keeps insertion order for a selection
of a leaf's rows, the reference the returned order - visible to a later RANSAC), a displacing map anywhere but as
the last mutating operation.
The third generation (SEEDS3, _Generator3) adds what changes the store itself: insert_moved / extend_moved (a cloud
stored under one rigid transform or, piecewise, under one of M per row; the model receives transform_rows_np of the
cloud as given and keeps numbering its rows as given), carve (rays from evidence_rays(); the model forms the counters
with ray_evidence_np over its own scheme leaves and applies carve_keep_np as one oracle apply_mask per pose),
remove_poses with its refused form (the oracle trees of the poses go, the scheme trees and the voxels stay, the
numbers are free again), and the read-only ray_evidence and store_size.  SEEDS and SEEDS2 keep the logs they had.
The fourth generation (SEEDS4, _Generator4) adds the scheme pruned and the radius searches: prune (the model prunes
its own oracle trees by the definition of DESIGN 4.18 - a grid's voxel without a point of any pose leaves the map, the
topmost internal nodes without one become leaves in the scheme tree and in every pose tree - books the five numbers
of the PruneResult, keeps the pooled table valid exactly when nothing was dropped, and carries stored evidence over by
the rule of RayEvidence.remapped: a carve record with "remapped" takes it), remove_sparse (sparse_keep_np on the
model's rows, tile by tile, applied as one oracle apply_mask per judged pose; the rows that left are booked), and
the read-only radius_count (counted by the model itself with radius_count_np: the count has no order),
point_registration_system and nearest_plane_registration_system (scans of jittered stored rows under a motion from the
identity to right out of the scene; n_used and n_located are booked).  An insert or extend that puts a row into a
node a prune has collapsed is Rejected - nothing defines where such a node stands in a pose's leaf list once it is
filled again - until a transform_poses has rebuilt the map; an insert into a voxel a prune has dropped is in the
domain: the voxel is created anew at the end of the creation order.  SEEDS, SEEDS2 and SEEDS3 keep the logs they had.
"""

import collections
import functools

import numpy as np

from octreelib_amd.criteria import MaxPoints, NotPlanar
from oracle import octree_np as onp
from oracle import ransac_np as rnp
from tests._util import _longdouble_lambda, _oracle_nodes, _scheme_nodes
from tests.test_gpu_fuzz import _cloud

SEEDS = list(range(24))
UTM = np.array([5.0e6, 4.0e5, 100.0])
MANAGER_POSES = [7, 2, 5, 0, 9, 4]
MUTATING = ("insert", "extend", "subdivide_count", "subdivide_planar_count", "subdivide_planar", "subdivide_callable",
            "filter_count", "filter_opaque", "filter_subset", "map_select", "map_transform", "apply_mask", "ransac")
READ_ONLY = ("leaf_statistics", "locate", "leaf_planes", "point_to_plane", "node_cubes", "get_leaf_points",
             "counters", "split_stats")
# the second generation of the generator (SEEDS2) draws these too; the first one never does, so its logs stay as they are
NEW_MUTATING = ("transform_poses", "transform_poses_refused")
NEW_READ_ONLY = ("nearest", "raycast", "plane_segments", "registration_system", "adjustment_system")
# the third generation (SEEDS3): what changes the store itself, and the two reads that go with it
GEN3_MUTATING = ("insert_moved", "extend_moved", "carve", "remove_poses", "remove_poses_refused")
GEN3_READ_ONLY = ("ray_evidence", "store_size")
REFUSED = ("transform_poses_refused", "remove_poses_refused")      # raise in the library: nothing changes, nothing is invalidated
# the fourth generation (SEEDS4): the radius neighbour counts, the scheme pruned, the two nearest-point registrations
GEN4_MUTATING = ("remove_sparse", "prune")
GEN4_READ_ONLY = ("radius_count", "point_registration_system", "nearest_plane_registration_system")
GEN3_ALL_READ_ONLY = READ_ONLY + NEW_READ_ONLY + GEN3_READ_ONLY      # (what the third generation draws its reads from)
ALL_MUTATING = MUTATING + NEW_MUTATING + GEN3_MUTATING + GEN4_MUTATING
ALL_READ_ONLY = GEN3_ALL_READ_ONLY + GEN4_READ_ONLY
SUBDIVIDES = ("subdivide_count", "subdivide_planar_count", "subdivide_planar", "subdivide_callable")
FILTERS = ("filter_count", "filter_opaque", "filter_subset")
TRANSITIONS = ("ransac>leaf_planes", "ransac>subdivide", "ransac>insert", "filter>insert", "filter>point_to_plane",
               "map_transform>subdivide", "map_select>ransac", "leaf_planes(S)>insert>point_to_plane(S)",
               "planar>count>split_stats", "extend>leaf_statistics", "point_to_plane>ransac>point_to_plane",
               "two_ransac")
SEEDS2 = list(range(100, 124))      # container, first subdivision and motif by (seed - 100) as SEEDS has them by seed
TRANSITIONS2 = ("transform_poses>subdivide>nearest", "transform_poses>subdivide>ransac>apply_mask", "apply_mask>raycast",
                "leaf_planes(S)>raycast_plane(S')>point_to_plane(S)", "nearest(S)>raycast_cube(S')>nearest(S)",
                "plane_segments>filter>plane_segments", "adjustment_system>transform_poses>subdivide>adjustment_system",
                "transform_poses_refused>point_to_plane", "map_transform(shift_z)>nearest")
SEEDS3 = list(range(200, 224))      # container, first subdivision and motif by (seed - 200)
TRANSITIONS3 = ("carve>remove_poses(carved pose)", "ransac>carve", "carve>plane_segments",
                "carve>transform_poses>subdivide>adjustment_system", "ray_evidence>remove_poses>carve(evidence_from)",
                "ray_evidence>insert_moved>carve(evidence_from)", "leaf_planes(S)>remove_poses(not in S)>point_to_plane(S)",
                "nearest>remove_poses>nearest", "remove_poses>insert(freed number)>ransac",
                "remove_poses(scheme-driving subset)>subdivide_planar_count>split_stats", "remove_poses>remove_poses",
                "insert_moved(late, piecewise)>nearest", "extend_moved>leaf_statistics",
                "adjustment_system>remove_poses>adjustment_system")
SEEDS4 = list(range(300, 324))      # container, first subdivision and motifs by (seed - 300)
TRANSITIONS4 = ("leaf_planes(S)>prune(changes)>point_to_plane(S)", "leaf_planes(S)>prune(no-op)>point_to_plane(S)",
                "plane_segments>prune>plane_segments", "nearest>prune>nearest",
                "adjustment_system>prune(drops an outermost voxel)>adjustment_system(origin None)",
                "subdivide_planar>prune>split_stats", "ray_evidence>prune>carve(evidence_from, remapped)",
                "prune(drops a voxel)>insert(into it)>subdivide>ransac", "remove_poses>prune>insert(freed number)",
                "carve>prune>transform_poses>subdivide", "prune>prune", "radius_count(S)>remove_sparse>radius_count(S)",
                "remove_sparse>nearest", "remove_sparse(pose subset, among subset)>prune",
                "plane_segments>remove_sparse>plane_segments", "adjustment_system>remove_sparse>adjustment_system",
                "nearest(S)>point_registration_system(S')>nearest(S)",
                "leaf_planes(S)>nearest_plane_registration_system(S')>point_to_plane(S)",
                "nearest_plane_registration_system>remove_sparse>nearest_plane_registration_system",
                "point_registration_system>prune>point_registration_system")
# container and motif (index into TRANSITIONS) by seed % 12; the second entry is for seeds >= 12
_CONTAINER = {0: "grid", 1: "grid", 2: "grid", 3: "manager", 4: ("octree", "octree"), 5: ("octree", "grid"), 6: "grid",
              7: "manager", 8: ("grid", "manager"), 9: ("manager", "octree"), 10: "grid", 11: "grid"}
_MOTIF = {0: ["ransac", "leaf_planes"], 1: ["ransac", "subdivide_count"], 2: ["ransac", "insert"],
          3: ["filter_count", "insert"], 4: ["filter_opaque", "point_to_plane"],
          5: ["map_transform", "subdivide_count"], 6: ["map_select", "ransac"],
          7: ["leaf_planes", "insert", "point_to_plane"],
          8: ["subdivide_planar_count", "subdivide_count", "split_stats"], 9: ["extend", "leaf_statistics"],
          10: ["point_to_plane", "ransac", "point_to_plane"], 11: ["ransac", "get_leaf_points", "ransac"]}


def cloud_edge(container):
    """The length the clouds of a container are scaled by: they span [-2, 2) of it."""
    return container["edge"] if container["kind"] == "grid" else container["edge"] / 4.0


class Rejected(Exception):
    """The drawn operation leaves the parity domain."""


# ---- clouds, criteria, functions: everything a log record names ---------------------------------------------------
def make_cloud(c):
    """The cloud of a record {"seed", "n", "edge", "utm", "form"} in the form the library is given; the model
    receives model_cloud() of it.  The forms "device32" / "device64" (the third generation) are the f32 / f64 array
    here: the replay hands the library a feed.DeviceCloud made from it."""
    rng = np.random.default_rng([c["seed"], 0xC10D])
    pts = _cloud(rng, c["n"], c["edge"], planar=True)
    if c.get("cube"):    # one cube with a negative corner: p - corner must not round up to the cube's edge
        pts = np.minimum(pts, 2.0 * c["edge"] * (1.0 - 2.0 ** -20))
    if c["utm"]:
        pts = np.unique(pts + UTM, axis=0)
        rng.shuffle(pts)
    if c["form"] in ("f32", "device32"):
        hi = np.float32(2.0 * c["edge"] * (1.0 - 2.0 ** -20))
        p32 = np.minimum(pts.astype(np.float32), hi)
        _, first = np.unique(p32, axis=0, return_index=True)
        return np.ascontiguousarray(p32[np.sort(first)])
    if c["form"] == "fortran":
        return np.asfortranarray(pts)
    if c["form"] == "strided":
        big = np.zeros((2 * len(pts), 4))
        big[::2, :3] = pts
        return big[::2, :3]
    return pts


def model_cloud(c):
    return np.ascontiguousarray(make_cloud(c), dtype=np.float64)


def _spread(points):
    return float((points.max(axis=0) - points.min(axis=0)).max()) if len(points) else 0.0


def build_criteria(spec):
    """Subdivision criteria of a record: [["MaxPoints", K] | ["NotPlanar", mv, min_points, ddof] |
    ["big_and_wide", n, w]] (the last one is opaque to the library's recogniser: the host level loop)."""
    out = []
    for s in spec:
        if s[0] == "MaxPoints":
            out.append(MaxPoints(s[1]))
        elif s[0] == "NotPlanar":
            out.append(NotPlanar(s[1], s[2], s[3]))
        else:
            out.append((lambda n, w: (lambda points: len(points) > n and _spread(points) > w))(s[1], s[2]))
    return out


def build_filter(spec):
    """Filter criteria: ["ge", c] / ["lt", c] / ["between", lo, hi] are point-count comparisons the library
    recognises; ["spread_lt", w] is opaque."""
    if spec[0] == "ge":
        c = spec[1]
        return [lambda pts: len(pts) >= c]
    if spec[0] == "lt":
        c = spec[1]
        return [lambda pts: len(pts) < c]
    if spec[0] == "between":
        lo, hi = spec[1], spec[2]
        return [lambda pts: len(pts) >= lo, lambda pts: hi >= len(pts)]
    w = spec[1]
    return [lambda pts: _spread(pts) < w]


def build_map(name, edge):
    if name == "every_other":
        return lambda pts: pts[::2]
    if name == "first_half":
        return lambda pts: pts[: (len(pts) + 1) // 2]
    if name == "upper_z":
        return lambda pts: pts[pts[:, 2] >= np.median(pts[:, 2])]
    if name == "toward_mean":       # stays inside the leaf's cube (checked on the model)
        return lambda pts: pts + 0.25 * (pts.mean(axis=0) - pts)
    if name == "shift_z":           # rows leave their cubes: only as the last mutating operation
        return lambda pts: pts + np.array([0.0, 0.0, 0.4 * edge]) if len(pts) % 2 else pts
    raise KeyError(name)


def _mix(x):
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def leaf_digests(rows, sizes):
    """Per leaf (n, sum, xor) of a 64-bit hash of every row's bits (-0.0 folded into +0.0): equal exactly when the
    leaves hold the same multisets of rows (up to a 2^-64 collision), whatever the order inside a leaf."""
    sizes = np.asarray(sizes, dtype=np.int64)
    if len(sizes) == 0:
        return []
    u = (np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 3) + 0.0).view(np.uint64)
    with np.errstate(over="ignore"):
        h = _mix(u[:, 0] + np.uint64(0x9E3779B97F4A7C15))
        h = _mix(h ^ u[:, 1])
        h = _mix(h ^ u[:, 2])
        starts = np.concatenate(([0], np.cumsum(sizes)[:-1]))
        s = np.add.reduceat(h, starts)
    x = np.bitwise_xor.reduceat(h, starts)
    return [(int(n), int(a), int(b)) for n, a, b in zip(sizes.tolist(), s.tolist(), x.tolist())]


def row_hashes(rows):
    """The 64-bit hash of every row's bits that leaf_digests sums (-0.0 folded into +0.0)."""
    u = (np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 3) + 0.0).view(np.uint64)
    with np.errstate(over="ignore"):
        h = _mix(u[:, 0] + np.uint64(0x9E3779B97F4A7C15))
        h = _mix(h ^ u[:, 1])
        return _mix(h ^ u[:, 2])


def motion(m):
    """The 4x4 rigid transform of a record {"xi": (w, v), "origin": c}: Rot(w)(p - c) + c + v."""
    from octreelib_amd.registration import se3_exp

    return se3_exp(m["xi"], m["origin"])


def inverse_motion(m):
    T = motion(m)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


MOVED = ("insert_moved", "extend_moved")


def moved_args(op, n):
    """(transform, segment) of an insert_moved / extend_moved record for a cloud of n rows, as the library is given
    them: one 4x4 or 3x4 ("motion"), or a stack of M with one index per row ("motions", "segment_seed",
    "segment_dtype"); an even segment_seed gives ascending indices, as the firing columns of a sweep have them."""
    cut = (lambda T: np.ascontiguousarray(T[..., :3, :])) if op["matrix"] == "3x4" else (lambda T: T)
    if "motion" in op:
        return cut(motion(op["motion"])), None
    T = np.stack([motion(m) for m in op["motions"]])
    seg = np.random.default_rng([op["segment_seed"], 0x5E6]).integers(0, len(T), n)
    if op["segment_seed"] % 2 == 0:
        seg = np.sort(seg)
    return cut(T), seg.astype(op["segment_dtype"])


def model_rows(op):
    """What the model receives for an insert / extend record: the cloud as f64 - for the moved kinds through
    transform_rows_np, the exported definition of what the library stores."""
    from octreelib_amd.registration import transform_rows_np

    pts = model_cloud(op["cloud"])
    if op["op"] not in MOVED:
        return pts
    T, seg = moved_args(op, len(pts))
    return transform_rows_np(T, pts, seg)


def stored_rows(rows):
    """The rows a map stores, in an order that belongs to no build history: lexicographic, without repeats (one
    zero row when there is none).  What evidence_rays() aims at, on the model and on the device."""
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 3)
    return np.unique(rows, axis=0) if len(rows) else np.zeros((1, 3))


def evidence_rays(rec, stored, edge):
    """(origins, directions, ranges, returned) of a ray_evidence / carve record {"seed", "n", "margin", "min_range",
    "returned"}: one sensor per record, at a stored point pushed by up to half a cloud edge; every ray aims at a
    stored point with a jitter of 0.01 edge and measures the distance to it times 0.6, 1 or 1.5 (it ends in front of
    the point, at it, or has passed through its leaf).  Nine rays are dead or empty: three zero directions, a NaN in
    an origin, a direction and a range, three ranges below min_range.  "returned" is None or the share of rays
    without an echo: the flags are then a bool array drawn from the same seed."""
    rng = np.random.default_rng([rec["seed"], 0xE71D])
    n = rec["n"]
    sensor = stored[rng.integers(0, len(stored))] + rng.uniform(-0.5, 0.5, 3) * edge
    D = stored[rng.integers(0, len(stored), n)] + rng.normal(0.0, 0.01 * edge, (n, 3)) - sensor
    ranges = np.sqrt((D * D).sum(axis=1)) * rng.choice([0.6, 1.0, 1.5], n)
    O = np.tile(sensor, (n, 1))
    D[-9:-6] = 0.0
    O[-6, 1], D[-5, 0], ranges[-4] = np.nan, np.nan, np.nan
    ranges[-3:] = rec["min_range"] - 0.5 * edge
    returned = None if rec.get("returned") is None else rng.random(n) >= rec["returned"]
    return np.ascontiguousarray(O), np.ascontiguousarray(D), ranges, returned


def count_queries(rec, stored, edge):
    """The queries of a radius_count record {"seed", "n"}: the recipe of the replay's Device.queries - stored points
    jittered by 0.01 edge, a tenth of them pushed out of the scene, and the BAD rows - drawn from stored_rows(), which
    belongs to no build history, so that the model can count for the same queries."""
    from tests.test_gpu_query import BAD as BAD_QUERIES

    rng = np.random.default_rng([rec["seed"], 0x9E21])
    n = rec["n"]
    Q = stored[rng.integers(0, len(stored), n)] + rng.normal(0.0, 0.01 * edge, (n, 3))
    Q[: n // 10] += rng.uniform(-3.0, 3.0, (n // 10, 3)) * edge
    return np.concatenate([Q, BAD_QUERIES])


def scan_of(rec, stored, edge):
    """(scan, transform) of a point_registration_system / nearest_plane_registration_system record {"seed", "n",
    "motion"}: n stored points (stored_rows()) with a jitter of 0.002 edge - the scan as given - and the record's
    motion as the transform the call is made under."""
    rng = np.random.default_rng([rec["seed"], 0x5CA4])
    scan = stored[rng.integers(0, len(stored), rec["n"])] + rng.normal(0.0, 0.002 * edge, (rec["n"], 3))
    return np.ascontiguousarray(scan), motion(rec["motion"])


def sparse_keep_tiled(rows, tested, among, radius, min_neighbours):
    """{pose: keep} of remove_sparse for the tested poses, by sparse_keep_np - evaluated tile by tile, because the
    brute force over 45 000 x 45 000 pairs takes minutes.  rows: {pose: (m, 3)}; tested, among: pose numbers in slot
    order.  The judged rows of a pose are grouped by a lattice of cells of w >= radius; a tile is judged by
    sparse_keep_np against the counted rows inside the cell's box grown by radius (1 + 1e-6) on every side, which
    holds every row that can count for it (d2 <= fl(r r) bounds every |dx| by r (1 + 2^-52)); the rows of the tile's
    own pose in that box are passed as the pose's cloud, so that the rule's own identity test applies."""
    from octreelib_amd.query import sparse_keep_np

    r = float(radius)
    out = {p: np.zeros(len(rows[p]), dtype=bool) for p in tested}
    counted = [rows[q] for q in among if len(rows[q])]
    if not counted:      # (nothing counts: no row has a neighbour)
        return out
    every = np.vstack(counted)
    lo = every.min(axis=0)
    w = max(r, float((every.max(axis=0) - lo).max()) / 5.0)
    pad = r * (1.0 + 1e-6)
    for p in tested:
        X = rows[p]
        if len(X) == 0:
            continue
        cell = np.floor((X - lo) / w).astype(np.int64)
        uniq, inv = np.unique(cell, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        for g, c in enumerate(uniq):
            mine = np.nonzero(inv == g)[0]
            a, b = lo + c * w - pad, lo + (c + 1) * w + pad
            box = {q: np.nonzero(np.all((rows[q] >= a) & (rows[q] <= b), axis=1))[0] for q in among}
            clouds = [(q, rows[q][box[q]]) for q in among]
            if p in among:
                assert np.all(np.isin(mine, box[p]))
                keep = sparse_keep_np(clouds, [p], r, min_neighbours)[list(among).index(p)]
                out[p][mine] = keep[np.searchsorted(box[p], mine)]
            else:
                out[p][mine] = sparse_keep_np(clouds, [(p, X[mine])], r, min_neighbours)[-1]
    return out


class _Leaf:
    """A leaf as query.HostMap reads one."""

    def __init__(self, corner, edge, rows):
        self.corner_min, self.edge_length, self._rows = corner, edge, rows

    def get_points(self):
        return self._rows


# ---- the model ---------------------------------------------------------------------------------------------------------
class Model:
    """The oracle behind one container: OGrid / OManager / OTree, with the bookkeeping the library keeps on its own
    (validity of the pooled table at the C ABI, what split_stats shows)."""

    def __init__(self, container):
        self.c = container
        kind = container["kind"]
        if kind == "grid":
            self.o = onp.OGrid(container["edge"])
        elif kind == "manager":
            self.o = onp.OManager(np.array(container["corner"], dtype=np.float64), float(container["edge"]))
        else:
            self.o = onp.OTree(np.array(container["corner"], dtype=np.float64), np.float64(container["edge"]))
        self.kind = kind
        self.poses = []
        self.displaced = False
        self.pooled = False          # the device holds a valid pooled table
        self.pooled_key = None
        self.stats = "none"          # "none" | "nan" | record of the last planar build
        self.stats_fresh = False     # nothing has mutated since that build
        self.untouched = False
        self.n_ransac = 0
        self.closest = np.inf        # NotPlanar margin over every node a rule evaluated, in e^2
        self.flags = {"depth2": False, "emptied": False, "late100": False}
        # Neighbours.index: every tree carries `orig`, the row number in the pose's cloud as first inserted of every
        # row of tree.points (-1: a row a map function made); n_inserted counts the rows a pose was ever given
        self.n_inserted = {}
        self.renumbered = False      # a map function replaced the contents: the library numbers the store anew
        # the third generation: what the library's own call must return (carve, remove_poses: the rows that left;
        # store_size: its triple), the counters every ray_evidence of the log returned, by the operation's index
        self.returned = None
        self.n_applied = 0
        self.evidence = {}
        # the fourth generation: the nodes the prunes collapsed since the model was last rebuilt, as (voxel key, corner
        # bytes, edge) - the guard of _guard_collapsed; the evidence records a prune has carried over; what the coverage
        # test tallies about the last operation (never compared with the library)
        self.collapsed = set()
        self.dropped = set()
        self.carried = set()
        self.facts = None

    @classmethod
    def replay(cls, container, log):
        m = cls(container)
        for op in log:
            m.apply(op)
        return m

    # -- structure ----------------------------------------------------------------------------------------------------
    def trees_of(self, p):
        if self.kind == "grid":
            return [self.o.managers[k].octrees[p] for k in self.o.pose_voxels[p]]
        if self.kind == "manager":
            return [self.o.octrees[p]]
        return [self.o]

    def scheme_trees(self):
        if self.kind == "grid":
            return [m.scheme for m in self.o.managers.values()]
        return [self.o.scheme] if self.kind == "manager" else [self.o]

    def managers(self):
        return list(self.o.managers.values()) if self.kind == "grid" else [self.o]

    def counters(self, p):
        if self.kind == "octree":
            return [self.o.n_nodes, self.o.n_leaves, self.o.n_points]
        return [self.o.n_nodes(p), self.o.n_leaves(p), self.o.n_points(p)]

    def leaf_rows(self, p, non_empty=True):
        return [(np.asarray(v.corner, dtype=np.float64), float(v.edge), t.points[v.idx])
                for t in self.trees_of(p) for v in t.leaves(non_empty)]

    def pose_rows(self, p):
        parts = [r for _, _, r in self.leaf_rows(p)]
        return np.vstack(parts) if parts else np.empty((0, 3))

    def observe(self):
        out = {}
        for p in self.poses:
            leaves = self.leaf_rows(p)
            dig = leaf_digests(np.vstack([r for _, _, r in leaves]) if leaves else np.empty((0, 3)),
                               [len(r) for _, _, r in leaves])
            out[p] = ([(((c + 0.0).tobytes(), np.float64(e).tobytes()), d) for (c, e, _), d in zip(leaves, dig)],
                      self.counters(p))
        return out

    def internal_nodes(self, poses=None):
        """{(corner bytes, edge): points of the given poses (None: all) below the node} of every internal node."""
        out = {}

        def walk(node, tree, acc):
            if node.children is None:
                return len(node.idx) if acc else 0
            n = sum(walk(ch, tree, acc) for ch in node.children)
            key = ((np.asarray(node.corner, dtype=np.float64) + 0.0).tobytes(), float(node.edge))
            out[key] = out.get(key, 0) + n
            return n

        if self.kind == "octree":
            walk(self.o.root, self.o, True)
            return out
        for m in self.managers():
            if m.scheme.root.children is None:
                continue
            walk(m.scheme.root, m.scheme, False)      # (every internal node, also where no pose has points)
            for p, t in m.octrees.items():
                if poses is None or p in poses:
                    walk(t.root, t, True)
        return out

    def n_leaves_total(self):
        return sum(len(t.cached) for t in self.scheme_trees())

    def max_depth(self):
        e0 = float(self.c["edge"])
        return max((int(round(np.log2(e0 / float(v.edge)))) for t in self.scheme_trees() for v in t.cached.values()),
                   default=0)

    # -- checks ---------------------------------------------------------------------------------------------------------
    def _distinct(self, poses):
        rows = [self.pose_rows(p) for p in poses]
        rows = np.vstack(rows) if rows else np.empty((0, 3))
        if len(np.unique(rows, axis=0)) != len(rows):
            raise Rejected("points are not distinct")

    def _planar_record(self, plane, K, trees=None):
        """_oracle_nodes on the fresh scheme trees: the margin condition, and what split_stats must show."""
        trees = self.scheme_trees() if trees is None else trees
        try:
            nodes, _ = _oracle_nodes(trees, plane, K)
        except AssertionError as e:
            if "scene unusable" in str(e):
                raise Rejected(str(e))
            raise
        rec = {}
        allrows = None
        if self.kind != "octree":
            allrows = {}
            for m in self.managers():
                rows = [t.points[t.get_idx()] for t in m.octrees.values()]      # (none: only removed poses were here)
                _, lst = _scheme_nodes(m.scheme, np.vstack(rows) if rows else np.empty((0, 3)))
                for c, e, _, idx in lst:
                    allrows[((c + 0.0).tobytes(), e)] = len(idx)
        for k, (e, n, lam, internal, rows) in nodes.items():
            ref = _longdouble_lambda(rows, plane.ddof)[0] if n >= plane.min_points else np.nan
            if n >= plane.min_points:
                self.closest = min(self.closest, abs(lam - plane.max_variance) / (e * e))
            rec[k] = (e, n, ref, bool(internal), n if allrows is None else allrows[k])
        return rec

    # -- operations -------------------------------------------------------------------------------------------------------
    def apply(self, op):
        kind = op["op"]
        index, self.n_applied, self.returned = self.n_applied, self.n_applied + 1, None
        self.facts = None
        fresh = self.stats_fresh
        if kind == "transform_poses_refused":      # (raises DomainError in the library: nothing changes, nothing is invalidated)
            self._transform(op)
        elif kind == "remove_poses_refused":       # (KeyError, before anything changes)
            self._remove(op)
        elif kind == "ray_evidence":
            self.evidence[index] = self._evidence(op)
        elif kind == "store_size":
            assert not self.renumbered
            self.returned = (sum(self.n_inserted[p] for p in self.poses), sum(self.counters(p)[2] for p in self.poses),
                             len(self.poses))
        elif kind in ALL_MUTATING:
            self.untouched = False
            getattr(self, "_sparse" if kind == "remove_sparse" else "_" + kind.split("_")[0])(op)
            if not self.untouched:
                self.pooled = False
                self.pooled_key = None
            if kind not in ("subdivide_planar", "subdivide_planar_count"):
                self.stats_fresh = False
            if kind == "prune" and self.untouched:      # (the call ends before anything is written: the statistics stand)
                self.stats_fresh = fresh
            if self.max_depth() >= 2:
                self.flags["depth2"] = True
        elif kind == "radius_count":
            self._radius(op)
        elif kind == "point_registration_system":
            self._register(op)
        elif kind in ("leaf_planes", "point_to_plane", "plane_segments", "registration_system",
                      "nearest_plane_registration_system") or (kind == "raycast" and op["surface"] == "plane"):
            if kind == "nearest_plane_registration_system":
                self._register(op)
            self.pooled = True      # (each of them makes the pooled table of its selection when the device's is not that)
            self.pooled_key = None if op.get("poses") is None else tuple(sorted(op["poses"]))

    def _insert(self, op):
        p, pts = op["pose"], model_rows(op)
        if op["op"] in MOVED and self.outside(pts):
            raise Rejected("a moved row leaves the domain")
        late = self.n_leaves_total()
        if self.kind == "octree":
            self.o.insert_points(pts)
        else:
            self.o.insert_points(p, pts)
        self.poses.append(p)
        self._set_orig(p, np.arange(len(pts), dtype=np.int64))
        self.n_inserted[p] = len(pts)
        self._distinct([p])
        self._guard_collapsed()
        if self.dropped:      # (a voxel a prune dropped is created anew: an unsplit root at the end of the creation order)
            hit = [k for k in self.o.pose_voxels[p] if k in self.dropped]
            self.facts = {"recreated": len(hit)}
            self.dropped -= set(hit)
        if late >= 100:
            self.flags["late100"] = True

    def _set_orig(self, p, orig):
        """`orig` of the trees of a pose whose rows were just inserted: orig[i] belongs to row i of what was inserted."""
        if self.kind == "grid":
            for key in self.o.pose_voxels[p]:
                self.o.managers[key].octrees[p].orig = orig[self.o.local_to_pose[(key, p)]]
        else:
            self.trees_of(p)[0].orig = orig

    def _extend(self, op):
        p, pts = op["pose"], model_rows(op)
        if op["op"] in MOVED and self.outside(pts):
            raise Rejected("a moved row leaves the domain")
        late = self.n_leaves_total()
        if self.kind == "octree":
            self.o.insert_points(pts)
        else:
            self.o.insert_points(p, pts)
        tree = self.trees_of(p)[0]      # (a manager or an octree: one tree per pose)
        tree.orig = np.concatenate([tree.orig, self.n_inserted[p] + np.arange(len(pts), dtype=np.int64)])
        self.n_inserted[p] += len(pts)
        self._distinct([p])
        self._guard_collapsed()
        if late >= 100:
            self.flags["late100"] = True

    def _subdivide(self, op):
        spec, poses = op["crit"], op["poses"]
        self._distinct(self.poses if poses is None else poses)
        before = set(self.internal_nodes())
        crit = spec[0][1] if len(spec) == 1 and spec[0][0] == "MaxPoints" else build_criteria(spec)
        plane = next((c for c in (crit if isinstance(crit, list) else []) if isinstance(c, NotPlanar)), None)
        K = min((s[1] for s in spec if s[0] == "MaxPoints"), default=-1)
        if self.kind == "octree":
            if plane is not None:      # dry run on the tree's current rows: the margin must hold before the model moves
                dry = onp.OTree(self.o.corner, self.o.edge)
                dry.insert_points(self.o.get_points())
                dry.subdivide(crit)
                rec = self._planar_record(plane, K, [dry])
            self.o.subdivide(crit)
        else:
            self.o.subdivide(crit, poses)
            if plane is not None:
                rec = self._planar_record(plane, K)
        if not before <= set(self.internal_nodes()):
            raise Rejected("the new scheme is not equal-or-finer")
        self.stats = rec if plane is not None else "nan"
        self.stats_fresh = plane is not None

    def _filter(self, op):
        crit = build_filter(op["crit"])
        before = sum(self.counters(p)[1] for p in self.poses)
        if self.kind == "grid":
            self.o.filter(crit)
        elif self.kind == "manager":
            self.o.filter(crit, op.get("poses"))
        else:
            self.o.filter(crit)
        after = sum(self.counters(p)[1] for p in self.poses)
        if after < before:
            self.flags["emptied"] = True
        elif op["op"] == "filter_opaque":
            self.untouched = True      # (evaluated on the host, nothing to remove: the library makes no device call)

    def _map(self, op):
        fn = build_map(op["fn"], cloud_edge(self.c))
        before = {id(t): (t, {id(v): v.idx.copy() for v in t.cached.values()}) for p in self.poses for t in self.trees_of(p)}
        if self.kind == "octree":
            self.o.map_leaf_points(fn)
        else:
            self.o.map_leaf_points(fn, op["poses"])
        # the rows a leaf keeps are matched with its own rows by value, as the library does: a selection keeps the
        # identity of its rows, anything else replaces the contents and the store is numbered anew
        for t, old in before.values():
            orig = np.full(len(t.points), -1, dtype=np.int64)
            orig[: len(t.orig)] = t.orig
            for v in t.cached.values():
                if len(v.idx) and v.idx[0] >= len(t.orig):
                    was = old[id(v)]
                    where = {}
                    for i in was[::-1].tolist():
                        where.setdefault((t.points[i] + 0.0).tobytes(), []).append(i)
                    for i in v.idx.tolist():
                        hit = where.get((t.points[i] + 0.0).tobytes())
                        if hit:
                            orig[i] = t.orig[hit.pop()]
                        else:
                            self.renumbered = True
            t.orig = orig
        if op["fn"] == "shift_z":
            self.displaced = True
            return
        if op["op"] == "map_transform":
            for p in self.poses:
                for c, e, rows in self.leaf_rows(p):
                    if len(rows) and not np.all((rows - c) // e == 0):
                        raise Rejected("a row left its leaf's cube")
                self._distinct([p])

    def pose_rows_orig(self, p):
        """(rows, orig) of the surviving rows of a pose in store order: ascending row number of the inserted cloud."""
        rows, orig = [np.empty((0, 3))], [np.empty(0, dtype=np.int64)]
        for t in self.trees_of(p):
            idx = np.concatenate([v.idx for v in t.leaves(True)] + [np.empty(0, dtype=np.int64)])
            rows.append(t.points[idx])
            orig.append(t.orig[idx])
        rows, orig = np.vstack(rows), np.concatenate(orig)
        order = np.argsort(orig, kind="stable")
        return np.ascontiguousarray(rows[order]), orig[order]

    def identity(self):
        """{pose: (orig, hash)} of the surviving rows in store order - what Neighbours.index must name for the row
        with that hash (row_hashes; rows are distinct within a pose) - or None once the store was numbered anew."""
        if self.renumbered:
            return None
        out = {}
        for p in self.poses:
            rows, orig = self.pose_rows_orig(p)
            out[p] = (orig, row_hashes(rows))
        return out

    def outside(self, rows):
        """The rows the library refuses: not finite, outside the cube (a manager) or the voxel key window (a grid)."""
        if not np.all(np.isfinite(rows)):
            return True
        if self.kind == "grid":
            return bool(len(rows)) and float(np.abs(rows / float(self.c["edge"])).max()) >= 2.0 ** 30
        d = rows - np.array(self.c["corner"], dtype=np.float64)
        return not (np.all(d >= 0.0) and np.all(d < float(self.c["edge"])))

    def _transform(self, op):
        """transform_poses: a fresh model of the same container with every pose inserted again, in slot order: its
        surviving rows in store order, those of the selected poses through transform_np."""
        from octreelib_amd.registration import transform_np

        chosen = [p for p in self.poses if op["poses"] is None or p in op["poses"]]      # (ascending slot order)
        T = {p: motion(m) for p, m in zip(chosen, op["motions"])}
        assert len(T) == len(op["motions"]) and not self.renumbered and not self.displaced
        moved = {}
        for p in self.poses:
            rows, orig = self.pose_rows_orig(p)
            moved[p] = (transform_np(T[p], rows) if p in T else rows, orig)
        refused = any(self.outside(moved[p][0]) for p in chosen)
        if op["op"] == "transform_poses_refused":
            if not refused:
                raise Rejected("the motion stays inside the domain")
            return
        if refused:
            raise Rejected("a moved row leaves the domain")
        fresh = Model(self.c)
        for p in self.poses:
            rows, orig = moved[p]
            fresh.o.insert_points(p, rows)
            fresh.poses.append(p)
            fresh._set_orig(p, orig)
            fresh._distinct([p])
        self.o = fresh.o
        self.collapsed = set()      # (a fresh map: no node of it was ever collapsed)
        self.dropped = set()
        self.stats, self.stats_fresh = "none", False

    # -- the third generation ---------------------------------------------------------------------------------------------
    def scheme_leaves(self):
        """(keys, corner (m, 3), edge (m,)) of every leaf of the scheme, empty ones included; the position in the
        list is the leaf's id here (the library's node ids belong to its own build history)."""
        leaves = [v for t in self.scheme_trees() for v in t.cached.values()]
        corner = np.array([np.asarray(v.corner, dtype=np.float64) for v in leaves], dtype=np.float64).reshape(-1, 3)
        edge = np.array([float(v.edge) for v in leaves], dtype=np.float64)
        return [((c + 0.0).tobytes(), float(e)) for c, e in zip(corner, edge)], corner, edge

    def stored(self):
        return stored_rows(np.vstack([self.pose_rows(p) for p in self.poses] + [np.empty((0, 3))]))

    def _evidence(self, rec):
        """(keys, through, hits) over scheme_leaves(): the record's rays through the library's stated host
        preprocessing (evidence_inputs, the grid's cap), counted by the definition."""
        from octreelib_amd.query import check_evidence_cap, evidence_inputs, ray_evidence_np

        keys, corner, edge = self.scheme_leaves()
        O, D, r, ret = evidence_rays(rec, self.stored(), float(cloud_edge(self.c)))
        inp = evidence_inputs(O, D, r, rec["margin"], rec["min_range"], ret)
        if self.kind == "grid":
            check_evidence_cap(*inp[2:], float(self.c["edge"]))
        ev = ray_evidence_np(*inp, np.arange(len(keys)), corner, edge, len(keys))
        return keys, ev.through, ev.hits

    def _carve(self, op):
        """carve_keep_np over the (leaf, pose) blocks of every selected pose, applied as one oracle apply_mask per
        pose in the pose's own row order; the scheme stays.  The library always compacts (Forest._carved, mask.hip
        forest_carve): the pooled table is invalid afterwards whether rows left or not."""
        from octreelib_amd.query import carve_keep_np

        assert not self.displaced and (op["poses"] is None or self.kind != "octree")
        if op.get("evidence_from") is not None:
            keys, through, hits = self.evidence[op["evidence_from"]]
            # (evidence a prune has carried over needs RayEvidence.remapped: the record says so with "remapped")
            if keys != self.scheme_leaves()[0] or (op["evidence_from"] in self.carried and not op.get("remapped")):
                raise Rejected("the node table has changed since the evidence was taken")
        else:
            keys, through, hits = self._evidence(op)
        local = {k: i for i, k in enumerate(keys)}
        before = sum(self.counters(p)[1] for p in self.poses)
        removed = 0
        for p in self.poses:
            if op["poses"] is not None and p not in op["poses"]:
                continue
            blocks = [(local[((np.asarray(v.corner, dtype=np.float64) + 0.0).tobytes(), float(v.edge))], len(v.idx))
                      for t in self.trees_of(p) for v in t.leaves(True)]
            node = np.array([b[0] for b in blocks], dtype=np.int64)
            keep = carve_keep_np(node, np.zeros(len(node), dtype=np.int64), through, hits, None, op["min_through"],
                                 op["max_hits"])
            mask = np.repeat(keep, [b[1] for b in blocks])
            removed += int((~mask).sum())
            if self.kind == "grid":
                self.o.apply_mask(p, mask)
            else:
                self.trees_of(p)[0].apply_mask(mask)
        self.returned = removed
        if sum(self.counters(p)[1] for p in self.poses) < before:
            self.flags["emptied"] = True

    def _remove(self, op):
        """remove_poses: the oracle trees of the poses are dropped, the scheme trees (and a grid's voxels) stay;
        the numbers are free again and the remaining poses keep their order.  The refused form names a pose the map
        does not hold: KeyError before anything changes."""
        unknown = [p for p in op["poses"] if p not in self.poses]
        if op["op"] == "remove_poses_refused":
            if not unknown:
                raise Rejected("every pose is known")
            return
        gone = sorted(set(op["poses"]))
        assert not unknown and not self.displaced and self.kind != "octree"
        if len(gone) >= len(self.poses):
            raise Rejected("no pose would remain")
        before = sum(self.counters(p)[1] for p in self.poses)
        self.returned = sum(self.counters(p)[2] for p in gone)
        for p in gone:
            if self.kind == "grid":
                for key in self.o.pose_voxels[p]:
                    del self.o.managers[key].octrees[p]
                    del self.o.local_to_pose[(key, p)]
                del self.o.pose_voxels[p], self.o.pose_points[p]
            else:
                del self.o.octrees[p]
            self.poses.remove(p)
            del self.n_inserted[p]
        if sum(self.counters(p)[1] for p in self.poses) < before:
            self.flags["emptied"] = True

    # -- the fourth generation -------------------------------------------------------------------------------------------
    def clouds(self, poses):
        """[(pose, rows)] of the given poses (None: all) in slot order, the rows in the pose's own leaf order."""
        return [(p, self.pose_rows(p)) for p in self.poses if poses is None or p in poses]

    def host_map(self):
        """query.HostMap over the model's own leaves (empty ones included): the host definitions of the map queries."""
        from octreelib_amd.query import HostMap

        leaves = {p: [_Leaf(c, e, r) for c, e, r in self.leaf_rows(p, non_empty=False)] for p in self.poses}
        edge = float(self.c["edge"])
        if self.kind == "grid":
            keys = sorted(k for k, mg in self.o.managers.items() if mg.octrees)
            return HostMap(0, edge, [(np.array(k, dtype=np.float64), edge) for k in keys], leaves)
        return HostMap(1, edge, [(np.array(self.c["corner"], dtype=np.float64), edge)], leaves)

    def _radius(self, op):
        """radius_count: the count does not depend on any order, so the model counts over its own rows."""
        from octreelib_amd.query import radius_count_np

        e = float(cloud_edge(self.c))
        cnt = radius_count_np(count_queries(op, self.stored(), e), self.clouds(op["poses"]), op["radius"] * e,
                              max_count=op["max_count"])
        self.returned = cnt
        self.facts = {"saturated": 0 if op["max_count"] is None else int((cnt == op["max_count"]).sum())}

    def _register(self, op):
        """The two nearest-point registration systems: the counts are exact on both sides (the correspondences are
        those of nearest_np, bit for bit; a plane is accepted by its point count and, with max_variance, by an
        eigenvalue that the two sides round differently - so n_used of the plane form is booked only without it)."""
        from octreelib_amd.query import nearest_np
        from octreelib_amd.registration import transform_np

        e = float(cloud_edge(self.c))
        scan, T = scan_of(op, self.stored(), e)
        r = op["max_distance"] * e
        if op["op"] == "point_registration_system":
            p = transform_np(T, scan)
            nb = nearest_np(p, self.clouds(op["poses"]), 1, max_distance=r)
            used = int((nb.count.reshape(-1) > 0).sum())
            self.returned = (used, int(np.all(np.isfinite(p), axis=1).sum()))
            self.facts = {"n": len(scan), "n_used": used}
            return
        s = self.host_map().nearest_plane_registration_system(
            scan, T, max_distance=r, pose_numbers=op["poses"], min_points=op["min_points"],
            max_variance=op["max_variance"], huber_delta=op["huber_delta"], origin=op["origin"], per_point=True)
        self.returned = (int(s.n_located), int(s.n_used) if op["max_variance"] is None else None)
        self.facts = {"n": len(scan), "n_used": int(s.n_used), "no_plane": int(((s.node >= 0) & (s.row < 0)).sum())}

    def _sparse(self, op):
        """remove_sparse: sparse_keep_np over the model's rows, applied as one oracle apply_mask per tested pose in the
        pose's own row order; the scheme stays.  The library compacts whatever the decisions are (radius.hip:
        octl_forest_remove_sparse goes through mask_apply as carve does): the pooled table is invalid afterwards
        whether rows left or not."""
        assert not self.displaced
        tested = [p for p in self.poses if op["poses"] is None or p in op["poses"]]
        among = [p for p in self.poses if op["among"] is None or p in op["among"]]
        keep = sparse_keep_tiled({p: self.pose_rows(p) for p in self.poses}, tested, among, op["radius"],
                                 op["min_neighbours"])
        before = sum(self.counters(p)[1] for p in self.poses)
        removed = 0
        for p in tested:
            removed += int((~keep[p]).sum())
            if self.kind == "grid":
                self.o.apply_mask(p, keep[p])
            else:
                self.trees_of(p)[0].apply_mask(keep[p])
        self.returned = removed
        self.facts = {"removed": removed}
        if sum(self.counters(p)[1] for p in self.poses) < before:
            self.flags["emptied"] = True

    def _groups(self):
        """(voxel key, [scheme tree, pose trees ...]) of every top-level cube; an octree is its own scheme.  The trees
        of one cube have the same shape (subdivide_as), so their nodes are walked side by side."""
        if self.kind == "octree":
            return [(None, [self.o])]
        if self.kind == "manager":
            return [(None, [self.o.scheme] + list(self.o.octrees.values()))]
        return [(k, [m.scheme] + list(m.octrees.values())) for k, m in self.o.managers.items()]

    @staticmethod
    def _below(nodes):
        """The points of every pose below the node the trees of one cube share."""
        if nodes[0].children is None:
            return sum(len(n.idx) for n in nodes)
        return sum(Model._below([n.children[i] for n in nodes]) for i in range(8))

    def _prune(self, op, dry=False):
        """prune() by the definition of DESIGN 4.18 on the oracle trees: a grid's voxel in which no pose has a point
        leaves the map (managers, every pose's voxel list) and the order of the rest is kept; in the cubes that stay
        the topmost internal nodes without a point below become leaves in the scheme tree and in every pose tree
        (what lay below them goes; a kept internal node keeps its eight children).  dry: nothing changes, the
        outcome is returned - {"voxels", "collapsed", "outer", "bare"}."""
        groups = self._groups()
        nodes_before = sum(trees[0].root.n_nodes() for _, trees in groups)
        gone = [k for k, trees in groups if self.kind == "grid" and self._below([t.root for t in trees]) == 0]
        tops = []

        def walk(vox, nodes):
            if nodes[0].children is None:
                return
            if self._below(nodes) == 0:
                tops.append((vox, nodes))
                return
            for i in range(8):
                walk(vox, [n.children[i] for n in nodes])

        for k, trees in groups:
            if k is None or k not in gone:
                walk(k, [t.root for t in trees])
        dropped = sum(trees[0].root.n_nodes() for k, trees in groups if k is not None and k in gone) \
            + sum(nodes[0].n_nodes() - 1 for _, nodes in tops)
        outer = False
        if gone:
            every, left = np.array([k for k, _ in groups]), np.array([k for k, _ in groups if k not in gone])
            outer = len(left) == 0 or not (np.array_equal(every.min(axis=0), left.min(axis=0))
                                           and np.array_equal(every.max(axis=0), left.max(axis=0)))
        facts = {"voxels": len(gone), "collapsed": len(tops), "outer": bool(outer),
                 "bare": self.kind != "grid" and any(nodes[0] is groups[0][1][0].root for _, nodes in tops)}
        if dry:
            return facts
        key = lambda v: ((np.asarray(v.corner, dtype=np.float64) + 0.0).tobytes(), float(v.edge))
        for k in gone:
            for p in self.o.managers[k].octrees:
                self.o.pose_voxels[p].remove(k)
                del self.o.local_to_pose[(k, p)]
            del self.o.managers[k]
        self.collapsed = {c for c in self.collapsed if c[0] not in gone}
        self.dropped |= set(gone)
        for vox, nodes in tops:
            for x in nodes:
                for ch in x.children:
                    ch._remove_from_cache()
                x.children, x.idx = None, np.empty(0, dtype=np.int64)
                x.tree.cached[id(x)] = x
            self.collapsed.add((vox,) + key(nodes[0]))
        self.returned = (nodes_before - dropped, len(groups) - len(gone), dropped, len(gone), len(tops))
        self.facts = facts
        if not dropped:      # (the library ends the call before it writes a table: content_stamp stands)
            self.untouched = True
            return
        self.stats = "nan"      # (split_stats_valid = false: zeros and NaN, as after a count-driven build)
        # stored evidence, by the rule of RayEvidence.remapped: a leaf that is still there keeps its counters, a
        # collapsed node - it was internal - starts at zero, what was dropped goes
        now = self.scheme_leaves()[0]
        for i, (keys, through, hits) in self.evidence.items():
            old = {k: (t, h) for k, t, h in zip(keys, through.tolist(), hits.tolist())}
            self.evidence[i] = (now, np.array([old.get(k, (0, 0))[0] for k in now], dtype=through.dtype),
                                np.array([old.get(k, (0, 0))[1] for k in now], dtype=hits.dtype))
            self.carried.add(i)

    def _guard_collapsed(self):
        """After an insert or an extend: Rejected when a row went into a node a prune has collapsed.  Neither the
        reference nor DESIGN says where in a pose's leaf list a collapsed node stands once it is filled again (it is
        empty, so until then no listing shows it); transform_poses rebuilds the map and lifts the guard."""
        if not self.collapsed:
            return
        for vox, trees in self._groups():
            for t in trees[0 if self.kind == "octree" else 1:]:
                for v in t.cached.values():
                    if len(v.idx) and (vox, (np.asarray(v.corner, dtype=np.float64) + 0.0).tobytes(), float(v.edge)) \
                            in self.collapsed:
                        raise Rejected("a row falls into a node the last prune collapsed")

    def _apply(self, op):
        p = op["pose"]
        tree = self.trees_of(p)[0]
        before = tree.n_leaves
        mask = np.random.default_rng([op["seed"], 0x3A5C]).random(tree.n_points) < op["keep"]
        tree.apply_mask(mask)
        if tree.n_leaves < before:
            self.flags["emptied"] = True

    def _ransac(self, op):
        np.random.seed(op["np_seed"])
        table = np.random.random((op["H"], 6))
        n = len(self.poses)
        before = sum(self.counters(p)[1] for p in self.poses)
        for i in range(0, n, op["ppb"]):
            batch = list(range(i, min(i + op["ppb"], n)))
            clouds, sizes = [], []
            for p in batch:
                for _, _, rows in self.leaf_rows(p):
                    clouds.append(rows)
                    sizes.append(len(rows))
            if not clouds:
                continue
            mask = rnp.evaluate(np.vstack(clouds), np.array(sizes, dtype=np.int32), table, op["thr"])
            off = 0
            for p in batch:
                m = self.o.n_points(p)
                self.o.apply_mask(p, mask[off: off + m])
                off += m
        self.n_ransac += 1
        if sum(self.counters(p)[1] for p in self.poses) < before:
            self.flags["emptied"] = True


# ---- the generator ---------------------------------------------------------------------------------------------------
class Sequence:
    def __init__(self, seed, container, log, obs, meta, draws, rejected, flags, closest, ident=None):
        self.seed, self.container, self.log, self.obs, self.meta = seed, container, log, obs, meta
        self.draws, self.rejected, self.flags, self.closest = draws, rejected, flags, closest
        self.ident = ident      # per step Model.identity() (the second generation only)

    def printed(self, upto=None):
        ops = self.log if upto is None else self.log[: upto + 1]
        # (a piecewise insert names up to 1024 motions: the first and the last are printed, generate(seed) has them all)
        ops = [{**op, "motions": [op["motions"][0], f"... {len(op['motions'])} in all ...", op["motions"][-1]]}
               if len(op.get("motions") or ()) > 8 else op for op in ops]
        return "\n".join([f"seed {self.seed} container {self.container}"] + [f"  {i:2d} {op}" for i, op in enumerate(ops)])


def _container(seed, rng):
    c = _CONTAINER[seed % 12]
    kind = c if isinstance(c, str) else c[seed // 12 % 2]
    if kind == "grid":
        utm = seed % 12 in (2, 10)
        return {"kind": "grid", "edge": 1 if utm else int(rng.choice([1, 2, 5])), "utm": utm}
    s = int(rng.choice([1, 2]))
    return {"kind": kind, "corner": [-2.0 * s] * 3, "edge": 4.0 * s, "utm": False}


class _Generator:
    read_kinds = READ_ONLY

    def __init__(self, seed, index=None):
        self.seed = seed
        self.rng = np.random.default_rng([seed, 0x0B5E9])
        seed = self.index = seed if index is None else index      # (what the seed's number fixes goes by this)
        self.ident = None
        self.container = _container(seed, self.rng)
        self.kind = self.container["kind"]
        self.model = Model(self.container)
        self.log, self.obs, self.meta = [], [], []
        self.draws = self.rejected = 0
        self.cloud_seed = 1000 * seed
        self.cloud_edge = cloud_edge(self.container)
        self.f32 = seed % 3 == 0 and not self.container["utm"] or seed % 12 in (4, 7)
        self.pose_order = ([1, 0, 2, 3, 4, 5] if seed % 4 == 1 else list(range(6))) if self.kind == "grid" \
            else MANAGER_POSES
        self.max_poses = 1 if self.kind == "octree" else int(self.rng.integers(4, 6))   # (a motif may add the sixth)
        self.in_motif = False
        self.shallow = seed % 12 in (1, 5)
        self.first_subdivide = "subdivide_count" if self.shallow else SUBDIVIDES[seed % 4]

    # -- parameters of one operation of a kind, or None when its precondition does not hold ---------------------------
    def _cloud_record(self, small=False):
        self.cloud_seed += 1
        form = "f64"
        r = self.rng.random()
        if self.f32 and r < 0.6:
            form = "f32"
        elif r > 0.8:
            form = "fortran" if r > 0.9 else "strided"
        n = int(self.rng.integers(2000, 4000 if small else 9000))
        return {"seed": self.cloud_seed, "n": n, "edge": self.cloud_edge, "utm": self.container["utm"], "form": form,
                "cube": self.kind != "grid"}

    def _subset(self, always=False):
        poses = self.model.poses
        if self.kind == "octree" or len(poses) < 2 or (not always and self.rng.random() < 0.5):
            return None
        k = int(self.rng.integers(1, len(poses)))
        return sorted(int(p) for p in self.rng.choice(poses, k, replace=False))

    def _count_k(self, poses):
        """K of a count rule that is equal-or-finer than the current scheme, None when there is none >= 4."""
        nodes = self.model.internal_nodes(poses)
        if not nodes:
            if self.shallow:      # few, dense internal nodes: a re-subdivide stays possible after points have left
                return int(self.rng.integers(200, 250))
            return int(self.rng.integers(30, 250)) if self.kind == "grid" else int(self.rng.integers(16, 48))
        cmin = min(nodes.values())
        if cmin < 3:
            return None
        return int(self.rng.integers(max(2, cmin // 2), cmin))

    def params(self, kind):
        m, rng = self.model, self.rng
        has_points = bool(m.poses) and any(m.counters(p)[2] > 0 for p in m.poses)
        split = bool(m.internal_nodes())
        if kind == "insert":
            if len(m.poses) >= (self.max_poses if not self.in_motif else 1 if self.kind == "octree" else 6):
                return None
            return {"op": kind, "pose": self.pose_order[len(m.poses)], "cloud": self._cloud_record()}
        if kind == "extend":
            if self.kind == "grid" or not m.poses or m.displaced:
                return None
            return {"op": kind, "pose": int(rng.choice(m.poses)), "cloud": self._cloud_record(small=True)}
        if kind in SUBDIVIDES:
            if not has_points or m.displaced or (self.kind == "octree" and split):
                return None
            if not split and kind != self.first_subdivide and self.first_subdivide is not None:
                kind = self.first_subdivide
            poses = self._subset()
            e2 = float(self.cloud_edge) ** 2
            plane = ["NotPlanar", float(rng.choice([2.5e-4, 1.0e-3])) * e2, int(rng.choice([8, 16])), int(rng.integers(0, 2))]
            if kind == "subdivide_planar":
                if split:
                    return None
                return {"op": kind, "crit": [plane], "poses": poses}
            if kind == "subdivide_callable":
                if split:
                    k = self._count_k(poses)
                    crit = None if k is None else [["big_and_wide", k, 0.0]]
                else:
                    crit = [["big_and_wide", int(rng.integers(30, 120)), 0.05 * float(self.cloud_edge)]]
                return None if crit is None else {"op": kind, "crit": crit, "poses": poses}
            k = self._count_k(poses)
            if k is None and poses is not None:
                poses, k = None, self._count_k(None)
            if k is None:
                return None
            if kind == "subdivide_planar_count":
                return {"op": kind, "crit": [plane, ["MaxPoints", max(k, 60) if not split else k]], "poses": poses}
            return {"op": kind, "crit": [["MaxPoints", k]], "poses": poses}
        if kind in FILTERS:
            if not has_points or (kind == "filter_subset" and (self.kind != "manager" or len(m.poses) < 2)):
                return None
            if kind == "filter_opaque":
                sp = [_spread(r) for p in m.poses for _, _, r in m.leaf_rows(p)]
                if len(sp) < 4:
                    return None
                crit = ["spread_lt", float(np.quantile(sp, float(rng.uniform(0.6, 0.9))))]
            else:
                crit = [["ge", int(rng.integers(3, 9))], ["lt", int(rng.integers(40, 200))],
                        ["between", int(rng.integers(2, 6)), int(rng.integers(60, 300))]][int(rng.integers(0, 3))]
            op = {"op": kind, "crit": crit}
            if kind == "filter_subset":
                op["poses"] = self._subset(always=True)
            return op
        if kind in ("map_select", "map_transform"):
            if not has_points or m.displaced:
                return None
            fn = str(rng.choice(["every_other", "first_half", "upper_z"])) if kind == "map_select" else "toward_mean"
            return {"op": kind, "fn": fn, "poses": self._subset()}
        if kind == "apply_mask":
            if self.kind == "grid" or not has_points:
                return None
            return {"op": kind, "pose": int(rng.choice(m.poses)), "seed": int(rng.integers(1 << 30)),
                    "keep": float(rng.choice([0.5, 0.7, 0.9]))}
        if kind == "ransac":
            if self.kind != "grid" or not has_points or m.n_ransac >= 2 or sorted(m.poses) != list(range(len(m.poses))):
                return None
            return {"op": kind, "H": int(rng.choice([64, 256, 1024])), "thr": float(rng.choice([0.01, 0.02])),
                    "ppb": int(rng.integers(1, 4)), "np_seed": int(rng.integers(1 << 30))}
        # read-only
        if not m.poses:
            return None
        if kind in ("leaf_statistics", "get_leaf_points"):
            return {"op": kind, "pose": int(rng.choice(m.poses))}
        if kind == "locate":
            return {"op": kind, "seed": int(rng.integers(1 << 30)), "n": 300}
        if kind == "leaf_planes":
            return {"op": kind, "poses": self._subset()}
        if kind == "point_to_plane":
            return {"op": kind, "poses": self._subset(), "seed": int(rng.integers(1 << 30)), "n": 300,
                    "min_points": int(rng.choice([1, 8, 16])),
                    "max_variance": [None, 1e-3 * float(self.cloud_edge) ** 2][int(rng.integers(0, 2))]}
        return {"op": kind}

    # -- one step -------------------------------------------------------------------------------------------------------
    def step(self, kind, fix=None):
        """Draw parameters for `kind` until the model accepts them (at most 4 times); False when the kind cannot be
        drawn in this state."""
        for _ in range(4):
            op = self.params(kind)
            if op is None:
                return False
            if fix:
                op.update(fix)
            self.draws += 1
            try:
                self.model.apply(op)
            except Rejected:
                self.rejected += 1
                flags, closest = self.model.flags, self.model.closest
                self.model = Model.replay(self.container, self.log)
                self.model.flags, self.model.closest = flags, min(closest, self.model.closest)
                continue
            self.log.append(op)
            mutating = op["op"] in ALL_MUTATING
            self.obs.append(self.model.observe() if mutating or not self.obs else self.obs[-1])
            if self.ident is not None:
                self.ident.append(self.model.identity() if mutating or not self.ident else self.ident[-1])
            st = self.model.stats
            self.meta.append({"mutating": mutating, "pooled": self.model.pooled,
                              "stats": st if isinstance(st, str) or self.model.stats_fresh else "stale"})
            if self.model.returned is not None:      # (the third generation: what the library's call must return)
                self.meta[-1]["returns"] = self.model.returned
            if self.model.facts is not None:         # (the fourth generation: what the coverage test tallies)
                self.meta[-1]["facts"] = self.model.facts
            return True
        return False

    def reads(self, lo, hi, avoid=()):
        for _ in range(int(self.rng.integers(lo, hi + 1))):
            kinds = [k for k in self.read_kinds if k not in avoid]
            self.step(str(self.rng.choice(kinds)))

    def run(self):
        rng = self.rng
        n0 = 1 if self.kind == "octree" else int(rng.integers(1, 4))
        for _ in range(n0):
            self.step("insert")
        self.reads(0, 1)
        motif = list(_MOTIF[self.seed % 12])
        if self.seed % 12 == 5 and self.kind == "octree":      # (an octree subdivides once: the motif comes first)
            self._motif(motif)
            motif = None
        self.step(self.first_subdivide)
        self.first_subdivide = None
        self.reads(1, 2)
        if self.kind == "octree":
            self.step("extend")
        else:
            self.step("insert")      # a late pose into the scheme
        self.reads(1, 1)
        weights = {"insert": 2, "extend": 3, "subdivide_count": 3, "subdivide_planar_count": 2, "subdivide_planar": 1,
                   "subdivide_callable": 2, "filter_count": 5, "filter_opaque": 3, "filter_subset": 3, "map_select": 3,
                   "map_transform": 2, "apply_mask": 8, "ransac": 2}
        if self.kind == "manager":
            weights.update({"filter_subset": 8, "insert": 1})
        n_mut = int(rng.integers(3, 7))
        at = 0 if self.shallow else int(rng.integers(0, 2))
        for i in range(n_mut):
            if motif is not None and i == at:
                self._motif(motif)
                motif = None
                self.reads(1, 1)
                continue
            if len(self.log) >= (12 if self.kind == "grid" else 9) and motif is None:
                break
            kinds = list(weights)
            w = np.array([weights[k] for k in kinds], dtype=float)
            for _ in range(6):
                if self.step(str(rng.choice(kinds, p=w / w.sum()))):
                    break
            self.reads(1, 2)
        if self.kind == "grid" and self.seed % 2 == 0:
            self.step("filter_opaque")
        if self.kind != "manager" and self.seed % 2 == 1:
            self.step("map_select")
        if self.kind == "manager":
            self.step("filter_subset")
        if self.kind != "grid":
            self.step("apply_mask")
            self.reads(1, 1)
        if not self.model.flags["emptied"]:
            self.step("filter_count", {"crit": ["ge", 6]})
        if self.seed % 4 == 3 and self.model.poses and not self.model.displaced and len(self.log) <= 18:
            # rows displaced out of their cubes: the last mutating operation, only statistics and queries follow
            self.step("map_transform", {"fn": "shift_z", "poses": None})
            for k in ("point_to_plane", "leaf_statistics")[: 20 - len(self.log)]:
                self.step(k)
        return Sequence(self.seed, self.container, self.log, self.obs, self.meta, self.draws, self.rejected,
                        self.model.flags, self.model.closest)

    def _motif(self, kinds):
        subset = None
        self.in_motif = True
        for k in kinds:
            fix = None
            if self.seed % 12 == 7 and k in ("leaf_planes", "point_to_plane"):
                if subset is None:
                    subset = self._subset(always=True) or [self.model.poses[0]]
                fix = {"poses": subset}
            ok = self.step(k, fix)
            assert ok, f"seed {self.seed}: motif step {k} cannot be drawn\n" + \
                "\n".join(str(o) for o in self.log)
        self.in_motif = False


class _Generator2(_Generator):
    """The second generation: the map queries (nearest, raycast, plane_segments, registration_system,
    adjustment_system) among the read-only kinds, transform_poses and its refused form among the mutating ones.  A
    transform_poses leaves no scheme, so a subdivide is always the next mutating operation."""

    read_kinds = READ_ONLY + NEW_READ_ONLY

    def __init__(self, seed, first=SEEDS2[0]):
        super().__init__(seed, seed - first)
        self.cloud_seed = 1000 * seed
        self.ident = []

    def _centre(self):
        return [float(x) for x in (UTM if self.container["utm"] else np.zeros(3))]

    def _motion(self, angle, shift):
        """A drawn rigid motion about the scene's centre: a rotation of up to `angle` about a drawn axis, a translation
        of up to `shift` per axis (a scalar or one bound per axis and sign: (3, 2))."""
        rng = self.rng
        axis = rng.normal(size=3)
        w = axis / np.linalg.norm(axis) * float(rng.uniform(0.2, 1.0)) * angle
        b = np.broadcast_to(np.asarray(shift, dtype=np.float64).reshape(-1, 1), (3, 2)) if np.ndim(shift) < 2 else shift
        u = rng.uniform(-1.0, 1.0, 3)
        v = np.where(u < 0, u * b[:, 0], u * b[:, 1])
        return {"xi": [float(x) for x in np.concatenate([w, v])], "origin": self._centre()}

    def _pose_motions(self, chosen):
        """One small motion per chosen pose.  A manager's clouds fill its cube, so there the motion is scaled by the
        room the pose's rows leave to the walls."""
        e, out = float(self.cloud_edge), []
        for p in chosen:
            if self.kind == "grid":
                out.append(self._motion(0.05, 0.25 * e))
                continue
            rows = self.model.pose_rows(p)
            lo = np.array(self.container["corner"], dtype=np.float64)
            hi = lo + float(self.container["edge"])
            if len(rows) == 0:
                out.append(self._motion(0.05, 0.25 * e))
                continue
            room = np.stack([(rows - lo).min(axis=0), (hi - rows).min(axis=0)], axis=1)      # (3, 2): towards -, towards +
            reach = float(np.abs(rows).max()) * np.sqrt(3.0)
            angle = min(0.05, 0.3 * float(room.min()) / reach)
            out.append(self._motion(angle, np.minimum(0.25 * e, 0.5 * np.maximum(room - angle * reach, 0.0))))
        return out

    def params(self, kind):
        m, rng = self.model, self.rng
        e = float(self.cloud_edge)
        if kind not in NEW_MUTATING + NEW_READ_ONLY:
            if m.displaced and kind in ("leaf_planes", "locate", "node_cubes", "get_leaf_points", "counters", "split_stats"):
                return None      # (after rows were displaced: the queries that must refuse, and the two gen-1 draws)
            return super().params(kind)
        has_points = bool(m.poses) and any(m.counters(p)[2] > 0 for p in m.poses)
        if not has_points:
            return None
        gates = lambda: {"min_points": int(rng.choice([1, 8, 16])),
                         "max_variance": [None, 1e-3 * e ** 2][int(rng.integers(0, 2))]}
        if kind in NEW_MUTATING:
            if self.kind == "octree" or m.displaced or m.renumbered:
                return None
            poses = self._subset()
            chosen = [p for p in m.poses if poses is None or p in poses]
            if kind == "transform_poses":
                return {"op": kind, "poses": poses, "motions": self._pose_motions(chosen)}
            motions = [self._motion(0.01, 0.0) for _ in chosen]
            far = 2.0 ** 31 * float(self.container["edge"]) if self.kind == "grid" else 5.0 * float(self.container["edge"])
            motions[int(rng.integers(0, len(chosen)))]["xi"][3 + int(rng.integers(0, 3))] = float(far)
            return {"op": kind, "poses": poses, "motions": motions}
        if m.displaced and kind not in ("nearest", "raycast"):
            return None
        if kind == "nearest":
            return {"op": kind, "seed": int(rng.integers(1 << 30)), "n": 300, "k": int(rng.choice([1, 3, 8])),
                    "r": float(rng.choice([0.05, 0.5, 2.0])) * e, "poses": self._subset()}
        if kind == "raycast":
            return {"op": kind, "seed": int(rng.integers(1 << 30)), "n": 300, "surface": str(rng.choice(["cube", "plane"])),
                    "poses": self._subset(), **gates(), "max_range": float(rng.uniform(0.5, 8.0)) * e,
                    "min_range": [0.0, 0.1 * e][int(rng.integers(0, 2))]}
        if kind == "plane_segments":
            return {"op": kind, "poses": self._subset(), "min_points": int(rng.choice([8, 16])),
                    "max_variance": [None, 1e-3 * e ** 2][int(rng.integers(0, 2))],
                    "max_angle": float(rng.choice([0.1, 0.3])), "max_offset": float(rng.choice([0.05, 0.02])) * e}
        if kind == "registration_system":
            with_points = [p for p in m.poses if m.counters(p)[2] > 0]
            return {"op": kind, "pose": int(rng.choice(with_points)), "seed": int(rng.integers(1 << 30)),
                    "n": int(rng.integers(300, 1001)), "motion": self._motion(0.02, 0.02 * e),
                    "inverse": bool(rng.integers(0, 2)), "poses": self._subset(), **gates(),
                    "max_distance": [None, 0.2 * e][int(rng.integers(0, 2))],
                    "huber_delta": [None, 0.02 * e][int(rng.integers(0, 2))]}
        # adjustment_system
        if self.kind == "octree" or len(m.poses) < 2:
            return None
        poses = self._subset()
        if poses is not None and len(poses) < 2:
            poses = None
        S = len(m.poses) if poses is None else len(poses)
        return {"op": kind, "poses": poses, "min_points": 8, "min_poses": 2,
                "max_variance": [None, 1e-3 * e ** 2][int(rng.integers(0, 2))],
                "motions": None if rng.random() < 0.5 else [self._motion(0.003, 0.004 * e) for _ in range(S)]}

    def must(self, kind, fix=None):
        ok = self.step(kind, fix)
        assert ok, f"seed {self.seed}: step {kind} cannot be drawn\n{Sequence.printed(self)}"

    def subdivide_again(self):
        """The subdivide that follows a transform_poses."""
        for kind in self.rng.permutation(["subdivide_count", "subdivide_planar_count", "subdivide_callable",
                                          "subdivide_count"]).tolist():
            if self.step(kind):
                return
        raise AssertionError(f"seed {self.seed}: no subdivide can be drawn\n{Sequence.printed(self)}")

    def transform_then_subdivide(self, fix=None, reads=(0, 1)):
        if not self.step("transform_poses", fix):
            return False
        self.reads(*reads)      # (as on a map that was never subdivided)
        self.subdivide_again()
        return True

    def mutate(self, weights):
        kinds = list(weights)
        w = np.array([weights[k] for k in kinds], dtype=float)
        for _ in range(6):
            kind = str(self.rng.choice(kinds, p=w / w.sum()))
            if self.transform_then_subdivide() if kind == "transform_poses" else self.step(kind):
                return True
        return False

    def run(self):
        rng, j = self.rng, self.index % 12
        second = self.index >= 12
        for _ in range(1 if self.kind == "octree" else int(rng.integers(2, 4))):
            self.step("insert")
        self.reads(0, 1)
        self.step(self.first_subdivide)
        self.first_subdivide = None
        self.reads(1, 2)
        self.step("extend" if self.kind == "octree" else "insert")      # a late pose into the scheme
        self.reads(1, 1)
        weights = {"insert": 1, "extend": 2, "subdivide_count": 2, "subdivide_planar_count": 1, "subdivide_callable": 1,
                   "filter_count": 4, "filter_opaque": 2, "filter_subset": 3, "map_select": 3, "map_transform": 1,
                   "apply_mask": 6, "ransac": 2, "transform_poses": 5, "transform_poses_refused": 3}
        if self.index % 3 != 1 or j in (2, 3):      # rows leave before the motif: a mask or a filter
            for kind in ("apply_mask", "ransac", "filter_count"):
                if kind != "ransac" or j not in (1, 10):      # (the motif's own RANSAC: at most two per sequence)
                    if self.step(kind):
                        break
            self.reads(1, 1)
        self._motif2(j, second)
        self.reads(1, 1)
        if self.index % 4 == 2 and self.step("transform_poses_refused"):
            self.reads(1, 1)
        for _ in range(int(rng.integers(1, 3))):
            if len(self.log) >= 17:
                break
            self.mutate(weights)
            self.reads(1, 2)
        if not self.model.flags["emptied"] and not self.model.displaced:
            self.step("filter_count", {"crit": ["ge", 6]})
            self.reads(1, 1)
        if (j == 4 or (j == 0 and len(self.log) <= 18)) and not self.model.displaced:
            # rows displaced out of their cubes: the last mutating operation; nearest and raycast must refuse
            self.must("map_transform", {"fn": "shift_z", "poses": None})
            self.must("nearest")
            for k in ("raycast", "point_to_plane", "leaf_statistics"):
                self.step(k)
        return Sequence(self.seed, self.container, self.log, self.obs, self.meta, self.draws, self.rejected,
                        self.model.flags, self.model.closest, self.ident)

    def _motif2(self, j, second):
        """The transition the seed's number fixes, with nothing mutating in between but what it names."""
        self.in_motif = True
        part = self._subset(always=True)      # (a proper subset S; S' is all poses)
        sub = (j in (2, 7, 11)) != second
        tp = {"poses": part if sub else None}
        if j in (0, 7) and part is not None:
            self.must("nearest", {"poses": part})
            self.must("raycast", {"poses": None, "surface": "cube"})
            self.must("nearest", {"poses": part})
        elif j == 1:
            self.must("ransac")
            self.must("raycast")
        elif j in (2, 10):
            self._fixed_transform(tp)
            self.subdivide_again()
            self.must("nearest" if j == 2 else "ransac")
        elif j in (3, 11):
            self.must("adjustment_system")
            self._fixed_transform(tp)
            self.subdivide_again()
            self.must("adjustment_system")
        elif j == 5 or (j == 4 and second):
            self.must("plane_segments")
            first = dict(self.log[-1])
            self.must("filter_count")
            self.must("plane_segments", first)
        elif j == 6 and part is not None:
            self.must("leaf_planes", {"poses": part})
            self.must("raycast", {"poses": None, "surface": "plane"})
            self.must("point_to_plane", {"poses": part})
        elif j == 8:
            self.must("point_to_plane", {"poses": part})
            self.must("transform_poses_refused")
            self.must("point_to_plane", {"poses": part})
        elif j == 9:
            self.must("apply_mask")
            self.must("raycast")
        elif j == 4:
            self.must("registration_system")
        if j == 7:
            self._fixed_transform(tp)
            self.subdivide_again()
            self.must("apply_mask")
        self.in_motif = False

    def _fixed_transform(self, fix):
        """transform_poses for the selection `fix` names (the motions are drawn for it)."""
        chosen = [p for p in self.model.poses if fix["poses"] is None or p in fix["poses"]]
        for _ in range(4):
            if self.step("transform_poses", {"poses": fix["poses"], "motions": self._pose_motions(chosen)}):
                self.reads(0, 1)
                return
        raise AssertionError(f"seed {self.seed}: no transform_poses can be drawn\n{Sequence.printed(self)}")


# the motif (and, for four seeds, a second one) of the third generation by seed - 200: the letters are the entries of
# TRANSITIONS3 in order
_MOTIF3 = {0: "b", 1: "i", 2: "e", 3: "a", 4: "c", 5: "m", 6: "j", 7: "f", 8: "d", 9: "g", 10: "h", 11: "l", 12: "b",
           13: "i", 14: "k", 15: "n", 16: "c", 17: "j", 18: "a", 19: "l", 20: "k", 21: "m", 22: "f", 23: "d"}
_MOTIF3_SECOND = {0: "h", 12: "g", 11: "e", 19: "n"}


class _Generator3(_Generator2):
    """The third generation: insert_moved / extend_moved, carve, remove_poses and its refused form among the mutating
    kinds, ray_evidence and store_size among the read-only ones.  A manager's and an octree's clouds fill the cube, so
    a cloud that goes in under a motion is drawn at 0.6 of the usual extent there: under every drawn motion it stays
    inside (1.2 s + 0.12 * 1.2 sqrt(3) s + 0.35 s < 2 s).  On a grid it is drawn that small where the motif needs the
    insert to create no voxel (evidence taken before it must still fit the node table)."""

    read_kinds = GEN3_ALL_READ_ONLY

    def __init__(self, seed, first=SEEDS3[0]):
        super().__init__(seed, first)
        self.inside = False          # moved clouds stay inside the voxels that exist
        self.piecewise = None        # None: drawn
        self.n_moved = self.n_piecewise = 0

    def _moved(self, op):
        """The motion(s), the matrix form and - for some - a device form for an insert / extend record."""
        rng, e, c = self.rng, float(self.cloud_edge), op["cloud"]
        inside = self.kind != "grid" or self.inside
        if inside:
            c["edge"] = 0.6 * self.cloud_edge
        k = self.index + self.n_moved
        self.n_moved += 1
        if rng.random() < 0.5:
            c["form"] = "device64" if c["utm"] or k % 2 else "device32"
        op["matrix"] = ["4x4", "3x4"][int(rng.integers(0, 2))]
        base = self._motion(0.1, 0.3 * e) if inside else self._motion(0.3, 1.0 * e)
        if not (rng.random() < 0.5 if self.piecewise is None else self.piecewise):
            op["motion"] = base
            return op
        k = self.index + self.n_piecewise
        self.n_piecewise += 1
        M = [1024, 2, 7][k % 3]
        step = rng.uniform(-1.0, 1.0, 6) * np.array([0.02] * 3 + [0.05 * e] * 3)      # (a sweep: the pose drifts)
        xi = np.array(base["xi"])
        op["motions"] = [{"xi": [float(x) for x in xi + step * (i / (M - 1))], "origin": base["origin"]} for i in range(M)]
        op["segment_seed"] = int(rng.integers(1 << 30))
        op["segment_dtype"] = ["int32", "uint16", "int64"][(k // 3 + k) % 3]
        return op

    def params(self, kind):
        m, rng = self.model, self.rng
        e = float(self.cloud_edge)
        if kind not in GEN3_MUTATING + GEN3_READ_ONLY:
            op = super().params(kind)
            if op is not None and kind == "insert":      # (a freed number first: pose numbers are no longer a prefix)
                op["pose"] = next(p for p in self.pose_order if p not in m.poses)
            return op
        if kind in MOVED:
            op = self.params("insert" if kind == "insert_moved" else "extend")
            if op is None:
                return None
            op["op"] = kind
            return self._moved(op)
        if not m.poses:
            return None
        has_points = any(m.counters(p)[2] > 0 for p in m.poses)
        rays = lambda: {"seed": int(rng.integers(1 << 30)), "n": 300, "margin": float(rng.choice([0.0, 0.02, 0.1])) * e,
                        "min_range": [0.0, 0.1 * e][int(rng.integers(0, 2))]}
        if kind == "ray_evidence":
            return {"op": kind, **rays(), "returned": [None, 0.1, 0.3][int(rng.integers(0, 3))]}
        if kind == "store_size":
            return None if m.renumbered else {"op": kind}
        if kind == "carve":
            if not has_points or m.displaced:
                return None
            # (min_through above the number of rays: nothing is freed, and the library still compacts)
            return {"op": kind, **rays(), "min_through": int(rng.choice([2, 4, 8, 1000], p=[0.3, 0.3, 0.25, 0.15])),
                    "max_hits": int(rng.choice([0, 1, 3])),
                    "poses": self._subset(), "fused": bool(rng.integers(0, 2))}
        if self.kind == "octree" or m.displaced:
            return None
        if kind == "remove_poses":
            if len(m.poses) < 2:
                return None
            k = 2 if len(m.poses) >= 4 and rng.random() < 0.3 else 1
            poses = sorted(int(p) for p in rng.choice(m.poses, k, replace=False))
            return {"op": kind, "poses": poses + poses[:1] if rng.random() < 0.15 else poses}      # (twice is once)
        # remove_poses_refused: a number the map does not hold (never used, or freed), alone or behind a known one
        unknown = int(rng.choice([p for p in range(12) if p not in m.poses]))
        return {"op": kind, "poses": [unknown] if rng.random() < 0.5 else [int(rng.choice(m.poses)), unknown]}

    def run(self):
        rng, idx = self.rng, self.index
        first, second = _MOTIF3[idx], _MOTIF3_SECOND.get(idx)
        tree = self.kind == "octree"
        many = {first, second} & {"g", "k", "n", "d"}
        for i in range(1 if tree else 3 if many else int(rng.integers(2, 4))):
            self.must("insert_moved" if i == 0 and idx % 4 == 0 else "insert")
        self.reads(0, 1)
        kind, self.first_subdivide = self.first_subdivide, None
        if first == "j":
            # the scheme from ONE pose, and only where its points are many AND wide (no chain of nodes down into a tight
            # cluster of its own): the other poses have points in every internal node, so that an equal-or-finer
            # count rule still exists once the driving pose has left
            self.must("subdivide_callable", {"crit": [["big_and_wide", 300, 0.6 * float(self.cloud_edge)]],
                                             "poses": [self.model.poses[idx % 2]]})
        else:
            self.must(kind)
        self.reads(1, 2)
        late = ("extend_moved" if idx % 2 else "extend") if tree else ("insert_moved" if idx % 2 else "insert")
        self.must(late)      # a late pose into the scheme
        self.reads(1, 1)
        if idx % 3 != 1:      # rows leave before the motif: a mask, a filter or a carve
            for kind in ("apply_mask", "ransac", "carve", "filter_count")[idx % 2:]:
                if kind != "ransac" or first not in ("b", "i"):      # (the motif's own RANSAC: at most two per sequence)
                    if self.step(kind):
                        break
            self.reads(1, 1)
        self._motif3(first)
        self.reads(1, 1)
        if second is not None:
            self._motif3(second)
            self.reads(1, 1)
        if idx % 4 in (1, 2) and self.step("remove_poses_refused"):
            self.reads(1, 1)
        weights = {"insert": 1, "insert_moved": 3, "extend": 1, "extend_moved": 4, "subdivide_count": 2,
                   "subdivide_planar_count": 1, "filter_count": 2, "filter_subset": 1, "map_select": 2, "apply_mask": 3,
                   "ransac": 1, "transform_poses": 2, "carve": 6, "remove_poses": 4, "remove_poses_refused": 3}
        for _ in range(int(rng.integers(1, 3))):
            if len(self.log) >= 21:
                break
            self.mutate(weights)
            self.reads(1, 2)
        if not self.model.flags["emptied"]:
            self.step("filter_count", {"crit": ["ge", 6]})
            self.reads(1, 1)
        return Sequence(self.seed, self.container, self.log, self.obs, self.meta, self.draws, self.rejected,
                        self.model.flags, self.model.closest, self.ident)

    def _motif3(self, name):
        """The transition of TRANSITIONS3 the letter names, with nothing mutating in between but what it lists."""
        rng = self.rng
        poses = lambda: list(self.model.poses)
        self.in_motif = True
        if name == "a":
            self.must("carve")
            carved = self.log[-1]["poses"] or poses()
            self.reads(0, 1)
            self.must("remove_poses", {"poses": [int(rng.choice(carved))]})
        elif name == "b":
            self.must("ransac")
            self.must("carve")
        elif name == "c":
            self.must("carve")
            self.must("plane_segments")
        elif name == "d":
            self.must("carve")
            self._fixed_transform({"poses": None if self.index < 12 else self._subset(always=True)})
            self.subdivide_again()
            self.must("adjustment_system")
        elif name in ("e", "f"):
            self.must("ray_evidence")
            k = len(self.log) - 1
            if name == "e":
                self.must("remove_poses")
            else:
                self.inside = True
                self.must("insert_moved")
                self.inside = False
            self.must("carve", {"evidence_from": k, "fused": False})
        elif name == "g":
            part = self._subset(always=True)
            self.must("leaf_planes", {"poses": part})
            self.must("remove_poses", {"poses": [int(rng.choice([p for p in poses() if p not in part]))]})
            self.must("point_to_plane", {"poses": part})
        elif name == "h":
            self.must("nearest")
            self.must("remove_poses", {"poses": [poses()[1 if len(poses()) > 2 else 0]]})      # (a middle slot)
            self.must("nearest")
        elif name == "i":
            self.must("remove_poses", {"poses": [poses()[0 if self.index < 12 else 1]]})       # (the first slot; a middle one)
            self.must("insert")
            self.must("ransac")
        elif name == "j":
            driving = next(op["poses"] for op in self.log if op["op"] in SUBDIVIDES)
            self.must("remove_poses", {"poses": driving})
            self.must("subdivide_planar_count")
            self.must("split_stats")
        elif name == "k":
            self.must("remove_poses", {"poses": [poses()[0]]})
            self.reads(0, 1)
            self.must("remove_poses")
        elif name == "l":
            self.piecewise = True
            self.must("insert_moved")
            self.piecewise = None
            self.must("nearest")
        elif name == "m":
            self.must("extend_moved")
            self.must("leaf_statistics", {"pose": self.log[-1]["pose"]})
        elif name == "n":
            self.must("adjustment_system")
            self.must("remove_poses")
            self.must("adjustment_system")
        self.in_motif = False


# the motifs of the fourth generation by seed - 300: the letters are the entries of TRANSITIONS4 in order
_MOTIF4 = {0: "al", 1: "bm", 2: "ek", 3: "cn", 4: "go", 5: "ds", 6: "h", 7: "jp", 8: "iq", 9: "rt", 10: "fh", 11: "eo",
           12: "as", 13: "gk", 14: "il", 15: "bm", 16: "ct", 17: "jq", 18: "rd", 19: "fn", 20: "gp", 21: "fk", 22: "h",
           23: "pd"}


class _Generator4(_Generator3):
    """The fourth generation: remove_sparse and prune among the mutating kinds, radius_count and the two nearest-point
    registration systems among the read-only ones.  Once a prune has collapsed a node, no insert or extend is drawn
    (Model._guard_collapsed would reject nearly every cloud: they fill the scene) until a transform_poses has rebuilt
    the map; the motifs that insert after a prune make holes that collapse nothing - a pose stored one and a half
    voxels out of the scene, alone in the voxels it adds, and removed again."""

    read_kinds = ALL_READ_ONLY

    def __init__(self, seed):
        super().__init__(seed, SEEDS4[0])
        self.n_counts = 0

    def params(self, kind):
        m, rng = self.model, self.rng
        e = float(self.cloud_edge)
        if kind not in GEN4_MUTATING + GEN4_READ_ONLY:
            if m.collapsed and kind in ("insert", "extend") + MOVED:
                return None
            return super().params(kind)
        if not m.poses or m.displaced:
            return None
        has_points = any(m.counters(p)[2] > 0 for p in m.poses)
        if kind == "prune":
            return {"op": kind}
        if not has_points:
            return None
        if kind == "radius_count":      # (on a grid the radius is at most twice the voxel edge, which is the cloud edge)
            self.n_counts += 1      # (the caps in turn, so that the seed set has each of them whatever else is drawn)
            return {"op": kind, "seed": int(rng.integers(1 << 30)), "n": 300, "radius": float(rng.choice([0.05, 0.2, 0.5])),
                    "max_count": [None, 1, 3, 7][(self.index // 3 + self.n_counts) % 4], "poses": self._subset()}
        if kind == "remove_sparse":
            return {"op": kind, "radius": float(rng.choice([0.05, 0.1, 0.2])) * e,
                    "min_neighbours": int(rng.choice([1, 2, 4])), "poses": self._subset(), "among": self._subset()}
        # the two registration systems: from the identity up to a shift of a few leaf edges, or right out of the scene
        how = str(rng.choice(["identity", "small", "leaves", "far"], p=[0.2, 0.3, 0.35, 0.15]))
        mo = {"identity": {"xi": [0.0] * 6, "origin": self._centre()}, "small": self._motion(0.02, 0.02 * e),
              "leaves": self._motion(0.05, 0.5 * e), "far": {"xi": [0.0, 0.0, 0.0, 6.0 * e, 0.0, 0.0], "origin": self._centre()}}[how]
        op = {"op": kind, "seed": int(rng.integers(1 << 30)), "n": int(rng.integers(300, 1001)), "motion": mo,
              "max_distance": float(rng.choice([0.05, 0.3, 1.0])), "huber_delta": [None, 0.02 * e][int(rng.integers(0, 2))],
              "origin": [None, [float(x) for x in np.array(self._centre()) + rng.uniform(-1.0, 1.0, 3) * e]][int(rng.integers(0, 2))],
              "poses": self._subset()}
        if kind == "nearest_plane_registration_system":
            op.update({"min_points": int(rng.choice([1, 8, 16])), "max_variance": [None, 1e-3 * e ** 2][int(rng.integers(0, 2))]})
        return op

    def holes(self, want="change"):
        """Mutating operations until a prune would find something to do (want "change"), or a voxel to drop ("voxels"):
        a remove_sparse that takes the uniform background away - the use the library's docstring names - then count
        filters of rising strictness."""
        e = float(self.cloud_edge)
        ok = lambda f: f["voxels"] + f["collapsed"] > 0 if want == "change" else f[want] > 0
        if ok(self.model._prune(None, dry=True)):
            return
        few = sum(self.model.counters(p)[2] > 0 for p in self.model.poses) < 2
        steps = [("remove_sparse", {"radius": 0.15 * e, "min_neighbours": 2 if few else 4, "poses": None, "among": None})] \
            + [("filter_count", {"crit": ["ge", c]}) for c in (8, 20, 50)]
        for kind, fix in steps[: 1 if self.shallow else None]:
            if self.step(kind, fix) and ok(self.model._prune(None, dry=True)):
                return
        if self.shallow:      # (few, dense internal nodes: none of them can be emptied - the prune finds nothing)
            return
        raise AssertionError(f"seed {self.seed}: no holes for a prune\n{Sequence.printed(self)}")

    def tie(self):
        """{"radius", "min_neighbours", ...} of a remove_sparse over every pose that the INCLUSIVE comparison decides: a
        stored row x with exactly min_neighbours other rows within the radius, the farthest of them at
        d2 == fl(radius radius) bit for bit (d2 by the formula of radius_count_np).  x stays; under d2 < r2 it would
        go.  The radius is kept between 0.05 and 0.25 cloud edges, as the drawn ones are."""
        e = float(self.cloud_edge)
        rows = np.vstack([self.model.pose_rows(p) for p in self.model.poses])
        for _ in range(256):
            d = rows[int(self.rng.integers(0, len(rows)))] - rows
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            t = np.partition(d2, 4)[int(self.rng.integers(1, 5))]      # (d2 = 0 is the row itself)
            if not (0.05 * e) ** 2 <= t <= (0.25 * e) ** 2:
                continue
            for r in (np.sqrt(t), np.nextafter(np.sqrt(t), 0.0), np.nextafter(np.sqrt(t), np.inf)):
                if r * r == t:
                    return {"radius": float(r), "min_neighbours": int((d2 <= t).sum()) - 1, "poses": None, "among": None}
        raise AssertionError(f"seed {self.seed}: no radius with an exact tie\n{Sequence.printed(self)}")

    def gentle(self, first):
        """{"radius", "min_neighbours", ...} of a remove_sparse that takes rows out of leaves of the
        segments of `first` (a plane_segments record over every pose) and empties no leaf: the pooled plane table keeps
        its rows, so a segment table kept across the call would still fit it - and would be wrong.  Found by trying
        the rule on the model's rows."""
        m, e = self.model, float(self.cloud_edge)
        hm = m.host_map()
        seg = hm.plane_segments(None, first["min_points"], first["max_variance"], first["max_angle"], first["max_offset"])
        key = lambda c, w: ((np.asarray(c, dtype=np.float64) + 0.0).tobytes(), float(w))
        nd = hm.nodes
        labelled = {key(nd["corner"][n], nd["edge"][n]) for n, lab in zip(seg.planes.node.tolist(), seg.label.tolist()) if lab >= 0}
        leaves = {p: [(key(c, w), len(r)) for c, w, r in m.leaf_rows(p)] for p in m.poses}
        rows = {p: m.pose_rows(p) for p in m.poses}
        # (one pose alone first: where its row is the last of its own in a leaf, another pose may still hold one there)
        for r, k in ((0.25, 1), (0.2, 1), (0.15, 1), (0.25, 2), (0.1, 1), (0.2, 2)):
            for tested in ([[p] for p in m.poses] if len(m.poses) > 1 else []) + [None]:
                keep = sparse_keep_tiled(rows, m.poses if tested is None else tested, m.poses, r * e, k)
                left, gone = collections.Counter(), collections.Counter()
                for p in m.poses:
                    at = 0
                    for leaf, n in leaves[p]:
                        stay = int(keep[p][at: at + n].sum()) if p in keep else n
                        left[leaf], gone[leaf], at = left[leaf] + stay, gone[leaf] + n - stay, at + n
                if all(left.values()) and any(gone[leaf] for leaf in labelled):
                    return {"radius": r * e, "min_neighbours": k, "poses": tested, "among": None}
        raise AssertionError(f"seed {self.seed}: no remove_sparse that thins a segment and empties no leaf\n{Sequence.printed(self)}")

    def outward(self):
        """The motion that stores a cloud one and a half voxels out of the scene along an axis the seed fixes."""
        xi = [0.0] * 6
        xi[3 + self.index % 3] = (-1.5 if self.index % 2 else 1.5) * float(self.cloud_edge)
        return {"xi": xi, "origin": self._centre()}

    def lonely_pose(self):
        """A late pose alone in the voxels it adds, inserted and removed again: holes that collapse no node."""
        self.piecewise = False
        self.must("insert_moved", {"motion": self.outward()})
        self.piecewise = None
        pose = self.log[-1]["pose"]
        self.must("remove_poses", {"poses": [pose]})
        return pose

    def pruned(self, **facts):
        """A prune whose outcome the motif needs."""
        self.must("prune")
        got = self.meta[-1]["facts"]
        for k, want in facts.items():
            assert (got[k] > 0) == want, f"seed {self.seed}: prune {got}, wanted {facts}\n{Sequence.printed(self)}"

    def again(self, first):
        self.must(first["op"], dict(first))

    def run(self):
        rng, idx = self.rng, self.index
        names = _MOTIF4[idx]
        tree = self.kind == "octree"
        for i in range(1 if tree else 3 if set(names) & set("enpqr") else int(rng.integers(2, 4))):
            self.must("insert_moved" if i == 0 and idx % 4 == 0 else "insert")
        self.reads(0, 1)
        kind, self.first_subdivide = self.first_subdivide, None
        self.must(kind)
        if tree and "f" in names:      # (an octree subdivides once: the motif is here)
            assert kind == "subdivide_planar_count"
            self.must("prune")
            self.must("split_stats")
        self.reads(1, 2)
        late = ("extend_moved" if idx % 2 else "extend") if tree else ("insert_moved" if idx % 2 else "insert")
        self.must(late)      # a late pose into the scheme
        self.reads(1, 1)
        if idx % 3 != 1 and not set(names) & set("hi"):      # rows leave before the motif: a mask, a filter, a carve or the sparse rows
            for kind in ("apply_mask", "ransac", "remove_sparse", "carve", "filter_count")[idx % 3:]:
                if kind != "ransac" or "h" not in names:      # (the motif's own RANSAC: at most two per sequence)
                    if self.step(kind):
                        break
            self.reads(1, 1)
        for name in names:
            if not (tree and name == "f"):
                self._motif4(name)
                self.reads(1, 1)
        weights = {"insert": 1, "insert_moved": 2, "extend": 1, "extend_moved": 2, "subdivide_count": 2,
                   "subdivide_planar_count": 1, "filter_count": 2, "filter_subset": 1, "map_select": 1, "apply_mask": 2,
                   "ransac": 1, "transform_poses": 2, "carve": 3, "remove_poses": 2, "remove_poses_refused": 1,
                   "remove_sparse": 6, "prune": 6}
        for _ in range(int(rng.integers(1, 3))):
            if len(self.log) >= 23:
                break
            self.mutate(weights)
            self.reads(1, 2)
        if not self.model.flags["emptied"]:
            self.step("filter_count", {"crit": ["ge", 6]})
            self.reads(1, 1)
        if idx == 20:      # a manager emptied to its bare root: every row is sparse when a million neighbours are asked for
            self.must("remove_sparse", {"radius": 0.1 * float(self.cloud_edge), "min_neighbours": 10 ** 6, "poses": None,
                                        "among": None})
            self.pruned(bare=True)
            self.reads(1, 2)
        return Sequence(self.seed, self.container, self.log, self.obs, self.meta, self.draws, self.rejected,
                        self.model.flags, self.model.closest, self.ident)

    def _motif4(self, name):
        """The transition of TRANSITIONS4 the letter names, with nothing mutating in between but what it lists."""
        rng = self.rng
        poses = lambda: list(self.model.poses)
        part = lambda: self._subset(always=True) or poses()[:1]      # (a proper subset S where there are two poses)
        self.in_motif = True
        if name in ("a", "b"):
            S_ = part()
            if name == "a":
                self.holes()
            else:
                self.must("prune")      # (whatever it finds: the next one finds nothing)
            self.must("leaf_planes", {"poses": S_})
            self.pruned(voxels=False, collapsed=False) if name == "b" else self.must("prune")
            self.must("point_to_plane", {"poses": S_})
        elif name in ("c", "d", "t"):
            self.holes()
            self.must({"c": "plane_segments", "d": "nearest", "t": "point_registration_system"}[name])
            first = self.log[-1]
            self.must("prune")
            self.again(first)
        elif name == "e":
            self.lonely_pose()
            self.must("adjustment_system")
            self.pruned(voxels=True, outer=True)
            self.must("adjustment_system")
        elif name == "f":
            self.must("subdivide_planar_count")
            self.must("prune")
            self.must("split_stats")
        elif name == "g":
            self.holes()
            self.must("ray_evidence")
            k = len(self.log) - 1
            self.must("prune")
            self.must("carve", {"evidence_from": k, "fused": False, "remapped": True})
        elif name == "h":
            self.lonely_pose()
            self.pruned(voxels=True, collapsed=False)
            self.piecewise = False
            self.must("insert_moved", {"motion": self.outward()})      # (the same number, into the voxels that went)
            self.piecewise = None
            assert self.meta[-1]["facts"]["recreated"] > 0
            self.subdivide_again()
            self.must("ransac")
        elif name == "i":
            pose = self.lonely_pose()
            self.pruned(collapsed=False)
            self.must("insert")
            assert self.log[-1]["pose"] == pose
        elif name == "j":
            self.must("carve")
            self.must("prune")
            self._fixed_transform({"poses": None if self.index < 12 else self._subset(always=True)})
            self.subdivide_again()
        elif name == "k":
            self.holes()
            self.must("prune")
            self.pruned(voxels=False, collapsed=False)
        elif name == "l":
            self.must("radius_count", {"poses": None if self.index < 12 else part(), "max_count": None})
            first = self.log[-1]
            self.must("remove_sparse")
            self.again(first)
        elif name == "m":
            self.must("remove_sparse", self.tie())      # (decided by d2 == r2: the inclusive comparison)
            self.must("nearest")
        elif name == "n":
            self.must("remove_sparse", {"poses": part(), "among": part()})
            self.must("prune")
        elif name in ("o", "p", "s"):
            self.must({"o": "plane_segments", "p": "adjustment_system", "s": "nearest_plane_registration_system"}[name],
                      {"poses": None} if name == "o" else
                      # (the second of the two seeds: right out of the scene, so that no point is used)
                      {"motion": {"xi": [0.0, 0.0, 0.0, 6.0 * float(self.cloud_edge), 0.0, 0.0], "origin": self._centre()},
                       "max_distance": 0.3} if name == "s" and self.index >= 12 else None)
            first = self.log[-1]
            # (o: the plane table keeps its rows, a stale segment table would still fit; p: decided by d2 == r2)
            self.must("remove_sparse", self.gentle(first) if name == "o" else self.tie() if name == "p" else None)
            self.again(first)
        elif name in ("q", "r"):
            S_ = part()
            self.must("nearest" if name == "q" else "leaf_planes", {"poses": S_})
            first = self.log[-1]
            self.must("point_registration_system" if name == "q" else "nearest_plane_registration_system", {"poses": None})
            self.again(first) if name == "q" else self.must("point_to_plane", {"poses": S_})
        self.in_motif = False


@functools.lru_cache(maxsize=None)
def generate(seed):
    if seed < SEEDS2[0]:
        return _Generator(seed).run()
    if seed < SEEDS3[0]:
        return _Generator2(seed).run()
    return _Generator3(seed).run() if seed < SEEDS4[0] else _Generator4(seed).run()


# ---- what the logs must cover ------------------------------------------------------------------------------------------
def transitions(log):
    """The names of TRANSITIONS that occur in a log with nothing mutating in between."""
    found = set()
    mut = [i for i, op in enumerate(log) if op["op"] in MUTATING]
    fam = lambda k: "subdivide" if k in SUBDIVIDES else "filter" if k in FILTERS else k

    def reads_after(i):
        out = []
        for op in log[i + 1:]:
            if op["op"] in MUTATING:
                break
            out.append(op)
        return out

    for a, i in enumerate(mut):
        k = fam(log[i]["op"])
        nxt = log[mut[a + 1]] if a + 1 < len(mut) else None
        after = reads_after(i)
        names = [op["op"] for op in after]
        if k == "ransac" and "leaf_planes" in names:
            found.add("ransac>leaf_planes")
        if k == "extend" and "leaf_statistics" in names:
            found.add("extend>leaf_statistics")
        if k == "filter":
            pooled = [n for n in names if n in ("leaf_planes", "point_to_plane")]
            if pooled and pooled[0] == "point_to_plane":
                found.add("filter>point_to_plane")
        if nxt is not None:
            pair = f"{k}>{fam(nxt['op'])}"
            if pair in ("ransac>subdivide", "ransac>insert", "filter>insert", "map_transform>subdivide",
                        "map_select>ransac"):
                found.add(pair)
            if log[i]["op"] in ("subdivide_planar", "subdivide_planar_count") and nxt["op"] == "subdivide_count" \
                    and "split_stats" in [op["op"] for op in reads_after(mut[a + 1])]:
                found.add("planar>count>split_stats")
        if k in ("insert", "ransac"):
            before = [op for op in log[(mut[a - 1] + 1 if a else 0): i] if op["op"] in ("leaf_planes", "point_to_plane")]
            pooled = [op for op in after if op["op"] in ("leaf_planes", "point_to_plane")]
            if before and pooled and pooled[0]["op"] == "point_to_plane":
                if k == "insert" and before[-1]["poses"] is not None and before[-1]["poses"] == pooled[0]["poses"]:
                    found.add("leaf_planes(S)>insert>point_to_plane(S)")
                if k == "ransac" and before[-1]["op"] == "point_to_plane":
                    found.add("point_to_plane>ransac>point_to_plane")
    if sum(op["op"] == "ransac" for op in log) >= 2:
        found.add("two_ransac")
    return found


def transitions2(log):
    """The names of TRANSITIONS2 that occur in a log of the second generation, with nothing mutating in between but
    what the name itself lists."""
    found = set()
    fam = lambda k: "subdivide" if k in SUBDIVIDES else "filter" if k in FILTERS else k
    mut = [i for i, op in enumerate(log) if op["op"] in ALL_MUTATING]
    sel = lambda op: None if op.get("poses") is None else tuple(sorted(op["poses"]))

    def reads_between(a):
        """The read-only operations after the a-th mutating one, up to the next."""
        end = mut[a + 1] if a + 1 < len(mut) else len(log)
        return log[mut[a] + 1: end]

    for a, i in enumerate(mut):
        k = fam(log[i]["op"])
        after = reads_between(a)
        chain = [fam(log[m]["op"]) for m in mut[a: a + 3]]
        if chain[:2] == ["transform_poses", "subdivide"]:
            if any(op["op"] == "nearest" for op in reads_between(a + 1)):
                found.add("transform_poses>subdivide>nearest")
            if len(chain) == 3 and chain[2] in ("ransac", "apply_mask"):      # (a grid's RANSAC applies its mask itself)
                found.add("transform_poses>subdivide>ransac>apply_mask")
            before = log[(mut[a - 1] + 1 if a else 0): i]
            if any(op["op"] == "adjustment_system" for op in before) \
                    and any(op["op"] == "adjustment_system" for op in reads_between(a + 1)):
                found.add("adjustment_system>transform_poses>subdivide>adjustment_system")
        if k in ("ransac", "apply_mask") and after and after[0]["op"] == "raycast":
            found.add("apply_mask>raycast")      # (the first call that looks at the forest after the mask)
        if k == "transform_poses_refused" and after and after[0]["op"] == "point_to_plane":
            found.add("transform_poses_refused>point_to_plane")
        if log[i].get("fn") == "shift_z" and any(op["op"] == "nearest" for op in after):
            found.add("map_transform(shift_z)>nearest")
        if k == "filter" and a and after:
            before = [op for op in reads_between(a - 1) if op["op"] == "plane_segments"]
            again = [op for op in after if op["op"] == "plane_segments"]
            if before and again and {n: v for n, v in before[-1].items()} == dict(again[0]):
                found.add("plane_segments>filter>plane_segments")
    for i in range(len(log) - 2):
        x, y, z = log[i: i + 3]
        if sel(x) is not None and sel(x) == sel(z) and sel(y) != sel(x):
            if x["op"] == "leaf_planes" and y["op"] == "raycast" and y["surface"] == "plane" and z["op"] == "point_to_plane":
                found.add("leaf_planes(S)>raycast_plane(S')>point_to_plane(S)")
            if x["op"] == "nearest" and y["op"] == "raycast" and y["surface"] == "cube" and z["op"] == "nearest":
                found.add("nearest(S)>raycast_cube(S')>nearest(S)")
    return found


def transitions3(log):
    """The names of TRANSITIONS3 that occur in a log of the third generation, with nothing mutating in between but
    what the name itself lists (a refused call counts as mutating here: it must not stand in between either)."""
    found = set()
    fam = lambda k: "subdivide" if k in SUBDIVIDES else k
    mut = [i for i, op in enumerate(log) if op["op"] in ALL_MUTATING]
    sel = lambda op: None if op.get("poses") is None else tuple(sorted(op["poses"]))

    def reads_between(a):
        """The read-only operations after the a-th mutating one (-1: from the start), up to the next."""
        start = mut[a] + 1 if a >= 0 else 0
        return log[start: mut[a + 1] if a + 1 < len(mut) else len(log)]

    for a, i in enumerate(mut):
        op, k = log[i], log[i]["op"]
        before, after = reads_between(a - 1), reads_between(a)
        names = [o["op"] for o in after]
        chain = [fam(log[j]["op"]) for j in mut[a: a + 3]]
        nxt = log[mut[a + 1]] if a + 1 < len(mut) else None
        if k == "carve":
            if nxt is not None and nxt["op"] == "remove_poses" and (op["poses"] is None or set(op["poses"]) & set(nxt["poses"])):
                found.add("carve>remove_poses(carved pose)")
            if i and log[i - 1]["op"] == "ransac":      # (directly: the asynchronous mask is still on its way)
                found.add("ransac>carve")
            if "plane_segments" in names:
                found.add("carve>plane_segments")
            if chain[1:] == ["transform_poses", "subdivide"] \
                    and any(o["op"] == "adjustment_system" for o in reads_between(a + 2)):
                found.add("carve>transform_poses>subdivide>adjustment_system")
            src = op.get("evidence_from")
            if src is not None and a and src > (mut[a - 2] if a >= 2 else -1) and src < mut[a - 1]:
                assert log[src]["op"] == "ray_evidence"
                if log[mut[a - 1]]["op"] == "remove_poses":
                    found.add("ray_evidence>remove_poses>carve(evidence_from)")
                if log[mut[a - 1]]["op"] == "insert_moved":
                    found.add("ray_evidence>insert_moved>carve(evidence_from)")
        if k == "remove_poses":
            planes = [o for o in before if o["op"] == "leaf_planes"]
            pooled = [o for o in after if o["op"] in ("leaf_planes", "point_to_plane")]
            if planes and pooled and sel(planes[-1]) is not None and not set(planes[-1]["poses"]) & set(op["poses"]) \
                    and pooled[0]["op"] == "point_to_plane" and sel(pooled[0]) == sel(planes[-1]):
                found.add("leaf_planes(S)>remove_poses(not in S)>point_to_plane(S)")
            for name in ("nearest", "adjustment_system"):
                if any(o["op"] == name for o in before) and name in names:
                    found.add(f"{name}>remove_poses>{name}")
            if chain[1:] == ["insert", "ransac"] and log[mut[a + 1]]["pose"] in op["poses"]:
                found.add("remove_poses>insert(freed number)>ransac")
            built = [o for o in log[:i] if o["op"] in SUBDIVIDES]
            if built and sel(built[-1]) is not None and sel(built[-1]) == tuple(sorted(set(op["poses"]))) \
                    and nxt is not None and nxt["op"] == "subdivide_planar_count" \
                    and any(o["op"] == "split_stats" for o in reads_between(a + 1)):
                found.add("remove_poses(scheme-driving subset)>subdivide_planar_count>split_stats")
            if nxt is not None and nxt["op"] == "remove_poses":
                found.add("remove_poses>remove_poses")
        if k == "insert_moved" and "motions" in op and "nearest" in names:
            earlier = [fam(o["op"]) for o in log[:i] if fam(o["op"]) in ("subdivide", "transform_poses")]
            if earlier and earlier[-1] == "subdivide":      # late: into a scheme
                found.add("insert_moved(late, piecewise)>nearest")
        if k == "extend_moved" and "leaf_statistics" in names:
            found.add("extend_moved>leaf_statistics")
    return found


def transitions4(log, meta):
    """The names of TRANSITIONS4 that occur in a log of the fourth generation, with nothing mutating in between but
    what the name itself lists (a refused call counts as mutating here, as in transitions3).  What a prune found and
    whether an insert re-created a dropped voxel is read from the bookkeeping (meta[i]["facts"])."""
    found = set()
    T = TRANSITIONS4
    fam = lambda k: "subdivide" if k in SUBDIVIDES else "insert" if k in ("insert", "insert_moved") else k
    mut = [i for i, op in enumerate(log) if op["op"] in ALL_MUTATING]
    sel = lambda op: None if op.get("poses") is None else tuple(sorted(op["poses"]))
    pooling = lambda o: o["op"] in ("leaf_planes", "point_to_plane", "plane_segments", "registration_system",
                                    "nearest_plane_registration_system") or (o["op"] == "raycast" and o["surface"] == "plane")

    def reads_between(a):
        """The read-only operations after the a-th mutating one (-1: from the start), up to the next."""
        start = mut[a] + 1 if a >= 0 else 0
        return log[start: mut[a + 1] if a + 1 < len(mut) else len(log)]

    for a, i in enumerate(mut):
        op, k = log[i], log[i]["op"]
        before, after = reads_between(a - 1), reads_between(a)
        names = [o["op"] for o in after]
        chain = [fam(log[j]["op"]) for j in mut[a: a + 4]]
        prev = log[mut[a - 1]] if a else None
        nxt = log[mut[a + 1]] if a + 1 < len(mut) else None

        def around(name, same=True):
            """The last `name` before and the first one after - the same record, where that is asked for."""
            b, c = [o for o in before if o["op"] == name], [o for o in after if o["op"] == name]
            return bool(b and c and (not same or b[-1] == c[0]))

        if k == "prune":
            facts = meta[i]["facts"]
            pb, pa = [o for o in before if pooling(o)], [o for o in after if pooling(o)]
            if pb and pa and pb[-1]["op"] == "leaf_planes" and pa[0]["op"] == "point_to_plane" \
                    and sel(pb[-1]) is not None and sel(pb[-1]) == sel(pa[0]):
                found.add(T[0] if facts["voxels"] + facts["collapsed"] else T[1])
            if around("plane_segments"):
                found.add(T[2])
            if around("nearest"):
                found.add(T[3])
            if facts["outer"] and around("adjustment_system", same=False):
                found.add(T[4])
            if prev is not None and prev["op"] in ("subdivide_planar", "subdivide_planar_count") and "split_stats" in names:
                found.add(T[5])
            if nxt is not None and nxt["op"] == "carve" and nxt.get("remapped") and nxt.get("evidence_from") is not None \
                    and (mut[a - 1] if a else -1) < nxt["evidence_from"] < i:
                assert log[nxt["evidence_from"]]["op"] == "ray_evidence"
                found.add(T[6])
            if facts["voxels"] and chain[1:] == ["insert", "subdivide", "ransac"] \
                    and meta[mut[a + 1]].get("facts", {}).get("recreated"):
                found.add(T[7])
            if prev is not None and prev["op"] == "remove_poses" and nxt is not None and fam(nxt["op"]) == "insert" \
                    and nxt["pose"] in prev["poses"]:
                found.add(T[8])
            if prev is not None and prev["op"] == "carve" and chain[1:3] == ["transform_poses", "subdivide"]:
                found.add(T[9])
            if nxt is not None and nxt["op"] == "prune":
                found.add(T[10])
            if prev is not None and prev["op"] == "remove_sparse" and prev["poses"] is not None and prev["among"] is not None:
                found.add(T[13])
            if around("point_registration_system"):
                found.add(T[19])
        if k == "remove_sparse":
            if around("radius_count"):
                found.add(T[11])
            if "nearest" in names:
                found.add(T[12])
            if around("plane_segments"):
                found.add(T[14])
            if around("adjustment_system", same=False):
                found.add(T[15])
            if around("nearest_plane_registration_system"):
                found.add(T[18])
    for i in range(len(log) - 2):
        x, y, z = log[i: i + 3]
        if sel(x) is not None and sel(x) == sel(z) and sel(y) != sel(x):
            if x["op"] == "nearest" and y["op"] == "point_registration_system" and z["op"] == "nearest":
                found.add(T[16])
            if x["op"] == "leaf_planes" and y["op"] == "nearest_plane_registration_system" and z["op"] == "point_to_plane":
                found.add(T[17])
    return found
