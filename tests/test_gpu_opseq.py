"""
Differential fuzz of random operation sequences over the whole API: the logs of tests/_opseq.py replayed on Grid /
OctreeManager / Octree and, after EVERY operation, everything a caller can observe checked with the contract the
project states elsewhere (no tolerance is introduced here):

  * every pose: leaf tables (corner bits, edge bits, row multisets), leaf list order, the counters - exactly, against
    the oracle model (tests/_util.assert_same_leaves);
  * leaf_statistics of every pose: bound 1 and the eigen contract of tests/test_gpu_leaf_stats.py;
  * split_stats: the bound of tests/test_gpu_planarity.py after a planar build, all NaN after a count-driven one;
  * locate == locate_np on tables downloaded now; every stored, undisplaced point locates to the leaf that stores it;
  * leaf_planes: the pooled bound of tests/test_gpu_query.py (_check_planes); point_to_plane rows / NaN rules equal to
    point_to_plane_np on the returned table, distances within 4 eps sum |n_i d_i| of the longdouble value;
  * nearest == nearest_np and raycast == raycast_np (both surfaces), bit for bit, on rows, leaves and planes downloaded
    now (tests/test_gpu_nearest.py, tests/test_gpu_raycast.py); Neighbours.index names rows of the clouds as first
    inserted, by the MODEL's bookkeeping (Sequence.ident), through masks, filters, extend and transform_poses;
  * plane_segments: neighbour, label, root, n_leaves equal to plane_segments_np, the merged table within the bound of
    tests/test_gpu_segments.py; registration_system: per-point answers and the sums under the contract of
    tests/test_gpu_registration.py; adjustment_system: the block table is that of the leaves downloaded now (moments
    within the bound of tests/test_gpu_adjustment.py::test_block_moments), the sums under _check_system;
  * transform_poses_refused raises DomainError and changes nothing; after rows were displaced nearest and raycast raise
    RuntimeError;
  * the third generation (SEEDS3): ray_evidence == ray_evidence_np count for count on the node table downloaded now
    (tests/test_gpu_evidence.py) and is read-only; carve - carve_rays or carve(ray_evidence(...)), or carve with the
    evidence an earlier operation of the log returned - and remove_poses return the number of rows the model lost, and
    the tables afterwards are the model's; directly before and after a remove_poses every remaining pose reads back
    the same bytes (get_points, leaf list, leaf_statistics, counters) and leaf_planes / nearest / raycast over the
    remaining poses before equal the calls over every pose after; store_size is (rows the remaining poses were
    given, alive rows, poses); remove_poses_refused raises KeyError and changes nothing; what insert_moved /
    extend_moved store is transform_rows_np of the cloud as given - a host array of any form or a DeviceCloud - bit
    for bit, and Neighbours.index names the rows of that cloud;
  * the fourth generation (SEEDS4): radius_count == the model's own count and == radius_count_np on the rows
    downloaded now, and is read-only; remove_sparse returns the number of rows the model lost, the tables afterwards
    are the model's, and the poses it does not judge read back the same bytes directly before and after; prune
    returns the model's five numbers, the tables after are prune_np of the tables before, every map query before
    equals the query after through node_map and every pose reads back the same rows, leaves and statistics
    (tests/test_gpu_prune.py: _prune_and_check, _queries, _queries_equal, on the state the log has reached); a carve
    takes evidence over the prunes in between with RayEvidence.remapped; point_registration_system: .neighbours is
    nearest_np(k = 1) bit for bit, the sums under _check_sums of tests/test_gpu_point_registration.py, n_used and
    n_located the model's; nearest_plane_registration_system: _check_per_point and _check_sums of
    tests/test_gpu_nearest_plane_registration.py, .planes under the pooled bound; the default origin of
    adjustment_system is the centre of the root cubes downloaded now;
  * after every operation, next to the queries above: one radius_count and one of each nearest-point registration
    system against their definitions on tables downloaded afterwards (RuntimeError once rows are displaced);
  * the queries are read-only (tables, permutation, coordinates, counters, the error word);
  * at the C ABI octl_forest_point_to_plane answers OCTL_E_STATE exactly when the model says something mutating has
    happened since the last pooled table.
What the log's own read-only operations RETURN is checked too, on every object, against tables downloaded at that
moment with the host-side caches put back afterwards (Device.neutral): a drawn leaf_planes(S) -> insert ->
point_to_plane(S) answers from exactly the caches a caller's would.

Two checks aim at the caches: a second object replays the log and nothing else (the results of its own operations
and the C ABI word aside) and is observed only at the end - its final observation equals the first one's byte for
byte; a third replays it with hints, speculation and bucket history
switched off - leaf_statistics and leaf_planes rows of the same leaves (matched by their cubes: node numbers belong to
one build history) have the same bits (bound 4 of tests/test_gpu_leaf_stats.py).

A failure carries the seed, the index of the operation and the log up to it.
"""

import contextlib
import math

import numpy as np
import pytest

from tests import _opseq as S
from tests._util import assert_same_leaves, set_option

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


# ---- the library behind a log ----------------------------------------------------------------------------------------
class Device:
    def __init__(self, container):
        from octreelib_amd.grid import Grid, GridConfig
        from octreelib_amd.octree import Octree, OctreeConfig
        from octreelib_amd.octree_manager import OctreeManager

        self.c, self.kind = container, container["kind"]
        if self.kind == "grid":
            self.o = Grid(GridConfig(voxel_edge_length=container["edge"]))
        elif self.kind == "manager":
            self.o = OctreeManager(Octree, OctreeConfig(), np.array(container["corner"]), container["edge"])
        else:
            self.o = Octree(OctreeConfig(), np.array(container["corner"]), np.float64(container["edge"]))
        self.f = self.o._forest
        self.poses = []
        self.displaced = False
        self.replaced = False      # a map function replaced the contents: the store is numbered anew, in block order
        self.n_applied = 0         # the index of the next operation: a carve names the ray_evidence it takes by it
        self.evidence = {}
        self.prunes = []           # (index, PruneResult) of every prune: evidence is carried over them by remapped()
        self.checked = None        # a seeded generator on the object that is observed: its prunes check themselves

    def leaves(self, p):
        if self.kind == "grid":
            return self.o.get_leaf_points(p)
        return self.o.get_leaf_points(True, p) if self.kind == "manager" else self.o.get_leaf_points()

    def counters(self, p):
        o = self.o
        if self.kind == "octree":
            return [o.n_nodes, o.n_leaves, o.n_points]
        return [o.n_nodes(p), o.n_leaves(p), o.n_points(p)]

    def leaf_statistics(self, p):
        return self.o.leaf_statistics() if self.kind == "octree" else self.o.leaf_statistics(p)

    def leaf_planes(self, poses):
        return self.o.leaf_planes() if self.kind == "octree" else self.o.leaf_planes(poses)

    def point_to_plane(self, Q, poses, mp, mv):
        if self.kind == "octree":
            return self.o.point_to_plane(Q, mp, mv)
        return self.o.point_to_plane(Q, poses, mp, mv)

    def nearest(self, Q, k, r, poses):
        if self.kind == "octree":
            return self.o.nearest(Q, k, max_distance=r)
        return self.o.nearest(Q, k, max_distance=r, pose_numbers=poses)

    def raycast(self, rays, poses, surface, mp, mv):
        O, D, tmin, tmax = rays
        sel = {} if self.kind == "octree" else {"pose_numbers": poses}
        return self.o.raycast(O, D, tmax, min_range=tmin, surface=surface, min_points=mp, max_variance=mv, **sel)

    def plane_segments(self, poses, **gates):
        return self.o.plane_segments(**gates) if self.kind == "octree" else self.o.plane_segments(poses, **gates)

    def registration_system(self, scan, T, poses, **gates):
        if self.kind == "octree":
            return self.o.registration_system(scan, T, per_point=True, **gates)
        return self.o.registration_system(scan, T, poses, per_point=True, **gates)

    def radius_count(self, Q, r, cap, poses):
        sel = {} if self.kind == "octree" else {"pose_numbers": poses}
        return self.o.radius_count(Q, r, max_count=cap, **sel)

    def point_system(self, scan, T, r, poses, delta, origin):
        sel = {} if self.kind == "octree" else {"pose_numbers": poses}
        return self.o.point_registration_system(scan, T, max_distance=r, huber_delta=delta, origin=origin, per_point=True,
                                                **sel)

    def plane_system(self, scan, T, r, poses, mp, mv, delta, origin):
        from octreelib_amd.matching import nearest_plane_registration_system

        sel = {} if self.kind == "octree" else {"pose_numbers": poses}
        return nearest_plane_registration_system(self.o, scan, T, max_distance=r, min_points=mp, max_variance=mv,
                                                 huber_delta=delta, origin=origin, per_point=True, **sel)

    def name(self, p):
        """The pose column of Neighbours for pose p (an Octree's is 0)."""
        return 0 if self.kind == "octree" else p

    def rays(self, seed, n, max_range, min_range):
        """(origins, directions, min_range (n,), max_range (n,)): origins at jittered stored points, a third of them
        pushed out of the scene; directions random, a quarter axis-parallel, four zero; six dead rays (max_range <
        min_range, a NaN component)."""
        rng = np.random.default_rng([seed, 0x4A7])
        e = S.cloud_edge(self.c)
        xyz = self.f.xyz
        O = (xyz[rng.integers(0, len(xyz), n)] if len(xyz) else np.zeros((n, 3))) + rng.normal(0.0, 0.01 * e, (n, 3))
        O[: n // 3] += rng.uniform(-3.0, 3.0, (n // 3, 3)) * e
        D = rng.normal(size=(n, 3))
        q = n // 4
        D[n // 3: n // 3 + q] = np.eye(3)[rng.integers(0, 3, q)] * rng.choice([-1.0, 1.0], q)[:, None]
        D[-10:-6] = 0.0
        tmin, tmax = np.full(n, float(min_range)), np.full(n, float(max_range))
        tmax[-6:-3] = min_range - 0.5 * e
        O[-3, 1], D[-2, 0], O[-1, 2] = np.nan, np.nan, np.inf
        return np.ascontiguousarray(O), np.ascontiguousarray(D), tmin, tmax

    def scan(self, op):
        """(scan, transform) of a registration_system record: stored points of one pose moved by the record's motion;
        the transform is None or that motion's inverse."""
        from octreelib_amd.registration import transform_np

        lv = self.leaves(op["pose"])
        rows = np.vstack([v.get_points() for v in lv]) if lv else np.empty((0, 3))
        pick = np.random.default_rng([op["seed"], 0x5CA]).permutation(len(rows))[: op["n"]]
        return transform_np(S.motion(op["motion"]), rows[pick]), S.inverse_motion(op["motion"]) if op["inverse"] else None

    def queries(self, seed, n):
        """Stored points jittered, some pushed out of the scene, and the BAD rows of tests/test_gpu_query.py."""
        from tests.test_gpu_query import BAD

        rng = np.random.default_rng([seed, 0x9E21])
        xyz = self.f.xyz
        if len(xyz) == 0:
            return BAD.copy()
        Q = xyz[rng.integers(0, len(xyz), n)] + rng.normal(0.0, 0.01 * S.cloud_edge(self.c), (n, 3))
        Q[: n // 10] += rng.uniform(-3.0, 3.0, (n // 10, 3)) * S.cloud_edge(self.c)
        return np.concatenate([Q, BAD])

    def apply(self, op):
        o, k = self.o, op["op"]
        index, self.n_applied = self.n_applied, self.n_applied + 1
        if k in ("insert", "extend") + S.MOVED:
            cloud = S.make_cloud(op["cloud"])
            how = {}
            if k in S.MOVED:
                how["transform"], how["segment"] = S.moved_args(op, len(cloud))
            if op["cloud"]["form"].startswith("device"):
                from octreelib_amd.feed import DeviceCloud

                cloud = DeviceCloud(cloud)
            o.insert_points(cloud, **how) if self.kind == "octree" else o.insert_points(op["pose"], cloud, **how)
            if k in ("insert", "insert_moved"):
                self.poses.append(op["pose"])
        elif k in ("ray_evidence", "carve"):
            from octreelib_amd.query import RayEvidence

            sel = {} if self.kind == "octree" else {"pose_numbers": op.get("poses")}
            if op.get("evidence_from") is not None:      # what that operation of the log returned
                ev = self.evidence[op["evidence_from"]]
                if op.get("remapped"):      # ... carried over every prune since
                    for at, res in self.prunes:
                        ev = ev.remapped(res) if at > op["evidence_from"] else ev
                return o.carve(ev, op["min_through"], op["max_hits"], **sel)
            O, D, r, returned = S.evidence_rays(op, S.stored_rows(self.f.xyz), float(S.cloud_edge(self.c)))
            args = (O, D, r, op["margin"], op["min_range"], returned)
            if k == "ray_evidence":
                ev = o.ray_evidence(*args)
                self.evidence[index] = RayEvidence(ev.through.copy(), ev.hits.copy())
                return args, ev
            if op["fused"]:
                return o.carve_rays(*args, op["min_through"], op["max_hits"], **sel)
            return o.carve(o.ray_evidence(*args), op["min_through"], op["max_hits"], **sel)
        elif k == "remove_poses":
            left = o.remove_poses(op["poses"])
            for p in set(op["poses"]):
                self.poses.remove(p)      # (the others keep their order: slots are renumbered densely, ascending)
            return left
        elif k == "remove_poses_refused":
            with pytest.raises(KeyError):
                o.remove_poses(op["poses"])
        elif k == "store_size":
            return self.f.store_size()
        elif k == "remove_sparse":
            if self.kind == "octree":
                return o.remove_sparse(op["radius"], op["min_neighbours"])
            return o.remove_sparse(op["radius"], op["min_neighbours"], pose_numbers=op["poses"], among=op["among"])
        elif k == "prune":
            res = o.prune() if self.checked is None else _checked_prune(self, f"operation {index} prune")
            self.prunes.append((index, res))
            return res
        elif k == "radius_count":
            e = float(S.cloud_edge(self.c))
            Q = S.count_queries(op, S.stored_rows(self.f.xyz), e)
            return Q, self.radius_count(Q, op["radius"] * e, op["max_count"], op["poses"])
        elif k in ("point_registration_system", "nearest_plane_registration_system"):
            e = float(S.cloud_edge(self.c))
            scan, T = S.scan_of(op, S.stored_rows(self.f.xyz), e)
            if k == "point_registration_system":
                return scan, T, self.point_system(scan, T, op["max_distance"] * e, op["poses"], op["huber_delta"], op["origin"])
            return scan, T, self.plane_system(scan, T, op["max_distance"] * e, op["poses"], op["min_points"],
                                              op["max_variance"], op["huber_delta"], op["origin"])
        elif k in S.SUBDIVIDES:
            crit = S.build_criteria(op["crit"])
            o.subdivide(crit) if self.kind == "octree" else o.subdivide(crit, op["poses"])
        elif k in S.FILTERS:
            crit = S.build_filter(op["crit"])
            o.filter(crit, op["poses"]) if k == "filter_subset" else o.filter(crit)
        elif k in ("map_select", "map_transform"):
            fn = S.build_map(op["fn"], S.cloud_edge(self.c))
            o.map_leaf_points(fn) if self.kind == "octree" else o.map_leaf_points(fn, op["poses"])
            self.displaced = self.displaced or op["fn"] == "shift_z"
            self.replaced = self.replaced or k == "map_transform"
        elif k == "apply_mask":
            n = self.counters(op["pose"])[2]
            mask = np.random.default_rng([op["seed"], 0x3A5C]).random(n) < op["keep"]
            o.apply_mask(mask) if self.kind == "octree" else o.apply_mask(mask, op["pose"])
        elif k == "ransac":
            np.random.seed(op["np_seed"])
            o.map_leaf_points_cuda_ransac(poses_per_batch=op["ppb"], threshold=op["thr"], hypotheses_number=op["H"],
                                          initial_points_number=6)
        elif k == "leaf_statistics":
            return self.leaf_statistics(op["pose"])
        elif k == "get_leaf_points":
            return self.leaves(op["pose"])
        elif k == "locate":
            Q = self.queries(op["seed"], op["n"])
            return Q, o.locate(Q)
        elif k == "leaf_planes":
            return self.leaf_planes(op["poses"])
        elif k == "point_to_plane":
            Q = self.queries(op["seed"], op["n"])
            return Q, self.point_to_plane(Q, op["poses"], op["min_points"], op["max_variance"])
        elif k in ("transform_poses", "transform_poses_refused"):
            from octreelib_amd import _native as nat

            T = [S.motion(m) for m in op["motions"]]
            if k == "transform_poses":
                o.transform_poses(T, op["poses"])
            else:
                with pytest.raises(nat.DomainError):
                    o.transform_poses(T, op["poses"])
        elif k == "nearest":
            Q = self.queries(op["seed"], op["n"])
            if self.displaced:
                with pytest.raises(RuntimeError):
                    self.nearest(Q, op["k"], op["r"], op["poses"])
                return None
            return Q, self.nearest(Q, op["k"], op["r"], op["poses"])
        elif k == "raycast":
            rays = self.rays(op["seed"], op["n"], op["max_range"], op["min_range"])
            args = (rays, op["poses"], op["surface"], op["min_points"], op["max_variance"])
            if self.displaced:
                with pytest.raises(RuntimeError):
                    self.raycast(*args)
                return None
            hits = self.raycast(*args)
            # (the table `row` names: the mirror's copy of the one the cast was made against, no device call)
            return rays, hits, self.leaf_planes(op["poses"]) if op["surface"] == "plane" else None
        elif k == "plane_segments":
            return self.plane_segments(op["poses"], **{g: op[g] for g in ("min_points", "max_variance", "max_angle", "max_offset")})
        elif k == "registration_system":
            scan, T = self.scan(op)
            gates = {g: op[g] for g in ("min_points", "max_variance", "max_distance", "huber_delta")}
            return scan, T, self.registration_system(scan, T, op["poses"], **gates)
        elif k == "adjustment_system":
            T = None if op["motions"] is None else np.stack([S.motion(m) for m in op["motions"]])
            return T, o.adjustment_system(T, op["poses"], min_points=op["min_points"], min_poses=op["min_poses"],
                                          max_variance=op["max_variance"], leaves=True)
        elif k == "node_cubes":
            return o.node_cubes()
        elif k == "counters":
            return {p: self.counters(p) for p in self.poses}
        elif k == "split_stats":
            return self.f.split_stats()
        else:
            raise KeyError(k)
        return None

    # -- observations ---------------------------------------------------------------------------------------------------
    @staticmethod
    def table(lv):
        """A list of leaves as the canonical leaf list with row digests of Model.observe()."""
        rows = [v.get_points() for v in lv]
        dig = S.leaf_digests(np.vstack(rows) if rows else np.empty((0, 3)), [len(r) for r in rows])
        return [(((np.asarray(v.corner_min, dtype=np.float64) + 0.0).tobytes(), np.float64(v.edge_length).tobytes()), d)
                for v, d in zip(lv, dig)]

    def tables(self):
        """Per pose (canonical leaf list, counters) in the form of Model.observe()."""
        return {p: (self.table(self.leaves(p)), self.counters(p)) for p in self.poses}

    @contextlib.contextmanager
    def neutral(self):
        """Inside, every getter downloads its table NOW; afterwards the forest's host-side caches and its booked
        point count are exactly what they were, so that looking does not change what a later call answers from."""
        f = self.f
        # every host-side cache Forest._invalidate() clears - read off the method itself, so that a cache added there
        # is saved here too - and the booked point count
        probe = object.__new__(type(f))
        type(f)._invalidate(probe)
        names = tuple(vars(probe)) + ("_n_ord", "_n_ord_pending")
        assert {"_nodes", "_voxels", "_blocks", "_order", "_xyz", "_perm", "_slot_blocks", "_counts", "_internal",
                "_pooled"} <= set(names)
        f.ensure_built()      # (a pending insertion is placed first: the build clears the caches itself)
        saved = {n: getattr(f, n) for n in names}
        f._invalidate()
        try:
            yield
        finally:
            for n, v in saved.items():
                setattr(f, n, v)

    def fresh(self):
        """The forest's tables downloaded now, its host-side caches left exactly as they are."""
        f = self.f
        with self.neutral():
            nodes, voxels, blocks = f.nodes, f.voxels, f.blocks
            snap = (tuple(v.tobytes() for v in nodes.values()), tuple(v.tobytes() for v in blocks.values()),
                    f.perm.tobytes(), f.xyz.tobytes(), tuple(f._slot_counts(s) for s in range(f.n_slots)))
        return nodes, voxels, snap

    def final(self):
        """Everything observable, as bytes."""
        from tests.test_gpu_leaf_stats import _stats_bytes

        out = []
        for p in self.poses:
            lv = self.leaves(p)
            out.append([(np.asarray(v.corner_min, dtype=np.float64).tobytes(), np.float64(v.edge_length).tobytes(),
                         v.get_points().tobytes(), v.node) for v in lv])
            out.append(self.counters(p))
            out.append(_stats_bytes(self.leaf_statistics(p)))
        pl = self.leaf_planes(None)
        out.append(_stats_bytes(pl) + (pl.node.tobytes(),))
        cnt, lam = self.f.split_stats()
        out.append((cnt.tobytes(), lam.tobytes()))
        near, hits, seg = self.map_answers()
        if near is not None:
            out.append(tuple(a.tobytes() for a in (near.index, near.pose, near.distance2, near.count)))
            out.append(tuple(a.tobytes() for h in hits for a in (h.node, h.t, h.row)))
        t = seg.segments
        out.append(tuple(np.ascontiguousarray(a).tobytes() for a in (seg.neighbour, seg.label, t.root, t.n_leaves, t.count,
                                                                      t.mean, t.covariance, t.eigenvalues, t.eigenvectors)))
        return out

    def map_answers(self):
        """nearest, raycast (both surfaces) and plane_segments for a fixed set of queries and rays that does not depend
        on the build history: drawn from the stored rows in lexicographic order.  (None, None, segments) once rows
        are displaced."""
        e = S.cloud_edge(self.c)
        seg = self.plane_segments(None, min_points=8, max_variance=1e-3 * e ** 2, max_angle=0.1, max_offset=0.05 * e)
        if self.displaced:
            return None, None, seg
        rows = [v.get_points() for p in self.poses for v in self.leaves(p)]
        U = np.unique(np.vstack(rows), axis=0) if rows else np.zeros((1, 3))
        rng = np.random.default_rng(0xF1A7)
        Q = U[rng.integers(0, len(U), 200)] + rng.normal(0.0, 0.01 * e, (200, 3))
        Q[:20] += rng.uniform(-3.0, 3.0, (20, 3)) * e
        D = rng.normal(size=(200, 3))
        D[:50] = np.eye(3)[rng.integers(0, 3, 50)]
        rays = (Q, D, np.zeros(200), np.full(200, 6.0 * e))
        near = self.nearest(Q, 4, 0.5 * e, None)
        return near, [self.raycast(rays, None, surface, None, None) for surface in ("cube", "plane")], seg

    def map_by_cube(self):
        """map_answers() with everything that belongs to one build history - node ids, plane rows, segment labels -
        named by the leaf's cube instead: nearest as bytes, raycast as (t bytes, cubes hit) per surface, the
        segments as the set of their leaves' cubes and the neighbour table by cube."""
        near, hits, seg = self.map_answers()
        corner, edge = self.o.node_cubes()
        cube = lambda n: None if n < 0 else ((corner[n] + 0.0).tobytes(), float(edge[n]))
        out = {}
        if near is not None:
            # (the numbers of a store that was numbered anew follow the block table: one build history's)
            out["nearest"] = tuple(a.tobytes() for a in ((near.pose, near.distance2, near.count) if self.replaced else
                                                         (near.index, near.pose, near.distance2, near.count)))
            pl = self.leaf_planes(None)
            for surface, h in zip(("cube", "plane"), hits):
                assert np.all((h.row >= 0) == ((h.node >= 0) & (surface == "plane")))
                assert surface == "cube" or np.array_equal(pl.node[h.row[h.row >= 0]], h.node[h.row >= 0])
                out["raycast " + surface] = (h.t.tobytes(), [cube(n) for n in h.node.tolist()])
        ids = seg.planes.node.tolist()
        parts = {}
        for n, lab in zip(ids, seg.label.tolist()):
            if lab >= 0:
                parts.setdefault(lab, []).append(cube(n))
        out["segments"] = sorted(sorted(v) for v in parts.values())
        out["neighbour"] = {cube(n): [cube(b) for b in nb] for n, nb in zip(ids, seg.neighbour.tolist())}
        return out

    def by_cube(self):
        """leaf_statistics and leaf_planes rows keyed by the leaf's cube (node numbers belong to one build history):
        {(pose, corner, edge): (sorted rows, statistics row)}, {(corner, edge): plane row}."""
        from tests.test_gpu_leaf_stats import _row

        stats, planes = {}, {}
        for p in self.poses:
            st = self.leaf_statistics(p)
            for i, v in enumerate(self.leaves(p)):
                key = (p, (np.asarray(v.corner_min, dtype=np.float64) + 0.0).tobytes(), float(v.edge_length))
                stats[key] = (sorted(map(bytes, v.get_points())), _row(st, i))
        pl = self.leaf_planes(None)
        corner, edge = self.o.node_cubes()
        for i, n in enumerate(pl.node.tolist()):
            planes[((corner[n] + 0.0).tobytes(), float(edge[n]))] = _row(pl, i)
        return stats, planes

    def abi_point_to_plane(self):
        from octreelib_amd import _native as nat

        f = self.f
        Q = np.zeros((1, 3))
        node, row, dist = np.empty(1, np.int32), np.empty(1, np.int32), np.empty(1)
        return f.lib.octl_forest_point_to_plane(f.handle, nat.ptr(Q), 1, 8, -1.0, nat.ptr(node), nat.ptr(row),
                                                nat.ptr(dist))


# ---- the checks of one step ----------------------------------------------------------------------------------------
def _check_split_stats(nd, cnt, lam, rec, op):
    """tests/test_gpu_planarity._check_arithmetic against the record the model made of the build."""
    plane = next(s for s in op["crit"] if s[0] == "NotPlanar")
    mv, min_points, ddof = plane[1], plane[2], plane[3]
    K = min((s[1] for s in op["crit"] if s[0] == "MaxPoints"), default=-1)
    keys = [((nd["corner"][i] + 0.0).tobytes(), float(nd["edge"][i])) for i in range(len(cnt))]
    assert set(keys) == set(rec)
    internal = nd["first_child"] >= 0
    for i, k in enumerate(keys):
        e, n, ref, o_internal, c = rec[k]
        assert int(cnt[i]) == n
        if n < min_points:
            assert math.isnan(lam[i])
        else:
            gamma = (math.ceil(c / 64) + math.ceil(c / 4096) + 16) * EPS
            bound = (4 * gamma + 64 * EPS) * 3 * (e / 2) ** 2 * n / (n - ddof)
            assert abs(lam[i] - ref) <= bound, (i, n, e, lam[i], ref, bound)
        want = (K >= 0 and n > K) or (n >= min_points and lam[i] > mv)
        assert bool(internal[i]) == want == o_internal


def _check_point_to_plane(res, planes, Q, node_ref, mp, mv):
    """Rows and NaN rules equal to point_to_plane_np on the returned table, distances within 4 eps sum |n_i d_i| of
    the longdouble value formed from the returned plane."""
    from octreelib_amd.query import point_to_plane_np

    assert res.planes is planes and np.array_equal(res.node, node_ref)
    row_ref, _ = point_to_plane_np(res.node, planes, Q, mp, mv)
    assert np.array_equal(res.row, row_ref)
    ok = res.row >= 0
    assert np.all(np.isnan(res.distance[~ok])) and np.all(np.isfinite(res.distance[ok]))
    nrm = planes.normal[res.row[ok]].astype(np.longdouble)
    terms = nrm * (Q[ok].astype(np.longdouble) - planes.mean[res.row[ok]].astype(np.longdouble))
    assert np.all(np.abs(res.distance[ok].astype(np.longdouble) - terms.sum(axis=1)) <= 4 * EPS * np.abs(terms).sum(axis=1))


def _check_stats_value(seq, i, last_build, nd, cnt, lam):
    stats = seq.meta[i]["stats"]
    if isinstance(stats, dict):
        _check_split_stats(nd, cnt, lam, stats, last_build)
    elif stats == "nan":
        assert len(cnt) == len(nd["edge"]) and not cnt.any() and np.isnan(lam).all()


# ---- the map queries against their definitions, on tables that are downloaded now ----------------------------------------
def _stored(dev, ident):
    """{pose: (rows, index)} of what the forest stores now - call inside Device.neutral(): the rows of every pose
    from the ordered coordinates, index = the row number of each in the cloud as first inserted.  The device's own
    account of it is the permutation (tests/test_gpu_nearest._survivors); where the model keeps one (ident: {pose:
    (index, row hash)} of Sequence.ident) it is the model's, found by the row's bits, and the two must agree."""
    f = dev.f
    xyz, perm = f.xyz, f.perm
    off = np.concatenate([[0], np.cumsum(f.slot_sizes)]).astype(np.int64)
    out = {}
    for s_, p in enumerate(dev.poses):
        mine = (perm >= off[s_]) & (perm < off[s_ + 1])
        rows, index = xyz[mine], perm[mine] - off[s_]
        if ident is not None:
            orig, hsh = ident[p]
            assert len(rows) == len(orig), (p, len(rows), len(orig))
            order = np.argsort(hsh, kind="stable")
            pos = np.minimum(np.searchsorted(hsh[order], S.row_hashes(rows)), max(len(hsh) - 1, 0))
            assert np.array_equal(hsh[order][pos], S.row_hashes(rows)), f"pose {p} stores a row the model does not have"
            assert np.array_equal(orig[order][pos], index), f"pose {p}: the rows' numbers are not the model's"
            index = orig[order][pos]
        a = np.argsort(index, kind="stable")
        out[p] = (np.ascontiguousarray(rows[a]), index[a])
    return out


def _check_nearest(dev, got, Q, k, r, sel, ident, what):
    """nearest_np over the stored rows, bit for bit; its indices mapped to rows of the clouds as first inserted (the
    map is ascending, so the order (d2, slot, index) is the same in both numberings)."""
    from octreelib_amd.query import nearest_np
    from tests.test_gpu_nearest import _assert_equal

    stored = _stored(dev, ident)
    chosen = [p for p in dev.poses if sel is None or p in sel]
    ref = nearest_np(Q, [(dev.name(p), stored[p][0]) for p in chosen], k, max_distance=r)
    index = ref.index.copy()
    for p in chosen:      # (pose numbers are distinct; an Octree has one cloud)
        m = (ref.pose == dev.name(p)) & (ref.index >= 0)
        index[m] = stored[p][1][ref.index[m]]
    ref.index = index
    _assert_equal(got, ref, what)


def _check_raycast(dev, got, rays, sel, surface, mp, mv, planes, what):
    """raycast_np over the leaves the tables downloaded now describe (tests/test_gpu_raycast._leaf_set) and, for the
    plane form, the table the cast was made against, bit for bit."""
    from octreelib_amd.query import normalize_directions, ray_inputs, raycast_np
    from tests._raycast import assert_hits_equal
    from tests.test_gpu_raycast import _leaf_set

    slot_of = {p: s_ for s_, p in enumerate(dev.poses)}
    cube, count = _leaf_set(dev.f, None if sel is None else [slot_of[p] for p in sel])
    O, D, tmin, tmax = rays
    o, dn, tmin, tmax = ray_inputs(O, normalize_directions(D), tmin, tmax)
    ref = raycast_np(o, dn, tmax, *cube, t_min=tmin, count=count, planes=planes, surface=surface, min_points=mp,
                     max_variance=mv)
    assert_hits_equal(got, ref, what)


def _check_pooled(dev, planes, sel, leaves, what):
    """A pooled table against the leaves downloaded now (tests/test_gpu_query._check_planes)."""
    from tests.test_gpu_query import _check_planes

    chosen = dev.poses if sel is None else sel
    slot_of = {p: s_ for s_, p in enumerate(dev.poses)}
    pose_of = {s_: p for p, s_ in slot_of.items()}
    if any(leaves[p] for p in chosen):
        _check_planes(dev.o, dev.f, planes, sorted(slot_of[p] for p in chosen), lambda s_: leaves[pose_of[s_]], what)
    else:
        assert len(planes) == 0


def _check_segments(dev, got, sel, gates, nodes, voxels, leaves, what):
    from octreelib_amd.query import plane_segments_np
    from tests.test_cpu_segments import table_error_over_bound
    from tests.test_gpu_segments import _assert_equal

    _check_pooled(dev, got.planes, sel, leaves, what)
    ref = plane_segments_np(got.planes, nodes, voxels, dev.f.mode, dev.f._cube[1], gates["min_points"],
                            gates["max_variance"], gates["max_angle"], gates["max_offset"])
    _assert_equal(got, ref, what)
    assert table_error_over_bound(got) <= 1.0, what


def _check_registration(dev, scan, T, s, op, nodes, voxels, leaves, what):
    from octreelib_amd.query import PointToPlane, locate_np
    from octreelib_amd.registration import default_origin, transform_np
    from tests.test_gpu_registration import _check_contract

    _check_pooled(dev, s.planes, op["poses"], leaves, what)
    moved = transform_np(T, scan)
    node = locate_np(nodes, voxels, dev.f.mode, dev.f._cube[1], moved)
    _check_point_to_plane(PointToPlane(s.node, s.row, s.residual, s.planes), s.planes, moved, node, op["min_points"],
                          op["max_variance"])
    assert np.array_equal(s.origin, default_origin(T, scan)), what
    _check_contract(s, scan, T, s.origin, what, max_distance=op["max_distance"], huber_delta=op["huber_delta"])


def _check_adjustment(dev, T, s, op, leaves, what):
    """The block table is that of the leaves downloaded now - counts exactly, moments within the bound of
    tests/test_gpu_adjustment.py::test_block_moments - and the sums are within _check_system's bound of the
    definition on it."""
    from octreelib_amd.adjustment import block_moments_np
    from tests.test_gpu_adjustment import _check_system

    from octreelib_amd.adjustment import root_box_centre

    LD = np.longdouble
    chosen = [p for p in dev.poses if op["poses"] is None or p in op["poses"]]
    assert list(s.pose_numbers) == chosen, (what, s.pose_numbers)
    nd = dev.f.nodes
    # (no record gives an origin: the default one is the centre of the root cubes that exist NOW - it follows a prune)
    roots = nd["depth"] == 0
    assert np.array_equal(s.origin, root_box_centre(nd["corner"][roots], nd["edge"][roots])), (what, s.origin)
    rows = [(v.node, k, nd["corner"][v.node] + nd["edge"][v.node] / 2.0, v.get_points())
            for k, p in enumerate(chosen) for v in leaves[p]]
    own = block_moments_np(rows, chosen, None, dtype=LD)
    bm = s.blocks
    assert np.array_equal(bm.node, own.node) and np.array_equal(bm.pose, own.pose) and np.array_equal(bm.count, own.count), what
    assert np.array_equal(bm.anchor, own.anchor), what
    points = {(int(n), int(k)): x for n, k, _, x in rows if len(x)}
    for i in range(len(bm)):
        d = points[(int(bm.node[i]), int(bm.pose[i]))].astype(LD) - bm.anchor[i].astype(LD)
        n, R = len(d), float(np.abs(d).max())
        gamma = (-(-n // 64) + -(-n // 4096) + 1 + 16) * EPS
        assert np.all(np.abs(bm.s[i].astype(LD) - own.s[i]) <= 2 * gamma * R * n), (what, i)
        assert np.all(np.abs(bm.M[i].astype(LD) - own.M[i]) <= 4 * gamma * R * R * n), (what, i)
    gates = {"min_points": op["min_points"], "min_poses": op["min_poses"]}
    if op["max_variance"] is not None:
        gates["max_variance"] = op["max_variance"]
    _check_system(s, T, s.origin, what, **gates)


# ---- the fourth generation -------------------------------------------------------------------------------------------
def _indexable(dev, stored, sel):
    """[(name, rows)] of the selected poses in slot order, rows[i] = row i of the pose's cloud as first inserted (NaN
    where it has left): what Neighbours.index refers to.  stored: _stored()."""
    out = []
    for p in dev.poses:
        if sel is None or p in sel:
            rows, index = stored[p]
            full = np.full((int(index.max()) + 1 if len(index) else 0, 3), np.nan)
            full[index] = rows
            out.append((dev.name(p), full))
    return out


def _check_radius_count(dev, got, Q, r, cap, sel, ident, what):
    """radius_count_np on the rows downloaded now, count for count - call inside Device.neutral()."""
    from octreelib_amd.query import radius_count_np

    stored = _stored(dev, ident)
    ref = radius_count_np(Q, [(dev.name(p), stored[p][0]) for p in dev.poses if sel is None or p in sel], r, max_count=cap)
    assert got.dtype == ref.dtype == np.int32 and np.array_equal(got, ref), (what, np.nonzero(got != ref)[0][:8])


def _check_origin(s, scan, T, origin, what):
    from octreelib_amd.registration import default_origin

    want = default_origin(T, scan) if origin is None else np.asarray(origin, dtype=np.float64)
    assert np.array_equal(s.origin, want), (what, s.origin, want)


def _check_point_system(dev, s, scan, T, r, sel, delta, origin, ident, what):
    """point_registration_system - call inside Device.neutral(): .neighbours is nearest_np(k = 1) on the rows
    downloaded now, bit for bit, its index by the model's bookkeeping; the sums are under _check_sums of
    tests/test_gpu_point_registration.py."""
    from octreelib_amd.registration import transform_np
    from tests.test_gpu_point_registration import _check_sums

    _check_nearest(dev, s.neighbours, transform_np(T, scan), 1, r, sel, ident, what)
    _check_origin(s, scan, T, origin, what)
    _check_sums(s, _indexable(dev, _stored(dev, ident), sel), scan, T, s.origin, delta, what)


def _check_plane_system(dev, s, scan, T, r, sel, delta, origin, leaves, ident, what):
    """nearest_plane_registration_system, the part that needs tables downloaded now - call inside Device.neutral():
    the correspondences are nearest_np's, .planes is under _check_pooled, the sums under _check_sums of
    tests/test_gpu_nearest_plane_registration.py.  Returns what Neighbours.index refers to, for _check_per_point."""
    from octreelib_amd.registration import transform_np
    from tests.test_gpu_nearest_plane_registration import _check_sums

    _check_nearest(dev, s.neighbours, transform_np(T, scan), 1, r, sel, ident, what)
    _check_pooled(dev, s.planes, sel, leaves, what)
    _check_origin(s, scan, T, origin, what)
    _check_sums(s, scan, T, s.origin, delta, what)
    return _indexable(dev, _stored(dev, ident), sel)


def _check_per_point(dev, s, clouds, scan, T, r, sel, mp, mv, what):
    """The per-point contract of tests/test_gpu_nearest_plane_registration.py, against the map's own nearest, locate,
    leaf_planes and point_to_plane over the same selection - call outside Device.neutral(): .planes must BE the
    table leaf_planes hands out."""
    from tests.test_gpu_nearest_plane_registration import _check_per_point as check

    check(dev.o, s, clouds, scan, T, r, sel, mp, mv, what)


def _pose_reads(dev):
    """What every pose reads back and a prune must not change: its rows, the leaf and point counters, the non-empty
    leaves with their rows, the statistics (or the kind of refusal)."""
    from tests.test_gpu_leaf_stats import _stats_bytes

    out = []
    for p in dev.poses:
        try:
            stats = _stats_bytes(dev.leaf_statistics(p))
        except Exception as e:   # noqa: BLE001
            stats = type(e).__name__
        pts = dev.o.get_points() if dev.kind == "octree" else dev.o.get_points(p)
        out.append((pts.tobytes(), dev.counters(p)[1:], stats,
                    [(np.asarray(v.corner_min, dtype=np.float64).tobytes(), np.float64(v.edge_length).tobytes(),
                      v.get_points().tobytes()) for v in dev.leaves(p)]))
    return out


def _checked_prune(dev, what):
    """prune() on the object that is observed, with the checks of tests/test_gpu_prune.py on the state the log has
    reached: the tables after are prune_np of the tables before (_prune_and_check), every map query before equals
    the query after through node_map (_queries, _queries_equal - with queries and rays of this scene's extent), and
    every pose reads back the same rows, leaves and statistics."""
    from tests.test_gpu_prune import _prune_and_check, _queries, _queries_equal

    rng, e = dev.checked, float(S.cloud_edge(dev.c))
    stored = S.stored_rows(dev.f.xyz)
    O, D, R, _ = S.evidence_rays({"seed": int(rng.integers(1 << 30)), "n": 150, "margin": 0.05 * e, "min_range": 0.0},
                                 stored, e)
    Q = S.count_queries({"seed": int(rng.integers(1 << 30)), "n": 300}, stored, e)[:-6]      # (the finite ones)
    scene = {"queries": Q, "origins": O, "directions": D, "ranges": R, "margin": 0.05 * e, "max_range": 6.0 * e,
             "radius": 0.3 * e, "max_variance": 1e-2 * e * e, "origin": S.UTM if dev.c["utm"] else np.zeros(3)}
    nodes_before = {k: v.copy() for k, v in dev.f.nodes.items()}
    before, reads = _queries(dev.o, scene), _pose_reads(dev)
    res, _, _ = _prune_and_check(dev.o, what, expect_change=False)
    _queries_equal(before, _queries(dev.o, scene), res, nodes_before, dev.o, what, scene)
    for n, (x, y) in enumerate(zip(reads, _pose_reads(dev))):
        assert x == y, f"{what}: pose {dev.poses[n]} reads back something else"
    return res


def _check_result(dev, seq, i, op, res, last_build):
    """What the log's own read-only operation returned - from whatever cache it answered - against tables that are
    downloaded now, with the same contracts as the battery below."""
    from octreelib_amd.query import locate_np
    from tests.test_gpu_leaf_stats import _assert_eigen, _assert_matches_leaves
    from tests.test_gpu_query import _check_planes

    k, f = op["op"], dev.f
    if k in ("carve", "remove_poses", "store_size", "remove_sparse"):      # the rows that left / the library's own count, by the model's book
        assert res == seq.meta[i]["returns"], (k, res, seq.meta[i]["returns"])
        return
    if k == "prune":      # the result's five numbers are those of the model's own trees
        got = (res.n_nodes, res.n_voxels, res.nodes_dropped, res.voxels_dropped, res.collapsed)
        assert got == seq.meta[i]["returns"], (k, got, seq.meta[i]["returns"])
        return
    if k not in S.ALL_READ_ONLY or (res is None and k in ("nearest", "raycast")):      # (refused: rows are displaced)
        return
    what = f"operation {i} {k}"
    e, clouds = float(S.cloud_edge(dev.c)), None
    with dev.neutral():
        nodes, voxels = f.nodes, f.voxels
        leaves = {p: dev.leaves(p) for p in dev.poses}
        want = seq.obs[i]
        for p in dev.poses:      # (the reference data itself)
            assert_same_leaves(dev.table(leaves[p]), want[p][0])
        if k == "leaf_statistics":
            _assert_matches_leaves(res, leaves[op["pose"]], f"pose {op['pose']}")
            _assert_eigen(res.eigenvalues, res.eigenvectors, res.covariance)
        elif k == "get_leaf_points":
            assert_same_leaves(dev.table(res), want[op["pose"]][0])
            assert [v.node for v in res] == [v.node for v in leaves[op["pose"]]]
        elif k == "counters":
            assert res == {p: want[p][1] for p in dev.poses}, res
        elif k == "node_cubes":
            assert np.array_equal(res[0], nodes["corner"]) and np.array_equal(res[1], nodes["edge"])
        elif k == "split_stats":
            _check_stats_value(seq, i, last_build, nodes, *res)
        elif k == "locate":
            Q, got = res
            assert got.dtype == np.int32 and np.array_equal(got, locate_np(nodes, voxels, f.mode, f._cube[1], Q))
        elif k == "ray_evidence":
            from octreelib_amd.query import evidence_inputs
            from tests._evidence import assert_evidence_equal, evidence_of_nodes

            assert_evidence_equal(res[1], evidence_of_nodes(nodes, *evidence_inputs(*res[0])), what)
        elif k == "nearest":
            _check_nearest(dev, res[1], res[0], op["k"], op["r"], op["poses"], seq.ident[i], what)
        elif k == "raycast":
            rays, hits, planes = res
            if planes is not None:
                _check_pooled(dev, planes, op["poses"], leaves, what)
            _check_raycast(dev, hits, rays, op["poses"], op["surface"], op["min_points"], op["max_variance"], planes, what)
        elif k == "plane_segments":
            _check_segments(dev, res, op["poses"], op, nodes, voxels, leaves, what)
        elif k == "registration_system":
            _check_registration(dev, *res, op, nodes, voxels, leaves, what)
        elif k == "adjustment_system":
            _check_adjustment(dev, *res, op, leaves, what)
        elif k == "radius_count":
            assert np.array_equal(res[1], seq.meta[i]["returns"]), (what, "the model counts otherwise")
            _check_radius_count(dev, res[1], res[0], op["radius"] * e, op["max_count"], op["poses"], seq.ident[i], what)
        elif k == "point_registration_system":
            scan, T, s = res
            _check_point_system(dev, s, scan, T, op["max_distance"] * e, op["poses"], op["huber_delta"], op["origin"],
                                seq.ident[i], what)
            assert (s.n_used, s.n_located) == seq.meta[i]["returns"], (what, s.n_used, s.n_located, seq.meta[i]["returns"])
        elif k == "nearest_plane_registration_system":
            scan, T, s = res
            clouds = _check_plane_system(dev, s, scan, T, op["max_distance"] * e, op["poses"], op["huber_delta"],
                                         op["origin"], leaves, seq.ident[i], what)
            located, used = seq.meta[i]["returns"]
            assert s.n_located == located and used in (None, s.n_used), (what, s.n_used, s.n_located, seq.meta[i]["returns"])
        else:
            Q, r = res if k == "point_to_plane" else (None, None)
            planes = r.planes if k == "point_to_plane" else res
            chosen = dev.poses if op["poses"] is None else op["poses"]
            slot_of = {p: s for s, p in enumerate(dev.poses)}
            pose_of = {s: p for p, s in slot_of.items()}
            if any(leaves[p] for p in chosen):
                _check_planes(dev.o, f, planes, sorted(slot_of[p] for p in chosen), lambda s: leaves[pose_of[s]],
                              f"operation {i} {op['poses']}")
            else:
                assert len(planes) == 0
            if k == "point_to_plane":
                _check_point_to_plane(r, planes, Q, locate_np(nodes, voxels, f.mode, f._cube[1], Q), op["min_points"],
                                      op["max_variance"])
    if clouds is not None:      # (with the host-side caches back in place: .planes is the table leaf_planes hands out)
        scan, T, s = res
        _check_per_point(dev, s, clouds, scan, T, op["max_distance"] * e, op["poses"], op["min_points"], op["max_variance"], what)


def _check_map_queries(dev, rng, displaced, sels, leaves, Q, ident):
    """The battery's map queries: one nearest, one raycast per surface, one plane_segments per pose selection, each
    against its definition on tables downloaded afterwards."""
    e = S.cloud_edge(dev.c)
    sel = sels[-1]
    k, r = int(rng.choice([1, 3, 8])), float(rng.choice([0.05, 0.5, 2.0])) * e
    ray_seed = int(rng.integers(1 << 30))
    rays = dev.rays(ray_seed, 150, float(rng.uniform(0.5, 8.0)) * e, [0.0, 0.1 * e][int(rng.integers(0, 2))])
    mp, mv = int(rng.choice([1, 8])), [None, 1e-3 * e ** 2][int(rng.integers(0, 2))]
    gates = {"min_points": int(rng.choice([8, 16])), "max_variance": mv, "max_angle": float(rng.choice([0.1, 0.3])),
             "max_offset": float(rng.choice([0.05, 0.02])) * e}
    # one radius_count and one of each nearest-point registration system: 48 of the queries (with the rows no query
    # may answer for the count, without them as the scan), drawn behind the others so that those stay what they were
    rng4 = np.random.default_rng([ray_seed, 0x4E4])
    cap, delta = [None, 1, 3, 7][int(rng4.integers(0, 4))], [None, 0.02 * e][int(rng4.integers(0, 2))]
    scan = np.ascontiguousarray(Q[-54:-6])
    T = S.motion({"xi": [float(x) for x in rng4.uniform(-1.0, 1.0, 6) * ([0.02] * 3 + [0.05 * e] * 3)],
                  "origin": [float(x) for x in (S.UTM if dev.c["utm"] else np.zeros(3))]})
    if displaced:      # (the ones that must refuse; the error word moves with them, so the caller reads it afterwards)
        with pytest.raises(RuntimeError):
            dev.nearest(Q[-150:], k, r, sel)
        for surface in ("cube", "plane"):
            with pytest.raises(RuntimeError):
                dev.raycast(rays, sel, surface, mp, mv)
        with pytest.raises(RuntimeError):
            dev.radius_count(Q[-54:], r, cap, sel)
        with pytest.raises(RuntimeError):
            dev.point_system(scan, T, r, sel, delta, None)
        with pytest.raises(RuntimeError):
            dev.plane_system(scan, T, r, sel, mp, mv, delta, None)
        return
    near = dev.nearest(Q[-150:], k, r, sel)
    hits = {}
    for surface in ("cube", "plane"):
        got = dev.raycast(rays, sel, surface, mp, mv)
        hits[surface] = (got, dev.leaf_planes(sel) if surface == "plane" else None)
    segments = [(x, dev.plane_segments(x, **gates)) for x in sels]
    # (last: the pooled table the plane form returns is still the one leaf_planes hands out when it is checked)
    counts = dev.radius_count(Q[-54:], r, cap, sel)
    ps = dev.point_system(scan, T, r, sel, delta, None)
    ns = dev.plane_system(scan, T, r, sel, mp, mv, delta, None)
    with dev.neutral():
        nodes, voxels = dev.f.nodes, dev.f.voxels
        _check_nearest(dev, near, Q[-150:], k, r, sel, ident, f"nearest {sel}")
        for surface, (got, planes) in hits.items():
            if planes is not None:
                _check_pooled(dev, planes, sel, leaves, f"raycast {surface} {sel}")
            _check_raycast(dev, got, rays, sel, surface, mp, mv, planes, f"raycast {surface} {sel}")
        for x, got in segments:
            _check_segments(dev, got, x, gates, nodes, voxels, leaves, f"plane_segments {x}")
        _check_radius_count(dev, counts, Q[-54:], r, cap, sel, ident, f"radius_count {sel}")
        _check_point_system(dev, ps, scan, T, r, sel, delta, None, ident, f"point_registration_system {sel}")
        clouds = _check_plane_system(dev, ns, scan, T, r, sel, delta, None, leaves, ident,
                                     f"nearest_plane_registration_system {sel}")
    _check_per_point(dev, ns, clouds, scan, T, r, sel, mp, mv, f"nearest_plane_registration_system {sel}")


def _check_queries(dev, rng, displaced, ident=None):
    from octreelib_amd.query import locate_np
    from tests.test_gpu_leaf_stats import _assert_eigen, _assert_matches_leaves
    from tests.test_gpu_query import BAD, _check_planes

    f, o = dev.f, dev.o
    nodes, voxels, snap = dev.fresh()
    if displaced:
        _check_map_queries(dev, rng, True, [None], None, dev.queries(int(rng.integers(1 << 30)), 400), ident)
    err = f.lib.octl_last_error(f.ctx.handle)
    # locate: jittered stored points, points on splitting planes, the BAD rows
    Q = dev.queries(int(rng.integers(1 << 30)), 400)
    internal = np.nonzero(nodes["first_child"] >= 0)[0]
    if len(internal):
        pick = internal[rng.integers(0, len(internal), 100)]
        half = (nodes["edge"][pick] / 2.0)[:, None]
        centres = nodes["corner"][pick] + half
        Q = np.concatenate([centres, centres + half * [0.5, 0.0, 0.25], nodes["corner"][pick], Q])
    got = o.locate(Q)
    assert got.dtype == np.int32 and np.array_equal(got, locate_np(nodes, voxels, f.mode, f._cube[1], Q))
    assert np.all(got[-len(BAD):] == -1)
    leaves = {p: dev.leaves(p) for p in dev.poses}
    if not displaced:
        for lv in leaves.values():
            if lv:
                rows = np.vstack([v.get_points() for v in lv])
                want = np.repeat([v.node for v in lv], [v.n_points for v in lv])
                assert np.array_equal(o.locate(rows), want)
    slot_of = {p: s for s, p in enumerate(dev.poses)}
    total = sum(v.n_points for lv in leaves.values() for v in lv)
    sels = [None]
    if dev.kind != "octree" and len(dev.poses) > 1:
        sels.append(sorted(int(p) for p in rng.choice(dev.poses, int(rng.integers(1, len(dev.poses))), replace=False)))
    for sel in sels:
        chosen = dev.poses if sel is None else sel
        if not any(leaves[p] for p in chosen):
            continue
        planes = dev.leaf_planes(sel)
        pose_of = {s: p for p, s in slot_of.items()}
        _check_planes(o, f, planes, sorted(slot_of[p] for p in chosen), lambda s: leaves[pose_of[s]], str(sel))
        mp, mv = int(rng.choice([1, 8])), [None, 1e-3 * S.cloud_edge(dev.c) ** 2][int(rng.integers(0, 2))]
        _check_point_to_plane(dev.point_to_plane(Q, sel, mp, mv), planes, Q, got, mp, mv)
    for p in dev.poses:
        st = dev.leaf_statistics(p)
        _assert_matches_leaves(st, leaves[p], f"pose {p}")
        _assert_eigen(st.eigenvalues, st.eigenvectors, st.covariance)
    o.node_cubes()
    assert total == sum(dev.counters(p)[2] for p in dev.poses)
    if not displaced:
        _check_map_queries(dev, rng, False, sels, leaves, Q, ident)
    # read-only: nothing moved, the error word did not move
    assert dev.fresh()[2] == snap
    assert f.lib.octl_last_error(f.ctx.handle) == err


def _read_back(dev, poses, sel, Q, rays):
    """Everything the given poses read back, and what the map answers over the selection `sel`, as bytes."""
    from tests.test_gpu_leaf_stats import _stats_bytes

    def attempt(fn):      # (the answer or the kind of refusal: the same before and after)
        try:
            return fn()
        except Exception as e:   # noqa: BLE001
            return type(e).__name__

    out = []
    for p in poses:
        lv = dev.leaves(p)
        out.append((dev.o.get_points(p).tobytes(), dev.counters(p), attempt(lambda: _stats_bytes(dev.leaf_statistics(p))),
                    [(np.asarray(v.corner_min, dtype=np.float64).tobytes(), np.float64(v.edge_length).tobytes(), v.node,
                      v.get_points().tobytes()) for v in lv]))

    def planes():
        pl = dev.leaf_planes(sel)
        return _stats_bytes(pl) + (pl.node.tobytes(),)

    def near():
        nn = dev.nearest(Q, 4, 0.5 * S.cloud_edge(dev.c), sel)
        return tuple(a.tobytes() for a in (nn.index, nn.pose, nn.distance2, nn.count))

    def cast():
        h = dev.raycast(rays, sel, "cube", None, None)
        return tuple(a.tobytes() for a in (h.node, h.t, h.row))

    return out + [attempt(planes), attempt(near), attempt(cast)]


def _check_moved(dev, op):
    """What an insert under a transform stored is transform_rows_np of the cloud as given, bit for bit, whatever form
    the cloud was given in (the order is the leaves'; the rows of a pose are distinct)."""
    from octreelib_amd.registration import transform_rows_np

    cloud = S.make_cloud(op["cloud"])
    T, segment = S.moved_args(op, len(cloud))
    want = sorted(map(bytes, transform_rows_np(T, cloud, segment)))
    got = sorted(map(bytes, dev.o.get_points() if dev.kind == "octree" else dev.o.get_points(op["pose"])))
    if op["op"] == "insert_moved":
        assert got == want, "the stored rows are not transform_rows_np of the cloud"
    else:
        assert set(want) <= set(got), "the appended rows are not transform_rows_np of the cloud"


def _replay(seq, observe):
    from octreelib_amd import _native as nat

    dev = Device(seq.container)
    rng = np.random.default_rng([seq.seed, 0x0B5])
    if observe:
        dev.checked = np.random.default_rng([seq.seed, 0x9B4])
    displaced = False
    last_build = None
    for i, op in enumerate(seq.log):
        try:
            before = None
            if observe and op["op"] == "remove_poses":
                # the commit's own contract on a drawn state: what the remaining poses read back, and a query over
                # them, directly before ...
                stay = [p for p in dev.poses if p not in op["poses"]]
                Q = dev.queries(int(rng.integers(1 << 30)), 200)
                rays = dev.rays(int(rng.integers(1 << 30)), 150, 6.0 * S.cloud_edge(dev.c), 0.0)
                before = _read_back(dev, stay, stay, Q, rays)
            if observe and op["op"] == "remove_sparse":
                # what the poses that are not judged read back, and the map's answers over them: the same bytes after
                stay = [] if op["poses"] is None else [p for p in dev.poses if p not in op["poses"]]
                Q = dev.queries(int(rng.integers(1 << 30)), 200)
                rays = dev.rays(int(rng.integers(1 << 30)), 150, 6.0 * S.cloud_edge(dev.c), 0.0)
                before = _read_back(dev, stay, stay, Q, rays) if stay else None
            if observe and op["op"] in S.GEN3_READ_ONLY + S.GEN4_READ_ONLY:
                before = (dev.fresh()[2], dev.f.lib.octl_last_error(dev.f.ctx.handle))
            res = dev.apply(op)
            if observe and op["op"] == "remove_sparse" and before is not None:
                for n, (x, y) in enumerate(zip(before, _read_back(dev, stay, stay, Q, rays))):
                    assert x == y, f"remove_sparse changed item {n} of what the poses {stay} it does not judge read back"
            if observe and op["op"] == "remove_poses":      # ... and the same calls over every pose directly after
                assert dev.poses == stay
                after = _read_back(dev, stay, None, Q, rays)
                for n, (x, y) in enumerate(zip(before, after)):
                    assert x == y, f"remove_poses changed item {n} of what the remaining poses {stay} read back"
            if observe and op["op"] in S.GEN3_READ_ONLY + S.GEN4_READ_ONLY:      # read-only, the error word included
                assert (dev.fresh()[2], dev.f.lib.octl_last_error(dev.f.ctx.handle)) == before
            if observe and op["op"] in S.MOVED:
                _check_moved(dev, op)
            if op["op"] in S.SUBDIVIDES:
                last_build = op
            displaced = displaced or op.get("fn") == "shift_z"
            _check_result(dev, seq, i, op, res, last_build)
            if not observe:
                # the C ABI on the object nobody looks at: stale exactly when the model says so
                rc = dev.abi_point_to_plane()
                assert rc == (0 if seq.meta[i]["pooled"] else nat.OCTL_E_STATE), rc
                continue
            got, want = dev.tables(), seq.obs[i]
            assert list(got) == list(want)
            for p in got:
                assert_same_leaves(got[p][0], want[p][0])
                assert got[p][1] == want[p][1], (p, got[p][1], want[p][1])
            _check_stats_value(seq, i, last_build, dev.f.nodes, *dev.f.split_stats())
            _check_queries(dev, rng, displaced, None if seq.ident is None else seq.ident[i])
        except Exception as e:      # (a library error is the likeliest symptom of a stale cache: it carries the log too)
            raise AssertionError(f"operation {i} ({'observed' if observe else 'log-only'} object): "
                                 f"{type(e).__name__}: {e}\n{seq.printed(i)}") from e
    return dev


@pytest.mark.parametrize("seed", S.SEEDS + S.SEEDS2 + S.SEEDS3 + S.SEEDS4)
def test_random_operation_sequences_vs_model(seed):
    seq = S.generate(seed)
    a = _replay(seq, observe=True)
    b = _replay(seq, observe=False)
    fa, fb = a.final(), b.final()
    for k, (x, y) in enumerate(zip(fa, fb)):
        assert x == y, f"observation order matters: final item {k} differs\n{seq.printed()}"
    # history: hints, speculation and bucket history off - the same bits for the same leaves
    for name in ("NO_GEOM_HINT", "NO_SPEC_FINISH", "NO_BUCKET_HISTORY"):
        set_option(name, 1)
    c = Device(seq.container)
    for op in seq.log:
        c.apply(op)
    (sa, pa), (sc, pc) = a.by_cube(), c.by_cube()
    assert list(sa) == list(sc), f"history changes the leaves or their order\n{seq.printed()}"
    for key in sa:
        assert sa[key][0] == sc[key][0], f"history changes the points of a leaf\n{seq.printed()}"
        assert sa[key][1] == sc[key][1], f"history changes the statistics of pose {key[0]}'s leaf {key[1:]}\n{seq.printed()}"
    assert pa == pc, f"history changes the pooled planes\n{seq.printed()}"
    ma, mc = a.map_by_cube(), c.map_by_cube()
    for key in ma:
        assert ma[key] == mc[key], f"history changes {key}\n{seq.printed()}"
