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
        if k in ("insert", "extend"):
            cloud = S.make_cloud(op["cloud"])
            o.insert_points(cloud) if self.kind == "octree" else o.insert_points(op["pose"], cloud)
            if k == "insert":
                self.poses.append(op["pose"])
        elif k in S.SUBDIVIDES:
            crit = S.build_criteria(op["crit"])
            o.subdivide(crit) if self.kind == "octree" else o.subdivide(crit, op["poses"])
        elif k in S.FILTERS:
            crit = S.build_filter(op["crit"])
            o.filter(crit, op["poses"]) if k == "filter_subset" else o.filter(crit)
        elif k in ("map_select", "map_transform"):
            fn = S.build_map(op["fn"], S.cloud_edge(self.c))
            o.map_leaf_points(fn) if self.kind == "octree" else o.map_leaf_points(fn, op["poses"])
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
        names = ("_nodes", "_voxels", "_blocks", "_order", "_xyz", "_perm", "_slot_blocks", "_counts", "_internal",
                 "_pooled", "_n_ord", "_n_ord_pending")
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


def _check_result(dev, seq, i, op, res, last_build):
    """What the log's own read-only operation returned - from whatever cache it answered - against tables that are
    downloaded now, with the same contracts as the battery below."""
    from octreelib_amd.query import locate_np
    from tests.test_gpu_leaf_stats import _assert_eigen, _assert_matches_leaves
    from tests.test_gpu_query import _check_planes

    k, f = op["op"], dev.f
    if k not in S.READ_ONLY:
        return
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


def _check_queries(dev, rng, displaced):
    from octreelib_amd.query import locate_np
    from tests.test_gpu_leaf_stats import _assert_eigen, _assert_matches_leaves
    from tests.test_gpu_query import BAD, _check_planes

    f, o = dev.f, dev.o
    nodes, voxels, snap = dev.fresh()
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
    # read-only: nothing moved, the error word did not move
    assert dev.fresh()[2] == snap
    assert f.lib.octl_last_error(f.ctx.handle) == err


def _replay(seq, observe):
    from octreelib_amd import _native as nat

    dev = Device(seq.container)
    rng = np.random.default_rng([seq.seed, 0x0B5])
    displaced = False
    last_build = None
    for i, op in enumerate(seq.log):
        try:
            res = dev.apply(op)
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
            _check_queries(dev, rng, displaced)
        except Exception as e:      # (a library error is the likeliest symptom of a stale cache: it carries the log too)
            raise AssertionError(f"operation {i} ({'observed' if observe else 'log-only'} object): "
                                 f"{type(e).__name__}: {e}\n{seq.printed(i)}") from e
    return dev


@pytest.mark.parametrize("seed", S.SEEDS)
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
