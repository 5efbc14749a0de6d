"""Euclidean clusters on the device: octl_forest_cluster_points / octl_forest_remove_small_clusters and
octreelib_amd.cluster / remove_small_clusters over a Grid, an OctreeManager and an Octree.

The contract: the answer consists of integers only - labels, sizes and first members EQUAL
cluster_labels_np over the rows that are still in the map, and the rows remove_small_clusters keeps EQUAL
small_cluster_keep_np - whatever the subdivision, the layout of the ordered arrays or the schedule of the lanes.  The
shapes are the smallest at which the kernels can still go wrong: maps of at most 20 k points."""

import ctypes as C

import numpy as np
import pytest

from octreelib_amd import MaxPoints, synthetic
from octreelib_amd import _native as nat
from octreelib_amd.clustering import Clusters, cluster, cluster_labels_np, remove_small_clusters, small_cluster_keep_np
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree_manager import OctreeManager
from tests._cell import lattice01, ulp_neighbours
from tests._cluster import CHAIN_RADIUS, diagonal_chain
from tests.test_gpu_neighbourhood import _alive
from tests.test_gpu_query import _counter

pytestmark = pytest.mark.gpu


# ---- helpers -------------------------------------------------------------------------------------------------------
def _grid(clouds, K, L=1):
    g = Grid(GridConfig(voxel_edge_length=L))
    for p, P in clouds.items():
        g.insert_points(p, np.ascontiguousarray(P))
    g.subdivide([MaxPoints(K)])
    return g


def _manager(clouds, K, corner, edge):
    m = OctreeManager(Octree, OctreeConfig(), np.asarray(corner, dtype=np.float64), edge)
    for p, P in clouds.items():
        m.insert_points(p, np.ascontiguousarray(P))
    m.subdivide([MaxPoints(K)])
    return m


def _octree(P, K, corner, edge):
    t = Octree(OctreeConfig(), np.asarray(corner, dtype=np.float64), edge)
    t.insert_points(np.ascontiguousarray(P))
    t.subdivide([MaxPoints(K)])
    return t


def _check(obj, clouds, r, what, pose_numbers=None, lo=1, hi=None):
    """cluster() of `obj` against the definition over the rows of `clouds` ({pose: cloud as inserted}) that are still in
    the ordered arrays: rows, (pose, index), labels, sizes, first members - all exact.  Returns the Clusters."""
    octree = isinstance(obj, Octree)
    alive = _alive(obj, clouds)
    chosen = [p for p in alive if pose_numbers is None or p in pose_numbers]
    listed = [(p, np.asarray(clouds[p])[alive[p]]) for p in chosen]
    assert sum(len(c) for _, c in listed) <= 20000, what
    kw = {} if octree else {"pose_numbers": pose_numbers}
    cl = cluster(obj, r, min_points=lo, max_points=hi, **kw)
    labels, sizes, first = cluster_labels_np(listed, r, lo, hi)
    assert isinstance(cl, Clusters) and cl.pose.dtype == np.int32 and cl.index.dtype == np.int32, what
    assert cl.label.dtype == np.int32 and cl.first_pose.dtype == np.int32 and cl.first_index.dtype == np.int32, what
    assert cl.pose.tolist() == sum(([p] * len(alive[p]) for p in chosen), []), what
    assert np.array_equal(cl.index, np.concatenate([alive[p] for p in chosen] + [np.empty(0, dtype=np.int64)])), what
    want = np.concatenate(labels + [np.empty(0, dtype=np.int32)])
    if not np.array_equal(cl.label, want):
        bad = np.nonzero(cl.label != want)[0]
        raise AssertionError(f"{what}, r={r}: {len(bad)} of {len(want)} labels differ, first at row {int(bad[0])}: got "
                             f"{int(cl.label[bad[0]])}, expected {int(want[bad[0]])}; {len(cl)} clusters for {len(sizes)}")
    assert np.array_equal(cl.sizes, sizes), what
    assert cl.first_pose.tolist() == [chosen[w] for w in first[:, 0]], what
    assert cl.first_index.tolist() == [int(alive[chosen[w]][i]) for w, i in first.tolist()], what
    return cl


def _launches(fn):
    a, b = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
    out = fn()
    return out, (_counter("octl_debug_launches") - a, _counter("octl_debug_host_syncs") - b)


def _round_robin(P, n):
    return {p: np.ascontiguousarray(P[p::n]) for p in range(n)}


# ---- 1. d2 == r2 joins, one ulp more does not: across leaf walls, voxel walls and poses ------------------------------
def test_the_chain_on_a_grid_a_manager_and_an_octree():
    chain = diagonal_chain()                                    # clusters [0, 41) and [41, 60)
    rng = np.random.default_rng(1)
    far = rng.random((300, 3)) * 0.5 + [2.0, -2.0, 1.0]         # voxels far from the chain: the grid has gaps
    X = np.concatenate([chain, far])
    # a grid with negative and missing voxels, the chain dealt round over three poses
    clouds = _round_robin(X, 3)
    g = _grid(clouds, 4)
    vox = np.asarray(g._forest.voxels)
    assert (vox < 0).any() and len(vox) < np.prod(vox.max(axis=0) - vox.min(axis=0) + 1)
    cl = _check(g, clouds, CHAIN_RADIUS, "chain, grid")
    assert 19 in cl.sizes and cl.label[0] == 0 and cl.sizes[0] == 41
    assert set(cl.pose[cl.members(0)].tolist()) == {0, 1, 2}
    _check(g, clouds, np.nextafter(CHAIN_RADIUS, 0.0), "chain, grid, an ulp less")
    _check(g, clouds, np.nextafter(CHAIN_RADIUS, 1.0), "chain, grid, an ulp more")
    sub = _check(g, clouds, CHAIN_RADIUS, "chain, grid, poses 0 and 2", pose_numbers=[2, 0])
    assert 41 not in sub.sizes and (sub.sizes == 2).sum() >= 18
    # a manager whose cube is not dyadic, pose numbers that are not slots
    named = {4: clouds[0], 9: clouds[1], 2: clouds[2]}
    m = _manager(named, 4, [-2.3, -2.9, -3.1], 6.7)
    cl = _check(m, named, CHAIN_RADIUS, "chain, manager")
    assert 41 in cl.sizes and 19 in cl.sizes and cl.first_pose[0] == 4
    _check(m, named, CHAIN_RADIUS, "chain, manager, poses 9 and 2", pose_numbers=[9, 2])
    # an octree: no pose arguments
    t = _octree(X, 4, [-2.3, -2.9, -3.1], 6.7)
    cl = _check(t, {0: X}, CHAIN_RADIUS, "chain, octree")
    assert cl.sizes[:2].tolist() == [41, 19] and cl.first_index[:2].tolist() == [0, 41]


# ---- 2. the lattice: pairs that straddle d2 == r2 ---------------------------------------------------------------------
def test_the_lattice_and_an_ulp_either_side():
    P, _ = lattice01(-4, 4)
    up, down = ulp_neighbours(P[np.all(P != 0.0, axis=1)])      # (no subnormal coordinates)
    X = np.concatenate([P, up[::5], down[::7]])
    clouds = _round_robin(X, 2)
    g = _grid(clouds, 8)
    a = _check(g, clouds, 0.1, "lattice")
    b = _check(g, clouds, 0.15, "lattice")
    assert len(a) > 1 and b.sizes.max() >= a.sizes.max()
    _check(g, clouds, 0.1, "lattice, pose 1", pose_numbers=[1])
    _check(g, clouds, 0.1, "lattice, gated", lo=2, hi=200)


# ---- 3. deep paths, 4. one contended root ----------------------------------------------------------------------------
def _polyline():
    """5 000 points of one polyline, consecutive ones 0.0125 apart and nothing else within the radius 0.015: 48 rows of
    100 points, 0.05 apart, joined at alternating ends."""
    rows = []
    for k in range(48):
        x = 0.105 + 0.0125 * np.arange(100)
        row = np.column_stack([x if k % 2 == 0 else x[::-1], np.full(100, 0.105 + 0.05 * k), np.full(100, 0.5)])
        rows.append(row)
        if k < 47:
            end = row[-1]
            rows.append(np.column_stack([np.full(3, end[0]), end[1] + 0.0125 * np.arange(1, 4), np.full(3, 0.5)]))
    tail = rows[-1][-1] + np.column_stack([np.zeros(59), 0.0125 * np.arange(1, 60), np.zeros(59)])
    return np.concatenate(rows + [tail])


def test_a_shuffled_polyline_is_one_cluster():
    line = _polyline()
    assert len(line) == 5000
    r = 0.015
    # it IS a polyline: without one inner point it falls in two
    assert cluster_labels_np([(0, np.delete(line, 2500, axis=0))], r)[1].tolist() == [2500, 2499]
    X = line[np.random.default_rng(8).permutation(len(line))]
    for K in (4, 64):
        g = _grid({0: X}, K, L=2)
        cl = _check(g, {0: X}, r, f"polyline, K={K}")
        assert cl.sizes.tolist() == [5000] and (cl.label == 0).all()


def test_a_blob_inside_the_radius_is_one_cluster():
    rng = np.random.default_rng(9)
    X = 0.4 + rng.random((2000, 3)) * 0.05                      # every pair within 0.0867 < 0.1, one voxel
    for clouds, K in (({0: X}, 64), (_round_robin(X, 2), 2000)):    # many leaves; two blocks of one leaf
        g = _grid(clouds, K)
        cl = _check(g, clouds, 0.1, f"blob, K={K}")
        assert cl.sizes.tolist() == [2000]


# ---- 5. the selected poses are the whole graph, 6. duplicates --------------------------------------------------------
def test_bridges_of_other_poses_and_duplicates():
    rng = np.random.default_rng(10)
    a = [0.3, 0.3, 0.3] + rng.random((150, 3)) * 0.1
    b = [0.9, 0.3, 0.3] + rng.random((150, 3)) * 0.1
    bridge = np.column_stack([np.arange(0.40, 0.91, 0.04), np.full(13, 0.35), np.full(13, 0.35)])
    clouds = {0: np.concatenate([a[:80], b[:70]]), 1: np.concatenate([b[70:], a[80:]]), 5: bridge}
    g = _grid(clouds, 16)
    r = 0.08
    whole = _check(g, clouds, r, "bridged")
    assert whole.sizes.tolist() == [313]
    two = _check(g, clouds, r, "not bridged", pose_numbers=[0, 1])
    assert two.sizes.tolist() == [150, 150] and len(two.label) == 300
    only = _check(g, clouds, r, "the bridge alone", pose_numbers=[5])
    assert only.sizes.tolist() == [13]
    # duplicates are neighbours at any radius: pairs and triples of identical rows, far from each other
    base = rng.random((300, 3)) * [3.0, 3.0, 1.0]
    D = {0: np.concatenate([base, base[:100]]), 1: np.concatenate([base[:40], base[200:]])}
    g = _grid(D, 8)
    cl = _check(g, D, 1e-12, "duplicates")
    assert sorted(set(cl.sizes.tolist())) == [1, 2, 3] and (cl.sizes == 3).sum() == 40
    _check(g, D, 0.2, "duplicates, a real radius")


# ---- 7. numbering follows ids, not the layout ------------------------------------------------------------------------
def test_the_smallest_member_is_the_smallest_id_not_the_first_position():
    # a row of points from x = 1.95 DOWN to 0.05 across the wall x = 1: row 0 of pose 0 lies in the second voxel
    x = 1.95 - 0.05 * np.arange(39)
    line = np.column_stack([x, np.full(39, 0.5), np.full(39, 0.5)])
    other = np.column_stack([x, np.full(39, 0.5), np.full(39, 2.5)])
    clouds = {0: np.concatenate([line[:20], other[20:]]), 1: np.concatenate([other[:20], line[20:]])}
    g = _grid(clouds, 4)
    cl = _check(g, clouds, 0.06, "ids and layout")
    assert cl.sizes.tolist() == [39, 39] and cl.first_pose.tolist() == [0, 0] and cl.first_index.tolist() == [0, 20]
    # ... and the layout does put another member first: the position of a cluster's smallest id is not its smallest
    f = g._forest
    perm = np.asarray(f.perm, dtype=np.int64)                   # store index of every position
    pos_of = np.empty(len(perm), dtype=np.int64)
    pos_of[perm] = np.arange(len(perm))
    off = np.concatenate([[0], np.cumsum(f.slot_sizes)]).astype(np.int64)
    store = off[[g._slots[p] for p in cl.pose.tolist()]] + cl.index
    crossed = 0
    for c in range(len(cl)):
        members = cl.members(c)
        crossed += int(pos_of[store[members]].min() != pos_of[store[members[0]]])
    assert crossed >= 1


# ---- 8. the answer does not depend on the subdivision, the layout or the schedule -----------------------------------
def test_the_same_points_subdivided_and_inserted_differently():
    rng = np.random.default_rng(11)
    X = np.concatenate([c + rng.normal(0.0, 0.03, (int(m), 3)) for c, m in
                        zip(rng.uniform(0.2, 2.8, (120, 3)) * [1.0, 1.0, 0.5], rng.integers(1, 80, 120))])
    r = 0.07
    answers = []
    for K, poses in ((8, 1), (64, 1), (8, 4), (64, 4)):
        cuts = np.linspace(0, len(X), poses + 1).astype(int)
        clouds = {p: X[cuts[p]:cuts[p + 1]] for p in range(poses)}        # ids in the order of the rows of X
        g = _grid(clouds, K)
        cl = _check(g, clouds, r, f"K={K}, {poses} poses", lo=2)
        again = cluster(g, r, min_points=2)
        for k in ("pose", "index", "label", "sizes", "first_pose", "first_index"):
            assert np.array_equal(getattr(cl, k), getattr(again, k)), k     # the same call twice
        answers.append((cl.label, cl.sizes, cuts[cl.first_pose] + cl.first_index))
    assert len(answers[0][1]) > 10 and (answers[0][0] == -1).any()
    for other in answers[1:]:
        for a, b in zip(answers[0], other):
            assert np.array_equal(a, b)


# ---- 9. removed points never connect; masked points still do ---------------------------------------------------------
def test_absent_points_never_connect_and_a_pending_mask_still_does():
    clouds = {p: synthetic.planar_cloud(3000, (2, 2, 2), seed=6, stream=p, sigma=0.002) for p in range(3)}
    g = _grid(clouds, 48)
    f = g._forest
    r = 0.03
    full = _check(g, clouds, r, "as inserted")
    g.filter([lambda pts: len(pts) >= 8])
    n1 = f.n_ord
    assert 0 < n1 < 9000
    _check(g, clouds, r, "after filter")
    g.remove_sparse(r, 3)
    _check(g, clouds, r, "after remove_sparse")
    from tests._raycast import box_rays

    rng = np.random.default_rng(2)
    O, D = box_rays(rng, [0, 0, 0], [2, 2, 2], 3000, 0.5)
    assert g.carve_rays(O, D, rng.uniform(0.3, 2.5, 3000), 0.05) > 0
    after = _check(g, clouds, r, "after carve")
    assert len(after.label) == f.n_ord < n1 < len(full.label)
    # a pending RANSAC mask: the kernels never read it - masked points have rows and connect
    np.random.seed(0)
    f.ransac_blocks(np.ascontiguousarray(f.order), np.random.random((128, 6)), 0.01)
    mask = f.device_mask()
    assert 0 < mask.sum() < len(mask)
    pending = _check(g, clouds, r, "with a pending mask")
    assert len(pending.label) == len(mask) and np.array_equal(pending.label, after.label)
    assert np.array_equal(f.device_mask(), mask)                # ... and it is still pending


# ---- 10. remove_small_clusters -----------------------------------------------------------------------------------------
def _speckle_scene():
    rng = np.random.default_rng(12)
    wall = np.column_stack([rng.random((2500, 2)) * [2.0, 2.0], 0.5 + rng.normal(0.0, 0.002, 2500)])
    clumps = np.concatenate([c + rng.normal(0.0, 0.004, (5, 3)) for c in rng.uniform(0.2, 1.8, (40, 3)) + [0.0, 0.0, 1.2]])
    lone = rng.uniform(0.1, 1.9, (60, 3)) + [2.0, 0.0, 0.0]
    X = np.concatenate([wall, clumps, lone])[rng.permutation(2760)]
    return {0: X[:1000], 3: X[1000:1900], 7: X[1900:]}


def test_remove_small_clusters_equals_the_rule():
    clouds = _speckle_scene()
    names = list(clouds)
    r = 0.05
    listed = [(p, clouds[p]) for p in names]
    # remove_sparse keeps the clumps of five: each of their points has four neighbours
    g = _grid(clouds, 32)
    keep6 = small_cluster_keep_np(listed, r, 6)
    gone = sum(int((~k).sum()) for k in keep6)
    assert gone >= 230
    assert g.remove_sparse(r, 1) < gone - 100                    # the lone points go, the clumps stay
    in_clumps = lambda: sum(int(((X[:, 2] > 1.0) & (X[:, 0] < 2.0)).sum()) for X in map(g.get_points, names))
    assert in_clumps() >= 190
    left = {p: g.get_points(p).copy() for p in names}
    keep = small_cluster_keep_np([(p, left[p]) for p in names], r, 6)
    n_nodes, n_vox = len(g._forest.nodes["depth"]), len(g._forest.voxels)
    before_cl = cluster(g, r)
    removed = remove_small_clusters(g, r, 6)
    assert removed == sum(int((~k).sum()) for k in keep) >= 190
    for p, k in zip(names, keep):
        assert g.get_points(p).tobytes() == left[p][k].tobytes(), p
        assert g.n_points(p) == int(k.sum())
    assert in_clumps() <= 20                                    # the clumps are gone (two that touch may stay)
    # Neighbours.index of the survivors is unchanged: the rows of the clouds as inserted
    after_cl = _check(g, clouds, r, "after remove_small_clusters")
    big = before_cl.sizes[before_cl.label] >= 6
    assert np.array_equal(after_cl.pose, before_cl.pose[big]) and np.array_equal(after_cl.index, before_cl.index[big])
    assert after_cl.sizes.min() >= 6
    assert remove_small_clusters(g, r, 6) == 0                   # a second call removes nothing
    # the scheme stays; prune afterwards drops the emptied voxels
    assert len(g._forest.nodes["depth"]) == n_nodes and len(g._forest.voxels) == n_vox
    g.prune()
    assert len(g._forest.voxels) < n_vox
    for p, k in zip(names, keep):
        assert g.get_points(p).tobytes() == left[p][k].tobytes(), (p, "after prune")


def _same_rows(A, B):
    """The same rows, in any order (get_points lists a pose leaf by leaf)."""
    A, B = np.asarray(A).reshape(-1, 3), np.asarray(B).reshape(-1, 3)
    order = lambda X: X[np.lexsort((X[:, 2], X[:, 1], X[:, 0]))]
    return A.shape == B.shape and order(A).tobytes() == order(B).tobytes()


def test_remove_small_clusters_poses_pending_mask_manager_and_octree():
    clouds = _speckle_scene()
    names = list(clouds)
    r = 0.05
    # the selected poses are the whole graph and the only ones judged
    g = _grid(clouds, 32)
    untouched = g.get_points(0).copy()
    keep = small_cluster_keep_np([(3, clouds[3]), (7, clouds[7])], r, 4)
    assert remove_small_clusters(g, r, 4, pose_numbers=[7, 3]) == sum(int((~k).sum()) for k in keep) > 0
    assert g.get_points(0).tobytes() == untouched.tobytes()
    for p, k in zip((3, 7), keep):
        assert _same_rows(g.get_points(p), clouds[p][k]), p
    with pytest.raises(KeyError):
        remove_small_clusters(g, r, 4, pose_numbers=[4])
    # a pending RANSAC mask goes into the same compaction, and its points are judged and connect
    a, plain = _grid(clouds, 32), _grid(clouds, 32)
    fa = a._forest
    np.random.seed(0)
    fa.ransac_blocks(np.ascontiguousarray(fa.order), np.random.random((128, 6)), 0.01)
    mask = fa.device_mask().astype(bool)                         # (per position of the ordered arrays)
    assert 0 < mask.sum() < len(mask)
    off = np.concatenate([[0], np.cumsum(fa.slot_sizes)]).astype(np.int64)
    perm = np.asarray(fa.perm, dtype=np.int64)                   # store index of every position
    keep = small_cluster_keep_np([(p, clouds[p]) for p in names], r, 6)      # the rule BEFORE the call, mask or not
    both = [k.copy() for k in keep]
    for s, p in enumerate(names):
        here = (perm >= off[s]) & (perm < off[s + 1])
        unmasked = np.ones(len(clouds[p]), dtype=bool)
        unmasked[perm[here] - off[s]] = mask[here]
        both[s] &= unmasked
    for g in (a, plain):
        cluster(g, r)                                            # (warm: the index and the tables are in place)
    before = fa.n_ord
    removed, cost = _launches(lambda: remove_small_clusters(a, r, 6))
    _, cost_plain = _launches(lambda: remove_small_clusters(plain, r, 6))
    assert cost == cost_plain, (cost, cost_plain)                # one compaction applies both
    assert removed == before - sum(int(k.sum()) for k in both)
    assert sum(int(k.sum()) for k in both) < min(sum(int(k.sum()) for k in keep), int(mask.sum()))
    for p, k, k_plain in zip(names, both, keep):
        assert _same_rows(a.get_points(p), clouds[p][k]), p
        assert _same_rows(plain.get_points(p), clouds[p][k_plain]), p
    # a manager whose cube is not dyadic, and an octree
    named = {4: clouds[0], 9: clouds[3]}
    m = _manager(named, 32, [-0.3, -0.2, -0.1], 4.7)
    k4, k9 = small_cluster_keep_np([(4, named[4]), (9, named[9])], r, 3)
    assert remove_small_clusters(m, r, 3) == int((~k4).sum() + (~k9).sum()) > 0
    assert _same_rows(m.get_points(4), named[4][k4]) and _same_rows(m.get_points(9), named[9][k9])
    X = np.concatenate([clouds[p] for p in names])
    t = _octree(X, 32, [-0.3, -0.2, -0.1], 4.7)
    k, = small_cluster_keep_np([(0, X)], r, 6)
    assert remove_small_clusters(t, r, 6) == int((~k).sum()) > 0
    assert _same_rows(t.get_points(), X[k])
    with pytest.raises(ValueError, match="single pose"):
        remove_small_clusters(t, r, 6, pose_numbers=[0])
    with pytest.raises(ValueError, match="single pose"):
        cluster(t, r, pose_numbers=[0])


# ---- 11. refusals -------------------------------------------------------------------------------------------------------
def test_refusals():
    clouds = _speckle_scene()
    g = _grid(clouds, 32)
    f = g._forest
    for bad in (0.0, -0.5, float("nan"), float("inf"), 2.0000001, None, "x"):
        with pytest.raises(ValueError):
            cluster(g, bad)
        with pytest.raises(ValueError):
            remove_small_clusters(g, bad, 3)
    with pytest.raises(ValueError, match="voxel edge"):
        cluster(g, 2.5)
    with pytest.raises(ValueError, match="voxel edge"):
        remove_small_clusters(g, 2.5, 2)
    assert len(cluster(g, 2.0)) >= 1                            # (twice the voxel edge is allowed)
    for bad in (0, -1, 2 ** 31, 1.5, None):
        with pytest.raises(ValueError, match="min_points"):
            cluster(g, 0.1, min_points=bad)
        with pytest.raises(ValueError, match="min_points"):
            remove_small_clusters(g, 0.1, bad)
    with pytest.raises(ValueError, match="below min_points"):
        cluster(g, 0.1, min_points=5, max_points=4)
    with pytest.raises(KeyError):
        cluster(g, 0.1, pose_numbers=[4])
    for other in (None, 3, np.zeros((4, 3)), f):
        with pytest.raises(TypeError):
            cluster(other, 0.1)
        with pytest.raises(TypeError):
            remove_small_clusters(other, 0.1, 2)
    n = f.n_ord
    # the ABI: a size query, a selection of the wrong length, a negative cap
    lib, h = f.lib, f.handle
    rows = C.c_int64(-5)
    assert lib.octl_forest_cluster_points(h, 0.1, None, 0, 0, C.byref(rows), None, None, None, None) == 0
    assert rows.value == n
    assert lib.octl_forest_cluster_points(h, 0.1, nat.ptr(np.ones(5, dtype=np.uint8)), 5, 0, C.byref(rows), None, None,
                                          None, None) == nat.OCTL_E_INVALID
    assert lib.octl_forest_cluster_points(h, 0.1, None, 0, -1, C.byref(rows), None, None, None, None) == nat.OCTL_E_INVALID
    assert lib.octl_forest_remove_small_clusters(h, 0.1, 0, None, 0, None) == nat.OCTL_E_INVALID
    assert f.n_ord == n
    # rows moved outside their leaves: no cube bounds what it holds
    g.map_leaf_points(lambda p: p + np.array([0.0, 0.0, 0.4]), [3])
    with pytest.raises(RuntimeError, match="outside their leaves"):
        cluster(g, 0.1)
    with pytest.raises(RuntimeError, match="outside their leaves"):
        remove_small_clusters(g, 0.1, 2)


# ---- 12. launches, and a map that is only read --------------------------------------------------------------------------
def test_launches_and_waits_do_not_depend_on_the_sizes():
    P = synthetic.planar_cloud(20000, (3, 3, 2), seed=3)
    line = _polyline()[np.random.default_rng(8).permutation(5000)]
    blob = 0.4 + np.random.default_rng(9).random((2000, 3)) * 0.05
    seen = {}
    for what, clouds, L, r in (("2000", {0: P[:1000], 1: P[1000:2000]}, 1, 0.1), ("20000", {0: P[:10000], 1: P[10000:]}, 1, 0.1),
                               ("chain", {0: line[:2500], 1: line[2500:]}, 2, 0.015),
                               ("blob", {0: blob[:1000], 1: blob[1000:]}, 1, 0.1)):
        g = _grid(clouds, 64, L)
        cluster(g, r)                                            # (warm: staging, tables, voxel codes and the index,
        assert remove_small_clusters(g, r, 1) == 0               #  the buffers of the compaction - nothing is below 1 -
        cluster(g, r)                                            #  and the index again, which the compaction dropped)
        g._forest.ctx.sync()
        _, seen[what, "cluster"] = _launches(lambda: cluster(g, r))
        _, seen[what, "cluster, gated"] = _launches(lambda: cluster(g, r, min_points=3, max_points=500))
        _, seen[what, "remove"] = _launches(lambda: remove_small_clusters(g, r, 3))
    print(seen)
    for kind in ("cluster", "cluster, gated", "remove"):
        costs = {seen[what, kind] for what in ("2000", "20000", "chain", "blob")}
        assert len(costs) == 1, (kind, seen)
    assert seen["2000", "cluster"] == (4, 1)                    # init, link, flatten, rows; one readback wait
    assert seen["2000", "remove"][1] == 1                       # the compaction's wait is the only one


def test_the_map_is_only_read():
    clouds = _speckle_scene()
    g = _grid(clouds, 32)
    f = g._forest
    Q = np.ascontiguousarray(clouds[0][:50])
    g.radius_count(Q, 0.05)                                     # the block index of every pose
    g.leaf_planes()                                             # a cached table
    nodes = {k: np.array(v) for k, v in f.nodes.items()}
    pts = {p: g.get_points(p).copy() for p in clouds}
    order, n = np.array(f.order), f.n_ord
    _, base = _launches(lambda: g.radius_count(Q, 0.05))
    _, planes = _launches(lambda: g.leaf_planes())
    cluster(g, 0.05)
    cluster(g, 0.05, min_points=2)
    _, again = _launches(lambda: g.radius_count(Q, 0.05))
    _, planes_again = _launches(lambda: g.leaf_planes())
    assert again == base and planes_again == planes             # the index and the pooled planes were reused
    assert f.n_ord == n and np.array_equal(f.order, order)
    for k, v in nodes.items():
        assert np.array_equal(np.array(f.nodes[k]), v), k
    for p in clouds:
        assert g.get_points(p).tobytes() == pts[p].tobytes()
    # another selection makes the index again - and the one before is made again on demand
    cluster(g, 0.05, pose_numbers=[3])
    assert np.array_equal(g.radius_count(Q, 0.05), g.radius_count(Q, 0.05, pose_numbers=[0, 3, 7]))
