"""ray_evidence_np and carve_keep_np - the definitions of ray_evidence and carve (octreelib_amd/query.py) - on hand-made
leaves where every case can be read off: inclusive ends on shared faces, the two intervals, rays without an echo, dead
rays, the keep rule's truth table.  No GPU."""

import ctypes as C
import itertools

import numpy as np
import pytest

import octreelib_amd
from octreelib_amd import RayEvidence, carve_keep_np, ray_evidence_np
from octreelib_amd.query import RAY_CAP_EDGES, HostMap, evidence_inputs
from tests.test_cpu_query import _Leaf

# node 0 is an inner node in spirit (not among the leaves); A = [0, 1]^3 is node 1, B = [1, 2] x [0, 1]^2 is node 2
NODE = np.array([1, 2])
CORNER = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
EDGE = np.array([1.0, 1.0])
A, B = 1, 2


def _ev(o, d, ranges, margin, min_range=0.0, returned=None):
    inp = evidence_inputs(np.atleast_2d(o), np.atleast_2d(d), ranges, margin, min_range, returned)
    return ray_evidence_np(*inp, NODE, CORNER, EDGE, 3), inp


def test_a_ray_along_a_shared_face_counts_both_leaves():
    # x = 1 is the face A and B share; the x axis bounds nothing (d_x = 0) and passes for both: 0 <= 1 <= 1 <= 2
    ev, _ = _ev([1.0, 0.5, -1.0], [0.0, 0.0, 1.0], 3.0, 0.5)
    assert ev.through.tolist() == [0, 1, 1] and ev.hits.tolist() == [0, 0, 0]
    # ... and ending inside them, on the face: a hit in both
    ev, _ = _ev([1.0, 0.5, -1.0], [0.0, 0.0, 1.0], 1.5, 0.25)
    assert ev.hits.tolist() == [0, 1, 1] and ev.through.tolist() == [0, 0, 0]
    # an ulp off the face: one leaf only
    ev, _ = _ev([np.nextafter(1.0, 2.0), 0.5, -1.0], [0.0, 0.0, 1.0], 3.0, 0.5)
    assert ev.through.tolist() == [0, 0, 1]


def test_margin_zero_on_a_face_is_a_hit_in_both_neighbours_and_a_through_in_neither():
    # from x = -1 along +x: A is crossed over t in [1, 2], B over [2, 3]; the measured point lies on their face, t = 2
    ev, (o, d, tmin, tfree, tend) = _ev([-1.0, 0.5, 0.5], [1.0, 0.0, 0.0], 2.0, 0.0)
    assert tfree[0] == tend[0] == 2.0
    assert ev.hits.tolist() == [0, 1, 1] and ev.through.tolist() == [0, 0, 0]
    # the same ray ending one ulp earlier ends in A alone; one ulp later it ends in B and has passed through A
    ev, _ = _ev([-1.0, 0.5, 0.5], [1.0, 0.0, 0.0], np.nextafter(2.0, 0.0), 0.0)
    assert ev.hits.tolist() == [0, 1, 0] and ev.through.tolist() == [0, 0, 0]
    ev, _ = _ev([-1.0, 0.5, 0.5], [1.0, 0.0, 0.0], np.nextafter(2.0, 3.0), 0.0)
    assert ev.hits.tolist() == [0, 0, 1] and ev.through.tolist() == [0, 1, 0]


def test_t_free_below_t_min_gives_no_through():
    # blind up to 1.2, measured 1.5 +- 0.5: F = [1.2, 1.0] is empty, E = [1.2, 2.0] crosses A and touches B
    ev, (o, d, tmin, tfree, tend) = _ev([-1.0, 0.5, 0.5], [1.0, 0.0, 0.0], 1.5, 0.5, min_range=1.2)
    assert tfree[0] < tmin[0] <= tend[0]
    assert ev.through.tolist() == [0, 0, 0] and ev.hits.tolist() == [0, 1, 1]
    # both intervals empty: nothing at all
    ev, (o, d, tmin, tfree, tend) = _ev([-1.0, 0.5, 0.5], [1.0, 0.0, 0.0], 1.5, 0.5, min_range=5.0)
    assert tfree[0] < tmin[0] and tend[0] < tmin[0]
    assert ev.through.sum() == 0 and ev.hits.sum() == 0


def test_a_ray_without_an_echo_hits_nothing():
    O = np.tile([-1.0, 0.5, 0.5], (3, 1))
    D = np.tile([1.0, 0.0, 0.0], (3, 1))
    r = np.array([1.5, 2.0, 3.5])
    with_echo, _ = _ev(O, D, r, 0.25)
    assert with_echo.hits.sum() > 0
    none, (o, d, tmin, tfree, tend) = _ev(O, D, r, 0.25, returned=np.zeros(3, dtype=bool))
    assert np.all(tend < np.maximum(tmin, tfree)) and np.array_equal(tend, np.nextafter(tfree, -np.inf))
    assert none.hits.tolist() == [0, 0, 0]
    # free up to 1.25 / 1.75 / 3.25: A is crossed from t = 1, B from t = 2
    assert none.through.tolist() == [0, 3, 1]
    mixed, _ = _ev(O, D, r, 0.25, returned=np.array([True, False, True]))
    assert mixed.hits.tolist() == [0, 1, 0] and mixed.through.tolist() == [0, 2, 1]


def test_every_kind_of_dead_ray_gives_all_zeros():
    o, d = np.array([-1.0, 0.5, 0.5]), np.array([1.0, 0.0, 0.0])
    live = ray_evidence_np([o], [d], 0.0, 2.5, 3.0, NODE, CORNER, EDGE, 3)
    assert live.through.tolist() == [0, 1, 0] and live.hits.tolist() == [0, 0, 1]
    nan, inf = np.nan, np.inf
    dead = [([nan, 0.5, 0.5], d, 0.0, 2.5, 3.0), ([-1.0, inf, 0.5], d, 0.0, 2.5, 3.0),
            (o, [nan, 0.0, 0.0], 0.0, 2.5, 3.0), (o, [1.0, 0.0, -inf], 0.0, 2.5, 3.0),
            (o, d, nan, 2.5, 3.0), (o, d, -inf, 2.5, 3.0), (o, d, 0.0, nan, 3.0), (o, d, 0.0, inf, 3.0),
            (o, d, 0.0, 2.5, nan), (o, d, 0.0, 2.5, inf),
            (o, [2.0, 0.0, 0.0], 0.0, 2.5, 3.0), (o, [1.0, 0.0, -1.5], 0.0, 2.5, 3.0),      # a component with |d| > 1
            (o, [0.0, 0.0, 0.0], 0.0, 2.5, 3.0), (o, [0.0, -0.0, 0.0], 0.0, 2.5, 3.0),
            (o, [1e-320, 0.0, 0.0], 0.0, 2.5, 3.0),                                             # 1 / d overflows
            ([0.5, 0.5, 0.5], [0.0, 0.0, 0.0], 0.0, 2.5, 3.0)]                                  # (inside A, going nowhere)
    for oo, dd, a, f, e in dead:
        ev = ray_evidence_np([oo], [dd], a, f, e, NODE, CORNER, EDGE, 3)
        assert ev.through.tolist() == [0, 0, 0] and ev.hits.tolist() == [0, 0, 0], (oo, dd, a, f, e)
    # all of them at once, the live ray among them
    rows = dead + [(o, d, 0.0, 2.5, 3.0)]
    ev = ray_evidence_np([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows],
                         [r[4] for r in rows], NODE, CORNER, EDGE, 3, chunk=4)
    assert np.array_equal(ev.through, live.through) and np.array_equal(ev.hits, live.hits)


def test_a_leaf_with_both_gets_a_hit_only():
    # measured 1.5 +- 0.25 from x = -1: F = [0, 1.25] and E = [1.25, 1.75] both cross A (t in [1, 2])
    o, d = [-1.0, 0.5, 0.5], [1.0, 0.0, 0.0]
    free_only, _ = _ev(o, d, 1.5, 0.25, returned=[False])
    assert free_only.through.tolist() == [0, 1, 0]                  # in_F holds for A ...
    ev, _ = _ev(o, d, 1.5, 0.25)
    assert ev.hits.tolist() == [0, 1, 0] and ev.through.tolist() == [0, 0, 0]       # ... and the hit takes it


def test_answer_shape_inner_nodes_and_sums():
    rng = np.random.default_rng(0)
    O = rng.uniform(-2.0, 3.0, (300, 3))
    D = rng.normal(size=(300, 3))
    ev, inp = _ev(O, D, rng.uniform(0.5, 4.0, 300), 0.1)
    assert ev.through.dtype == ev.hits.dtype == np.uint32 and len(ev) == 3
    assert ev.through[0] == 0 and ev.hits[0] == 0 and ev.hits.sum() > 0 and ev.through.sum() > 0
    parts = [ray_evidence_np(*[a[s] for a in inp], NODE, CORNER, EDGE, 3) for s in (slice(0, 100), slice(100, 300))]
    both = parts[0] + parts[1]
    assert np.array_equal(both.through, ev.through) and np.array_equal(both.hits, ev.hits)
    with pytest.raises(ValueError):
        ev + RayEvidence(np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint32))
    e = ray_evidence_np(np.empty((0, 3)), np.empty((0, 3)), 0.0, 1.0, 2.0, NODE, CORNER, EDGE, 3)
    assert e.through.tolist() == [0, 0, 0] and e.hits.dtype == np.uint32
    free = RayEvidence(np.array([0, 2, 5], dtype=np.uint32), np.array([0, 0, 1], dtype=np.uint32))
    assert free.free().tolist() == [False, True, False] and free.free(1, 1).tolist() == [False, True, True]
    assert free.free(3, 5).tolist() == [False, False, True]


def test_inputs_are_checked():
    o, d = np.zeros((2, 3)), np.ones((2, 3))
    for bad in (-0.1, np.nan, np.inf):
        with pytest.raises(ValueError):
            evidence_inputs(o, d, 1.0, bad)
    with pytest.raises(ValueError):
        evidence_inputs(o, d, [1.0, 2.0, 3.0], 0.1)
    with pytest.raises(ValueError):
        evidence_inputs(o, d, 1.0, 0.1, returned=[True])
    with pytest.raises(ValueError):
        evidence_inputs(o, np.ones((3, 3)), 1.0, 0.1)
    _, dn, tmin, tfree, tend = evidence_inputs(o, d * 5.0, [1.0, 2.0], 0.25, 0.5)
    assert np.allclose((dn * dn).sum(axis=1), 1.0) and tmin.tolist() == [0.5, 0.5]
    assert tfree.tolist() == [0.75, 1.75] and tend.tolist() == [1.25, 2.25]


def test_carve_keep_truth_table():
    through = np.array([0, 1, 2, 3, 2, 2], dtype=np.uint32)
    hits = np.array([0, 0, 0, 0, 1, 2], dtype=np.uint32)
    blk_node = np.array([0, 1, 2, 3, 4, 5, 2, 3])
    blk_slot = np.array([0, 0, 0, 0, 0, 0, 1, 1])
    for min_through, max_hits, sel in itertools.product((1, 2, 3), (0, 1, 2), (None, [1, 1], [1, 0], [0, 1], [0, 0])):
        keep = carve_keep_np(blk_node, blk_slot, through, hits, sel, min_through, max_hits)
        assert keep.dtype == bool and keep.shape == (8,)
        for b in range(8):
            chosen = sel is None or bool(sel[blk_slot[b]])
            emptied = chosen and through[blk_node[b]] >= min_through and hits[blk_node[b]] <= max_hits
            assert keep[b] == (not emptied), (min_through, max_hits, sel, b)
    # the defaults: two rays through, none ending
    assert carve_keep_np(blk_node, blk_slot, through, hits).tolist() == [True, True, False, False, True, True, False,
                                                                         False]
    for bad in ((0, 0), (1, -1), (1.5, 0), (True, 0)):
        with pytest.raises(ValueError):
            carve_keep_np(blk_node, blk_slot, through, hits, None, *bad)
    assert carve_keep_np([], [], through, hits).shape == (0,)


def test_host_map_answers_on_the_definition_and_checks_the_cap():
    leaves = {0: [_Leaf(CORNER[0], 1.0, np.full((1, 3), 0.5)), _Leaf(CORNER[1], 1.0, np.empty((0, 3)))]}
    hm = HostMap(0, 1.0, [(CORNER[0], 1.0), (CORNER[1], 1.0)], leaves)
    ev = hm.ray_evidence([[-1.0, 0.5, 0.5]], [[3.0, 0.0, 0.0]], 2.5, 0.25)
    assert len(ev) == 2 and ev.through.tolist() == [1, 0] and ev.hits.tolist() == [0, 1]
    with pytest.raises(ValueError):
        hm.ray_evidence([[-1.0, 0.5, 0.5]], [[1.0, 0.0, 0.0]], RAY_CAP_EDGES + 1.0, 0.25)
    # (a ray that is dead for its range is not checked)
    assert hm.ray_evidence([[-1.0, 0.5, 0.5]], [[1.0, 0.0, 0.0]], np.inf, 0.25).hits.sum() == 0
    one = HostMap(1, 1.0, [(CORNER[0], 1.0)], {0: leaves[0][:1]})
    assert one.ray_evidence([[-1000.0, 0.5, 0.5]], [[1.0, 0.0, 0.0]], 2000.0, 0.25).through.tolist() == [1]


def test_exports_and_signatures():
    from octreelib_amd import _native as nat

    for name in ("RayEvidence", "ray_evidence_np", "carve_keep_np"):
        assert name in octreelib_amd.__all__ and hasattr(octreelib_amd, name)
    p, i32, i64, pi64 = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_int64)
    assert nat.SIGNATURES["octl_forest_ray_evidence"] == (C.c_int, [p, p, p, p, p, p, i64, i64, p, p, pi64])
    assert nat.SIGNATURES["octl_forest_ray_evidence_device"] == (C.c_int, [p, p, p, p, p, p, i64, p, p, i64])
    for name in ("octl_forest_carve", "octl_forest_carve_device"):
        assert nat.SIGNATURES[name] == (C.c_int, [p, p, p, i64, p, i32, i64, i64, pi64])
    lib = nat.load()
    for name in ("octl_forest_ray_evidence", "octl_forest_ray_evidence_device", "octl_forest_carve",
                 "octl_forest_carve_device"):
        assert getattr(lib, name).argtypes == nat.SIGNATURES[name][1]
    from octreelib_amd.grid import Grid
    from octreelib_amd.octree import Octree
    from octreelib_amd.octree_manager import OctreeManager

    for cls in (Grid, OctreeManager, Octree):
        for m in ("ray_evidence", "carve", "carve_rays"):
            assert callable(getattr(cls, m))
