"""cell_index_np, cell_count_np and thin_keep_np, the definitions of the cell count and of voxel-grid thinning
(octreelib_amd/thinning.py), HostMap.cell_count / thin - what the classes on the caller's own plug types answer with -
and the refusals of the module-level cell_count / thin that need no GPU.  The definitions hash cell indices; here they
are held to an independent dict-of-tuples model in exact rational arithmetic (tests/_cell.py).  The device kernels are
compared with the definitions count for count in tests/test_gpu_cell.py."""

import ctypes as C
import itertools
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import octreelib_amd
from octreelib_amd import cell_count, cell_count_np, cell_index_np, check_cell_args, thin, thin_keep_np, thinning
from octreelib_amd.query import COUNT_MAX, HostMap
from tests._cell import CELL, exact_cell, lattice01, model_count, model_keep, ulp_neighbours
from tests.test_cpu_map_operations import UNKNOWN, _on_plug_types
from tests.test_cpu_radius import _Leaf


def _clouds(seed=3):
    """Three poses (numbers that are not positions) of a few hundred points over [-1, 1)^3: about three points per
    cell of 0.25, duplicates within one pose and across poses, rows that are not finite."""
    rng = np.random.default_rng(seed)
    A, B, D = rng.uniform(-1.0, 1.0, (500, 3)), rng.uniform(-1.0, 1.0, (400, 3)), rng.uniform(-1.0, 1.0, (300, 3))
    A[200:220] = A[100:120]                # duplicates within a pose: the earlier row wins
    B[:40] = A[:40]                        # ... and across poses: the earlier pose wins
    D[:25], D[25:40] = B[100:125], A[:15]
    D[290] = [np.nan, 0.0, 0.0]
    D[291] = [0.5, np.inf, 0.5]
    return [(7, A), (2, B), (11, D)]


def test_definitions_equal_an_independent_model():
    clouds = _clouds()
    rng = np.random.default_rng(4)
    Q = np.concatenate([rng.uniform(-1.2, 1.2, (300, 3)), clouds[0][1][:50], clouds[2][1][280:],
                        [[np.nan, 0.5, 0.5], [0.5, -np.inf, 0.5], [1e300, 0.0, 0.0]]])
    for cell in (0.25, 0.07):
        full = cell_count_np(Q, clouds, cell)
        assert full.dtype == np.int32 and full.shape == (len(Q),)
        assert np.array_equal(full, model_count(Q, clouds, cell))
        for cap in (1, 3, 7, COUNT_MAX):
            assert np.array_equal(cell_count_np(Q, clouds, cell, max_count=cap), np.minimum(full, cap))
        assert np.array_equal(cell_count_np(Q, clouds[1:2], cell), model_count(Q, clouds[1:2], cell))
        assert np.all(full[-3:] == 0)                                # queries that are not finite, or far away
    assert (cell_count_np(Q, clouds, 0.25) > 3).any() and (cell_count_np(Q, clouds, 0.25) == 0).any()
    names = [p for p, _ in clouds]
    subsets = [s for r in (1, 2, 3) for s in itertools.combinations(names, r)]
    seen_removed = 0
    for m in (1, 2, 5):
        for tested in subsets:
            for counted in subsets:        # every combination, a tested pose that is not counted included
                want = model_keep(clouds, counted, tested, 0.25, m)
                cc = [c for c in clouds if c[0] in counted]
                tt = [p if p in counted else (p, P, sum(1 for q in names[:names.index(p)] if q in counted))
                      for p, P in clouds if p in tested]
                got = thin_keep_np(cc, tt, 0.25, m)
                by = {p: got[i] for i, (p, _) in enumerate(cc)}
                extra = len(cc)
                for (p, P), w in zip(clouds, want):
                    if p in tested and p in counted:
                        k = by[p]
                    elif p in tested:
                        k, extra = got[extra], extra + 1
                    else:
                        assert p not in by or by[p].all()
                        continue
                    assert k.dtype == bool and np.array_equal(k, w), (m, tested, counted, p)
                    seen_removed += int((~k).sum())
    assert seen_removed > 1000
    # a pair without a position is a new scan: after every counted cloud
    a, = thin_keep_np(clouds[:2], [clouds[2]], 0.25, 2)[2:]
    b, = thin_keep_np(clouds[:2], [(11, clouds[2][1], 2)], 0.25, 2)[2:]
    assert np.array_equal(a, b) and np.array_equal(a, cell_count_np(clouds[2][1], clouds[:2], 0.25) < 2)
    # ... and one that comes before every counted cloud loses nothing
    assert thin_keep_np(clouds[:2], [(11, clouds[2][1], 0)], 0.25, 1)[2].all()


def test_the_default_rule_keeps_the_first_of_every_cell_and_is_idempotent():
    clouds = _clouds(5)
    for m in (1, 3):
        keep = thin_keep_np(clouds, None, 0.25, m)
        left = [(p, P[k]) for (p, P), k in zip(clouds, keep)]
        assert 0 < sum(int(k.sum()) for k in keep) < sum(len(k) for k in keep)
        again = thin_keep_np(left, None, 0.25, m)
        assert all(k.all() for k in again)
        per_cell = {}
        for _, P in left:
            for row in P.tolist():
                key = exact_cell(row, 0.25)
                per_cell[key] = per_cell.get(key, 0) + 1
        assert max(v for k, v in per_cell.items() if k is not None) == m
        # nothing that was occupied became empty
        before = {exact_cell(r, 0.25) for _, P in clouds for r in P.tolist()}
        assert before == set(per_cell)
    # duplicates: the smaller id wins, within a pose and across poses
    keep = thin_keep_np(clouds, None, 1e-6, 1)
    assert keep[0][100:120].all() and not keep[0][200:220].any() and not keep[1][:40].any()
    assert not keep[2][:40].any() and keep[2][290] and keep[2][291]          # (rows that are not finite stay)


def test_lattice_coordinates_fall_either_side_of_their_walls():
    k = np.arange(-2000, 2000)
    x = k * CELL
    idx = cell_index_np(np.column_stack([x, x, x]), CELL)[:, 0]
    exact = np.array([(Fraction(float(v)) / Fraction(CELL)).__floor__() for v in x])
    assert np.array_equal(idx, exact)
    assert int((exact == k - 1).sum()) == 1988 and int((exact == k).sum()) == 4000 - 1988      # fl(k * 0.1) below k * 0.1
    P, K = lattice01()
    up, down = ulp_neighbours(P)
    for X in (P, up, down):
        got = cell_index_np(X, CELL)
        want = np.array([exact_cell(r, CELL) for r in X.tolist()], dtype=np.float64)
        assert np.array_equal(got, want)
    assert (cell_index_np(P, CELL) < K).any() and (cell_index_np(P, CELL) == K).any()
    assert (cell_index_np(up, CELL) != cell_index_np(down, CELL)).any()
    Q = np.concatenate([P[::3], up[::3], down[::3]])
    clouds = [(0, P[::2]), (1, P[1::2])]
    got = cell_count_np(Q, clouds, CELL)
    assert np.array_equal(got, model_count(Q, clouds, CELL))
    assert got.max() > 1 and (got == 0).any()          # walls that moved put two lattice points into one cell
    keep = thin_keep_np(clouds, None, CELL, 1)
    assert all(np.array_equal(a, b) for a, b in zip(keep, model_keep(clouds, (0, 1), (0, 1), CELL, 1)))
    assert not all(k.all() for k in keep)


def test_argument_refusals_and_exports():
    P = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    for c in (0.0, -1.0, np.nan, np.inf, -np.inf, None, "x"):
        with pytest.raises(ValueError):
            check_cell_args(c)
        with pytest.raises(ValueError):
            cell_index_np(P, c)
        with pytest.raises(ValueError):
            cell_count_np(P, [(0, P)], c)
        with pytest.raises(ValueError):
            thin_keep_np([(0, P)], None, c)
    for bad in (0, -1, 2 ** 31, 1.5, 2.0, True, "3"):
        with pytest.raises(ValueError):
            check_cell_args(1.0, max_count=bad)
        with pytest.raises(ValueError):
            check_cell_args(1.0, max_per_cell=bad)
        with pytest.raises(ValueError):
            cell_count_np(P, [(0, P)], 1.0, max_count=bad)
        with pytest.raises(ValueError):
            thin_keep_np([(0, P)], None, 1.0, bad)
    with pytest.raises(ValueError):
        thin_keep_np([(0, P)], None, 1.0, None)
    assert check_cell_args(np.float32(0.5), np.int64(3), 2 ** 31 - 1) == (0.5, 3, COUNT_MAX)
    assert check_cell_args(2, None, None) == (2.0, None, None)
    with pytest.raises(ValueError):
        cell_count_np(np.zeros((3, 2)), [(0, P)], 1.0)
    with pytest.raises(ValueError):
        thin_keep_np([(1, P)], [2], 1.0)                       # brings no points
    with pytest.raises(ValueError):
        thin_keep_np([(1, P)], [(1, P)], 1.0)                  # counted: named by its number
    assert cell_count_np(np.empty((0, 3)), [(0, P)], 1.0).shape == (0,)
    assert cell_count_np(P, [], 1.0).tolist() == [0, 0] and cell_count_np(P, [(0, np.empty((0, 3)))], 1.0).tolist() == [0, 0]
    assert cell_count_np(P.astype(np.float32), [(0, P)], 2.0).tolist() == [2, 2]
    assert [k.tolist() for k in thin_keep_np([(0, np.empty((0, 3)))], None, 1.0)] == [[]] and thin_keep_np([], None, 1.0) == []
    assert cell_index_np(np.array([[-0.05, 0.0, -0.0], [0.1, 0.3, -0.3]]), 0.1).tolist() == [[-1.0, 0.0, 0.0], [1.0, 2.0, -3.0]]
    assert str(cell_index_np(np.array([[-0.0, 0.0, 0.0]]), 0.1)[0, 0]) == "0.0"
    for name in ("cell_index_np", "cell_count_np", "thin_keep_np", "check_cell_args", "cell_count", "thin"):
        assert name in octreelib_amd.__all__ and getattr(octreelib_amd, name) is getattr(thinning, name)
    assert sorted(thinning.__all__) == ["cell_count", "cell_count_np", "cell_index_np", "check_cell_args", "thin",
                                        "thin_keep_np", "thin_ranks_np"]
    from octreelib_amd import matching

    assert sorted(matching.__all__) == ["align_nearest_planes", "nearest_plane_registration_system"]


def test_declared_and_in_the_signature_table():
    from octreelib_amd import _native as nat

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "octreelib_hip.h")).read()
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    p, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    assert ("int octl_forest_cell_count(octl_forest* f, const double* xyz, int64_t n, double cell, int32_t max_count, "
            "const uint8_t* slot_sel, int32_t n_sel, int32_t* count);") in header
    assert ("int octl_forest_cell_count_device(octl_forest* f, const double* xyz_dev, int64_t n, double cell, int32_t "
            "max_count, const uint8_t* slot_sel, int32_t n_sel, int32_t* count_dev);") in header
    assert ("int octl_forest_thin(octl_forest* f, double cell, int32_t max_per_cell, const uint8_t* slot_sel, int32_t "
            "n_sel, const uint8_t* among_sel, int32_t n_among, int64_t* n_alive);") in header
    for name in ("octl_forest_cell_count", "octl_forest_cell_count_device"):
        assert nat.SIGNATURES[name] == (C.c_int, [p, p, i64, f64, i32, p, i32, p])
    assert nat.SIGNATURES["octl_forest_thin"] == (C.c_int, [p, f64, i32, p, i32, p, i32, C.POINTER(C.c_int64)])


def test_host_map_agrees_with_the_definitions():
    rng = np.random.default_rng(5)
    roots = [(np.array([0.0, 0.0, 0.0]), 2.0), (np.array([2.0, 0.0, 0.0]), 2.0)]
    pts = {p: rng.uniform(0.0, 4.0, (n, 3)) * [1.0, 0.5, 0.5] for p, n in ((3, 700), (8, 500), (11, 40))}
    leaves = {p: [_Leaf(c, e, P[(P[:, 0] >= c[0]) & (P[:, 0] < c[0] + e)]) for c, e in roots] for p, P in pts.items()}
    hm = HostMap(0, 2.0, roots, leaves)
    clouds = hm.clouds()
    assert [p for p, _ in clouds] == [3, 8, 11]
    Q = np.concatenate([rng.uniform(-0.5, 4.5, (300, 3)) * [1.0, 0.5, 0.5], [[np.nan, 0.0, 0.0]]])
    for cap in (None, 1, 3, 7):
        assert np.array_equal(hm.cell_count(Q, 0.3, max_count=cap), cell_count_np(Q, clouds, 0.3, max_count=cap))
    assert np.array_equal(hm.cell_count(Q, 0.3, pose_numbers=[8]), cell_count_np(Q, clouds[1:2], 0.3))
    assert (hm.cell_count(Q, 0.3) > 3).any()
    got = hm.thin(0.3, 2)
    ref = thin_keep_np(clouds, None, 0.3, 2)
    assert [p for p, _ in got] == [3, 8, 11] and all(np.array_equal(k, r) for (_, k), r in zip(got, ref))
    assert 0 < sum(int(k.sum()) for _, k in got) < sum(len(k) for _, k in got)
    # the newest pose against the whole map; against the older poses only (it is not counted itself)
    (p, k), = hm.thin(0.3, pose_numbers=[11])
    assert p == 11 and np.array_equal(k, thin_keep_np(clouds, [11], 0.3)[2])
    (p, k), = hm.thin(0.3, 2, pose_numbers=[11], among=[3, 8])
    assert p == 11 and np.array_equal(k, cell_count_np(clouds[2][1], clouds[:2], 0.3) < 2) and not k.all()
    # the oldest pose against the newer ones: nothing comes before it
    (p, k), = hm.thin(0.3, 1, pose_numbers=[3], among=[8, 11])
    assert p == 3 and k.all()
    # the middle pose is judged against the older one of the two
    (p, k), = hm.thin(0.3, 1, pose_numbers=[8], among=[3, 11])
    assert p == 8 and np.array_equal(k, cell_count_np(clouds[1][1], clouds[:1], 0.3) < 1)
    for bad in (2.5, 2.0 * 2.0 ** -21):
        with pytest.raises(ValueError, match="voxel edge"):
            hm.cell_count(Q, bad)
        with pytest.raises(ValueError, match="voxel edge"):
            hm.thin(bad)
    assert hm.cell_count(Q, 2.0).sum() > 0                       # (the voxel edge itself is allowed)
    for bad in (None, 0, 1.5, True):
        with pytest.raises(ValueError):
            hm.thin(0.3, bad)
    cube = HostMap(1, 4.0, [(np.array([-1.0e6, 0.0, 0.0]), 4.0)], {0: [_Leaf(np.array([-1.0e6, 0.0, 0.0]), 4.0, np.empty((0, 3)))]})
    with pytest.raises(ValueError, match="reach"):
        cube.cell_count(Q, 1.0e6 * 2.0 ** -50)
    assert cube.cell_count(Q, 1.0e6 * 2.0 ** -49).tolist() == [0] * len(Q)


@pytest.mark.parametrize("name", ["Grid", "OctreeManager"])
def test_plug_types(name):
    obj = _on_plug_types(name)
    pts = obj._host_map().clouds()[0][1]
    assert len(pts) == 50
    Q = np.concatenate([pts[:20], [[0.5, 0.5, 0.5], [np.nan, 0.0, 0.0], [9.0, 9.0, 9.0]]])
    for cap in (None, 1):
        got = cell_count(obj, Q, 0.25, max_count=cap, pose_numbers=[0])
        assert np.array_equal(got, cell_count_np(Q, [(0, pts)], 0.25, max_count=cap)) and got[:20].min() >= 1
    (p, k), = obj._host_map().thin(0.25)
    assert p == 0 and np.array_equal(k, thin_keep_np([(0, pts)], None, 0.25)[0]) and 0 < k.sum() < 50
    with pytest.raises(NotImplementedError) as raised:
        thin(obj, 0.25, pose_numbers=[UNKNOWN], among=[UNKNOWN])       # refused by name before the pose lookup
    assert type(raised.value) is NotImplementedError
    assert "plug types" in str(raised.value) and name in str(raised.value) and "HostMap.thin" in str(raised.value)
    with pytest.raises(KeyError):
        cell_count(obj, Q, 0.25, pose_numbers=[UNKNOWN])
    for bad in (0.0, np.nan, "x"):
        with pytest.raises(ValueError):
            cell_count(obj, Q, bad)
    with pytest.raises(ValueError):
        cell_count(obj, Q, 0.25, max_count=0)
    with pytest.raises(ValueError, match="voxel edge" if name == "Grid" else "reach"):
        cell_count(obj, Q, 2.5 if name == "Grid" else 2.0 ** -49)
    for other in (None, 3, np.zeros((4, 3)), obj._host_map()):
        with pytest.raises(TypeError):
            cell_count(other, Q, 0.25)
        with pytest.raises(TypeError):
            thin(other, 0.25)
