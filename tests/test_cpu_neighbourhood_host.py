"""The row of the neighbourhood kernels (octreelib_amd/csrc/radius_moments.h: the moments sink, finish with p0 = q and
the eigen solver, over the walk of nearest_walk.h) compiled for the CPU alone, with AddressSanitizer and UBSan, as the
stand-alone program tests/host/moments_host.cpp, and compared with neighbourhood_statistics_np over host-built maps:
counts exact, moments within the derived bound of DESIGN.md 4.23 against exact rationals.  No GPU and nothing loaded
into Python: the program gets tables of exactly their size from a file, so a lookup outside one, a signed overflow or a
bad conversion ends it with an error instead of a wrong answer.  This is where a wrong sink or a wrong shift of finish
shows without a GPU.  The test compiles the program once (a few seconds) and starts it once per case."""

import numpy as np
import pytest

from octreelib_amd import neighbourhood_statistics_np, radius_count_np
from oracle.octree_np import OGrid
from tests._cell import host_tables, lattice01, ulp_neighbours
from tests._neighbourhood import (assert_exact_bound, assert_reference_bound, build_host_program, neighbours_of,
                                  pick_rows, run_host_program)
from tests.test_cpu_query import _depths, _grid_map
from tests.test_cpu_raycast_host import _cube_map
from tests.test_gpu_leaf_stats import _assert_eigen


# (far away, not finite, outside every voxel.  No query beyond 2^63 voxel edges: for such a one the walk forms - and
#  then discards - voxel indices by a float-to-integer conversion that saturates on the device and that UBSan refuses
#  on the host; tests/test_gpu_neighbourhood.py covers 1e300 on the device)
BAD = np.array([[1e15, 0.0, 0.0], [0.0, -2.0 ** 31, 0.0], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf],
                [-777.5, 3.0, 3.0]])


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("moments_host")
    return build_host_program(d), d


def _grid(clouds, L, K):
    og = OGrid(L)
    for p, P in clouds.items():
        og.insert_points(p, P)
    og.subdivide(K)
    return _grid_map(og, L)


def _compare(program, hm, Q, radius, what, pose_numbers=None, limit=40, max_n=100):
    """The host build against the definition: counts exact, NaN rows where nothing is near, the bound on `limit` rows
    against rationals and on every row against the longdouble definition, the eigen contract on the program's own
    covariance.  Returns the counts."""
    exe, d = program
    clouds = hm.clouds(pose_numbers)
    got = run_host_program(exe, d, hm, Q, radius, pose_numbers=pose_numbers)
    want = radius_count_np(Q, clouds, radius)
    if not np.array_equal(got.count, want):
        bad = np.nonzero(got.count != want)[0]
        raise AssertionError(f"{what}, r={radius}: {len(bad)} of {len(Q)} counts differ, first {int(bad[0])} at "
                             f"{Q[bad[0]].tolist()}: got {int(got.count[bad[0]])}, expected {int(want[bad[0]])}")
    none = want == 0
    for a in (got.mean, got.covariance, got.eigenvalues, got.eigenvectors):
        assert np.isnan(a[none]).all() and np.isfinite(a[~none]).all(), what
    lists = neighbours_of(Q, clouds, radius)
    worst = assert_exact_bound(got, Q, lists, pick_rows(want, limit, max_n), what)
    print(f"{what}, r={radius}: largest error / bound: mean {worst[0]:.3f}, covariance {worst[1]:.3f}")
    ref = neighbourhood_statistics_np(Q, clouds, radius, dtype=np.longdouble, eigen=False)
    assert_reference_bound(got, ref, Q, lists, np.nonzero(~none)[0], what)
    _assert_eigen(got.eigenvalues[~none], got.eigenvectors[~none], got.covariance[~none], gap_check=False)
    one = want == 1
    assert np.all(got.covariance[one] == 0.0) and np.all(got.eigenvalues[one] == 0.0), what
    # without the decomposition the moments are the same bits
    plain = run_host_program(exe, d, hm, Q, radius, eigen=False, pose_numbers=pose_numbers)
    assert plain.eigenvalues is None and plain.mean.tobytes() == got.mean.tobytes()
    assert plain.covariance.tobytes() == got.covariance.tobytes() and np.array_equal(plain.count, got.count)
    return want


def test_the_lattice_and_an_ulp_either_side(program):
    P, _ = lattice01()
    hm = _grid({0: P[::2], 1: P[1::2]}, 1, 8)
    assert _depths(hm.nodes).max() >= 2
    up, down = ulp_neighbours(P)
    Q = np.concatenate([P[::2], up[::7], down[::7], np.column_stack([up[::11, 0], P[::11, 1], down[::11, 2]]), BAD])
    # fl(k 0.1) steps either side of 0.1: pairs of lattice neighbours straddle the sphere of radius 0.1
    for r in (0.1, 0.15):
        c = _compare(program, hm, Q, r, "lattice")
        assert c.max() > 4 and (c[:len(P[::2])] >= 1).all() and np.all(c[-len(BAD):] == 0)
    c1 = radius_count_np(Q, hm.clouds(), 0.1)
    assert len(np.unique(c1[:len(P[::2])])) > 3                      # the rounding of k 0.1 decides who is inside
    _compare(program, hm, Q[::4], 0.15, "lattice, pose 1", pose_numbers=[1], limit=16)


def test_a_grid_with_missing_and_negative_voxels(program):
    rng = np.random.default_rng(2)
    vox = np.argwhere(rng.random((5, 5, 3)) < 0.45) - [2, 2, 1]                      # occupied voxels with gaps, negative too
    P = np.concatenate([v + rng.random((60, 3)) for v in vox])
    P[:300:3] = np.floor(P[:300:3] * 8) / 8                                        # on leaf and voxel walls
    hm = _grid({0: P[::2], 1: P[1::2]}, 1, 10)
    assert _depths(hm.nodes).max() >= 2 and len(vox) < 5 * 5 * 3
    Q = np.concatenate([P[::3] + rng.normal(0.0, 0.02, (len(P[::3]), 3)), P[:200], rng.uniform(-3.0, 4.0, (300, 3)),
                        np.floor(P[:100]), np.floor(P[:100]) + [0.0, 0.5, 1.0], BAD])
    for r in (0.15, 0.4, 2.0):                                                   # inside a leaf, across voxels, the cap 2 L
        c = _compare(program, hm, Q, r, "sparse grid", limit=24)
        assert c.max() > 1 and np.all(c[-5:] == 0)
    assert radius_count_np(Q, hm.clouds(), 2.0).max() > 600
    _compare(program, hm, Q[::2], 0.4, "sparse grid, pose 0", pose_numbers=[0], limit=16)
    # the same scene far from the origin: the bound holds with R from the neighbourhood, not from the coordinates
    far = P + 2.0 ** 20
    hm = _grid({0: far[::2], 1: far[1::2]}, 1, 10)
    c = _compare(program, hm, Q[:600] + 2.0 ** 20, 0.4, "sparse grid at 2^20", limit=24)
    assert c.max() > 8


def test_a_cube_that_is_not_dyadic(program):
    rng = np.random.default_rng(5)
    c0, e0 = 0.1, 3.3
    P = c0 + rng.random((4000, 3)) * e0 * [1.0, 1.0, 0.3]
    P = P[np.all((P - c0 >= 0) & (P - c0 < e0), axis=1)]
    hm = _cube_map(P, [c0, c0, c0], e0, 20)
    assert _depths(hm.nodes).max() >= 3
    nd = hm.nodes
    inner = np.nonzero(nd["first_child"] >= 0)[0]
    split = nd["corner"][inner] + (nd["edge"][inner] / 2.0)[:, None]                # points on the splitting planes
    Q = np.concatenate([P[:400] + rng.normal(0.0, 0.01, (400, 3)), P[:200], split[:150], np.nextafter(split[:100], -9.0),
                        rng.uniform(-0.5, 4.0, (200, 3)), BAD])
    for r in (0.08, 0.3, 5.0):                                                   # (one cube has no cap on the radius)
        c = _compare(program, hm, Q[::(1 if r < 5.0 else 40)], r, "non-dyadic cube", limit=24)
        assert c.sum() > 0
    assert radius_count_np(Q[:1], hm.clouds(), 5.0)[0] > 3000
    # the tables the program read are the ones the walk is defined on
    t = host_tables(hm)
    assert len(t["xyz_ord"]) == len(P) and t["cnt"].sum() == len(t["rec"])
