"""The walk of the ray-evidence kernel (octreelib_amd/csrc/raycast_walk.h: ray_evidence - the slab march, the stackless
descent, nothing pruned by a best t) compiled for the CPU alone, with AddressSanitizer and UBSan, as the stand-alone
program tests/host/evidence_host.cpp, and compared with ray_evidence_np count for count over the scenes of
tests/test_cpu_raycast_host.py.  No GPU and nothing loaded into Python: the program gets tables of exactly their size
from a file.  This test is about that program: it compiles it once (a few seconds) and starts it once per scene - and,
in one test, once per ray: a leaf reached twice by one ray would show as a counter of 2."""

import numpy as np
import pytest

from octreelib_amd import synthetic
from octreelib_amd.query import RAY_CAP_EDGES, evidence_inputs
from tests._evidence import (assert_evidence_equal, build_host_program, compare_host, evidence_of_nodes, measured,
                             run_host_program)
from tests._raycast import DIRECTIONS, box_rays, lattice_points, lattice_rays
from tests.test_cpu_query import _depths
from tests.test_cpu_raycast_host import _cube_map, _grid


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("evidence_host")
    return build_host_program(d), d


def test_lattice_walls_and_grazing_contacts(program):
    hm = _grid({0: lattice_points()}, 1, 8)
    assert _depths(hm.nodes).max() == 2
    O, D = lattice_rays()
    rng = np.random.default_rng(0)
    r, ret = measured(rng, len(O), 0.0, 4.0)
    ref, _ = compare_host(program, hm, O, D, r, 0.125, "lattice", returned=ret)
    leaf = hm.nodes["first_child"] < 0
    print(f"lattice: {len(O)} rays, {int(ref.hits.sum())} hits, {int(ref.through.sum())} throughs")
    assert ref.hits[~leaf].sum() == 0 and ref.through[~leaf].sum() == 0
    assert ref.hits.sum() > 500 and ref.through.sum() > 5000 and ((ref.hits + ref.through)[leaf] > 0).mean() > 0.9
    compare_host(program, hm, O, D, r, 0.0, "lattice, margin 0")
    compare_host(program, hm, O, D, r, 0.25, "lattice, blind range", min_range=0.5)
    compare_host(program, hm, O, D, 6.0, 0.5, "lattice, all the way through")


def test_sparse_grid_with_gaps_at_the_cap(program):
    rng = np.random.default_rng(2)
    vox = np.argwhere(rng.random((14, 14, 3)) < 0.25) * [3, 3, 2] - [20, 20, 2]
    P = np.concatenate([v + rng.random((40, 3)) for v in vox])
    hm = _grid({0: P}, 1, 12)
    O, D = box_rays(rng, [-20, -20, -2], [22, 22, 4], 1500, 120.0)
    # the walk's interval [0, range + margin] is exactly the cap
    ref, _ = compare_host(program, hm, O, D, RAY_CAP_EDGES - 0.5, 0.5, "sparse grid, range at the cap")
    assert ref.through.sum() > 300
    r, ret = measured(rng, len(O), 100.0, 250.0)
    ref, _ = compare_host(program, hm, O, D, r, 0.5, "sparse grid, measured", returned=ret)
    print(f"sparse grid: {int(ref.hits.sum())} hits, {int(ref.through.sum())} throughs")
    assert ref.hits.sum() > 0 and ref.through.sum() > 100
    compare_host(program, hm, O, D, 200.0 + RAY_CAP_EDGES - 1.0, 1.0, "sparse grid, the cap from min_range",
                 min_range=200.0)
    # above the cap the device form adds nothing (the host form refuses)
    exe, d = program
    inp = evidence_inputs(O[:50], D[:50], RAY_CAP_EDGES, 0.5)
    over = run_host_program(exe, d, hm, *inp)
    assert over.through.sum() == 0 and over.hits.sum() == 0
    # axis rays along voxel walls and through the gaps
    A = np.repeat(np.array([[-30.0, 1.0, 0.5], [-30.0, -8.0, 1.0], [4.0, 40.0, 0.0], [1.5, 1.5, -40.0]]), 6, axis=0)
    Da = np.tile(DIRECTIONS[np.abs(DIRECTIONS).sum(axis=1) == 1], (4, 1))
    ref, _ = compare_host(program, hm, A, Da, 100.0, 0.5, "sparse grid, axis rays")
    assert ref.through.sum() > 0


def test_non_dyadic_cube(program):
    rng = np.random.default_rng(5)
    c0, e0 = 0.1, 3.3
    P = c0 + rng.random((5000, 3)) * e0 * [1.0, 1.0, 0.3]
    P = P[np.all((P - c0 >= 0) & (P - c0 < e0), axis=1)]
    hm = _cube_map(P, [c0, c0, c0], e0, 20)
    assert _depths(hm.nodes).max() >= 3
    nd = hm.nodes
    inner = np.nonzero(nd["first_child"] >= 0)[0]
    split = nd["corner"][inner] + (nd["edge"][inner] / 2.0)[:, None]             # points on the splitting planes
    S = np.repeat(split[:100], 3, axis=0)
    S[:, 0] -= 5.0
    Ds = np.tile(np.array([[1.0, 0, 0], [1.0, 0.3, 0], [1.0, 0, -0.2]]), (100, 1))
    Ob, Db = box_rays(rng, [c0] * 3, [c0 + e0] * 3, 400, 2.0)
    O, D = np.concatenate([S, Ob]), np.concatenate([Ds, Db])
    r, ret = measured(rng, len(O), 1.0, 9.0)
    ref, _ = compare_host(program, hm, O, D, r, 0.05, "non-dyadic cube", returned=ret)
    assert ref.hits.sum() > 100 and ref.through.sum() > 1000
    compare_host(program, hm, O, D, 2e6, 1.0, "non-dyadic cube from afar", min_range=3.0)          # (one cube has no cap)


def test_utm_offsets_and_an_unsplit_voxel(program):
    rng = np.random.default_rng(7)
    off = np.array([5.0e6, 4.0e5, 100.0])
    U = synthetic.planar_cloud(6000, (3, 3, 2), seed=9) + off
    hm = _grid({0: U[:4000], 1: U[4000:]}, 1, 32)
    assert _depths(hm.nodes).max() >= 2
    O, D = box_rays(rng, off, off + [3, 3, 2], 2000, 2.0)
    O[:200] = np.floor(O[:200])                                                      # on voxel walls
    D[:100] = DIRECTIONS[rng.integers(0, len(DIRECTIONS), 100)]
    r, ret = measured(rng, len(O), 0.5, 6.0)
    ref, _ = compare_host(program, hm, O, D, r, 0.02, "utm", returned=ret)
    assert ref.hits.sum() > 500 and ref.through.sum() > 5000
    # one voxel of 5 000 points, never subdivided: a root that is a leaf
    h0 = _grid({0: rng.random((5000, 3))}, 1, 10 ** 6)
    assert len(h0.nodes["edge"]) == 1
    O0, D0 = box_rays(rng, [0, 0, 0], [1, 1, 1], 300, 2.0)
    r0, _ = compare_host(program, h0, O0, D0, 1.5, 0.5, "one unsplit voxel")
    assert 0 < r0.hits[0] < 300 and 0 < r0.through[0] < 300


def test_one_ray_per_run_reaches_every_leaf_once(program):
    """Rays along voxel walls and through voxel corners are where a leaf could be reached from two slabs or two
    ranges of a slab: with ONE ray per run a counter of 2 would show it."""
    exe, d = program
    hm = _grid({0: lattice_points()}, 1, 8)             # voxels [0, 2)^3, walls at 0, 1, 2
    axes = DIRECTIONS[np.abs(DIRECTIONS).sum(axis=1) == 1]
    diag = DIRECTIONS[np.abs(DIRECTIONS).sum(axis=1) == 3]
    O, D = [], []
    for a in axes:                                       # along the wall x / y / z = 1, in the wall's plane, on an edge
        for o in ([1.0, 1.0, 1.0], [1.0, 0.5, 1.0], [1.0, 1.0, 0.25], [0.5, 1.0, 1.0], [2.0, 1.0, 0.0]):
            O.append(np.asarray(o) - 3.0 * a)
            D.append(a)
    for g in diag:                                       # through the corner shared by all eight voxels, and others
        for c in ([1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [2.0, 2.0, 2.0], [1.0, 1.0, 0.0], [0.5, 0.5, 0.5]):
            O.append(np.asarray(c) - 2.0 * g)
            D.append(g)
    for g in DIRECTIONS[np.abs(DIRECTIONS).sum(axis=1) == 2][:6]:       # face diagonals inside a wall
        O.append(np.array([1.0, 1.0, 1.0]) - 2.5 * g)
        D.append(g)
    O, D = np.array(O), np.array(D)
    twice = 0
    for i in range(len(O)):
        inp = evidence_inputs(O[i:i + 1], D[i:i + 1], 8.0, 0.5)
        got = run_host_program(exe, d, hm, *inp)
        ref = evidence_of_nodes(hm.nodes, *inp)
        assert_evidence_equal(got, ref, f"ray {i}: o = {O[i]}, d = {D[i]}")
        assert got.through.max() <= 1 and got.hits.max() <= 1
        twice += int(ref.through.sum() >= 8)
    # (the rays do cross many leaves each: walls and corners touch up to eight leaves at a time)
    assert twice >= len(O) // 2
