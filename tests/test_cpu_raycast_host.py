"""The traversal of the raycast kernel (octreelib_amd/csrc/raycast_walk.h: the slab march over the top-level voxels,
the stackless walk, the widened-box pruning) compiled for the CPU alone, with AddressSanitizer and UBSan, as the
stand-alone program tests/host/raycast_host.cpp, and compared with raycast_np bit for bit over host-built maps.  No GPU
and nothing loaded into Python: the program gets tables of exactly their size from a file, so a lookup outside one, a
signed overflow or a bad conversion ends it with an error instead of a wrong answer.  This test is about that program:
it compiles it once (a few seconds) and starts it once per scene."""

import numpy as np
import pytest

from octreelib_amd import normalize_directions, raycast_np, synthetic
from octreelib_amd.query import RAY_CAP_EDGES, HostMap, node_table_from_leaves
from oracle.octree_np import OGrid, OTree, tree_leaf_table
from tests._raycast import (DIRECTIONS, assert_hits_equal, box_rays, build_host_program, host_counts, lattice_points,
                            lattice_rays, leaves_of, run_host_program, tie_mask)
from tests.test_cpu_query import _Leaf, _depths, _grid_map


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("raycast_host")
    return build_host_program(d), d


def _grid(clouds, L, K):
    og = OGrid(L)
    for p, P in clouds.items():
        og.insert_points(p, P)
    og.subdivide(K)
    return _grid_map(og, L)


def _compare(program, hm, O, D, t_max, what, t_min=0.0, surface="cube", pose_numbers=None, **kw):
    exe, d = program
    Dn = normalize_directions(D)
    got = run_host_program(exe, d, hm, O, Dn, t_min, t_max, surface, pose_numbers=pose_numbers, **kw)
    cube, count = leaves_of(hm.nodes, host_counts(hm, pose_numbers))
    planes = hm.leaf_planes(pose_numbers) if surface == "plane" else None
    ref = raycast_np(O, Dn, t_max, *cube, t_min=t_min, count=count, planes=planes, surface=surface, **kw)
    assert_hits_equal(got, ref, what)
    return ref, cube, count


def test_lattice_ties_and_grazing_contacts(program):
    hm = _grid({0: lattice_points()}, 1, 8)
    assert _depths(hm.nodes).max() == 2
    O, D = lattice_rays()
    ref, cube, count = _compare(program, hm, O, D, 6.0, "lattice")
    ties = tie_mask(O, normalize_directions(D), 6.0, cube, count=count)
    print(f"lattice: {len(O)} rays, {ref.hit.mean():.3f} hit, {ties.sum()} with a tie in t")
    assert ties.sum() >= 100 and 0.3 < ref.hit.mean() < 1.0
    _compare(program, hm, O, D, 6.0, "lattice, min_range", t_min=0.25)
    _compare(program, hm, O, D, 0.5, "lattice, short", t_min=0.125, min_points=8)
    _compare(program, hm, O, D, 6.0, "lattice, nothing holds 9", min_points=9)


def test_sparse_grid_with_gaps_at_the_cap(program):
    rng = np.random.default_rng(2)
    vox = np.argwhere(rng.random((14, 14, 3)) < 0.25) * [3, 3, 2] - [20, 20, 2]      # occupied voxels, none adjacent in x, y
    P = np.concatenate([v + rng.random((40, 3)) for v in vox])
    hm = _grid({0: P}, 1, 12)
    O, D = box_rays(rng, [-20, -20, -2], [22, 22, 4], 1500, 120.0)
    ref, _, _ = _compare(program, hm, O, D, RAY_CAP_EDGES, "sparse grid, range at the cap")
    assert 0.1 < ref.hit.mean() < 0.9 and (ref.t[ref.hit] > 100.0).sum() > 50
    _compare(program, hm, O, D, 200.0 + RAY_CAP_EDGES, "sparse grid, the cap from min_range", t_min=200.0)
    # above the cap the device form finds nothing (the host form refuses)
    exe, d = program
    over = run_host_program(exe, d, hm, O[:50], normalize_directions(D[:50]), 0.0, np.nextafter(RAY_CAP_EDGES, 1e9))
    assert np.all(over.node == -1) and np.all(np.isinf(over.t))
    # axis rays along voxel walls and through the gaps
    A = np.repeat(np.array([[-30.0, 1.0, 0.5], [-30.0, -8.0, 1.0], [4.0, 40.0, 0.0], [1.5, 1.5, -40.0]]), 6, axis=0)
    Da = np.tile(DIRECTIONS[np.abs(DIRECTIONS).sum(axis=1) == 1], (4, 1))
    _compare(program, hm, A, Da, 100.0, "sparse grid, axis rays")


def _cube_map(P, corner, edge, K):
    t = OTree(np.asarray(corner, dtype=np.float64), edge)
    t.insert_points(P)
    t.subdivide(K)
    table = tree_leaf_table(t, False)
    leaves = {0: [_Leaf(np.asarray(c, dtype=np.float64), float(e), P[i]) for c, e, i in table]}
    return HostMap(1, float(edge), [(np.asarray(corner, dtype=np.float64), float(edge))], leaves)


def test_non_dyadic_cube_faces_and_splitting_planes(program):
    rng = np.random.default_rng(5)
    c0, e0 = 0.1, 3.3
    P = c0 + rng.random((5000, 3)) * e0 * [1.0, 1.0, 0.3]
    P = P[np.all((P - c0 >= 0) & (P - c0 < e0), axis=1)]
    hm = _cube_map(P, [c0, c0, c0], e0, 20)
    assert _depths(hm.nodes).max() >= 3
    nd = hm.nodes
    inner = np.nonzero(nd["first_child"] >= 0)[0]
    split = nd["corner"][inner] + (nd["edge"][inner] / 2.0)[:, None]             # points on the splitting planes
    O, D = [], []
    for a in range(3):                      # through every face, on the faces, an ulp outside the cube
        for sign, wall in ((1.0, c0), (-1.0, c0 + e0)):
            o = c0 + rng.random((60, 3)) * e0 * [1.0, 1.0, 0.3]
            o[:, a] = wall - sign * 1.0
            d = np.zeros((60, 3))
            d[:, a] = sign
            d[20:40] += rng.normal(0.0, 0.2, (20, 3))
            b = (a + 1) % 3
            o[40:50, b], o[50:55, b], o[55:, b] = c0, np.nextafter(c0, -1.0), np.nextafter(c0 + e0, 9.0)
            o[45:50, b] = c0 + e0
            O.append(o)
            D.append(d)
    S = np.repeat(split[:100], 3, axis=0)
    S[:, 0] -= 5.0
    O.append(S)
    D.append(np.tile(np.array([[1.0, 0, 0], [1.0, 0.3, 0], [1.0, 0, -0.2]]), (100, 1)))
    O, D = np.concatenate(O), np.concatenate(D)
    ref, _, _ = _compare(program, hm, O, D, 1e6, "non-dyadic cube")
    assert 0.3 < ref.hit.mean() < 0.98
    _compare(program, hm, O, D, 2e6, "non-dyadic cube from afar", t_min=3.0)          # (one cube has no cap)
    _compare(program, hm, O, D, 9.0, "non-dyadic cube, planes", surface="plane", min_points=5)


def test_utm_offsets_random_rays_both_surfaces_and_an_unsplit_voxel(program):
    rng = np.random.default_rng(7)
    off = np.array([5.0e6, 4.0e5, 100.0])
    U = synthetic.planar_cloud(6000, (3, 3, 2), seed=9) + off
    hm = _grid({0: U[:4000], 1: U[4000:]}, 1, 32)
    assert _depths(hm.nodes).max() >= 2
    O, D = box_rays(rng, off, off + [3, 3, 2], 2000, 2.0)
    O[:200] = np.floor(O[:200])                                                      # on voxel walls
    D[:100] = DIRECTIONS[rng.integers(0, len(DIRECTIONS), 100)]
    cube, _, _ = _compare(program, hm, O, D, 8.0, "utm, cube")
    assert cube.hit.mean() >= 0.25 and (~cube.hit).mean() >= 0.25
    plane, _, _ = _compare(program, hm, O, D, 8.0, "utm, plane", surface="plane", max_variance=1e-3)
    later = plane.hit & (plane.node != cube.node)
    print(f"utm: cube {cube.hit.mean():.3f} hit, plane {plane.hit.mean():.3f}, {later.sum()} rays pass a rejected leaf")
    assert later.sum() >= 100
    one, _, _ = _compare(program, hm, O, D, 8.0, "utm, pose 1", pose_numbers=[1], min_points=2)
    assert not np.array_equal(one.node, cube.node)
    # one voxel of 5 000 points, never subdivided: a root that is a leaf
    B = rng.random((5000, 3))
    h0 = _grid({0: B}, 1, 10 ** 6)
    assert len(h0.nodes["edge"]) == 1
    O0, D0 = box_rays(rng, [0, 0, 0], [1, 1, 1], 300, 2.0)
    r0, _, _ = _compare(program, h0, O0, D0, 5.0, "one unsplit voxel")
    assert r0.hit.any() and not r0.hit.all()
    _compare(program, h0, O0, D0, 5.0, "one unsplit voxel, plane", surface="plane")
