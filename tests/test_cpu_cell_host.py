"""The walk of the cell kernels (octreelib_amd/csrc/cell_walk.h: the voxels a cell touches, the stackless traversal,
the box prune, membership by fused remainders) compiled for the CPU alone, with AddressSanitizer and UBSan, as the
stand-alone program tests/host/cell_host.cpp, and compared with cell_count_np and thin's rank count for count over
host-built maps.  No GPU and nothing loaded into Python: the program gets tables of exactly their size from a file, so
a lookup outside one, a signed overflow or a bad conversion ends it with an error instead of a wrong answer.  This is
where a wrong box prune shows without a GPU.  The test compiles the program once (a few seconds) and starts it once
per case."""

import numpy as np
import pytest

from octreelib_amd import cell_count_np
from octreelib_amd.thinning import thin_ranks_np
from oracle.octree_np import OGrid
from tests._cell import CAPS, CELL, build_host_program, host_tables, lattice01, run_host_program, ulp_neighbours
from tests.test_cpu_query import _depths, _grid_map
from tests.test_cpu_raycast_host import _cube_map

BAD = np.array([[1e300, 0.0, 0.0], [0.0, -2.0 ** 31, 0.0], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf],
                [-777.5, 3.0, 3.0]])


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("cell_host")
    return build_host_program(d), d


def _grid(clouds, L, K):
    og = OGrid(L)
    for p, P in clouds.items():
        og.insert_points(p, P)
    og.subdivide(K)
    return _grid_map(og, L)


def _compare(program, hm, Q, cell, what, pose_numbers=None, caps=CAPS):
    exe, d = program
    clouds = hm.clouds(pose_numbers)
    ref = cell_count_np(Q, clouds, cell)
    tables = host_tables(hm, pose_numbers)
    for cap in caps:
        got = run_host_program(exe, d, hm, Q, cell, cap, tables=tables)
        want = ref if cap is None else np.minimum(ref, cap)
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            raise AssertionError(f"{what}, cell={cell}, cap={cap}: {len(bad)} of {len(Q)} counts differ, first "
                                 f"{int(bad[0])} at {Q[bad[0]].tolist()}: got {int(got[bad[0]])}, expected "
                                 f"{int(want[bad[0]])}")
    return ref


def _compare_ranks(program, hm, cell, what):
    """The rank of every stored point (thin with every pose tested and counted) against thin_ranks_np."""
    exe, d = program
    t = host_tables(hm)
    ranks = np.concatenate(thin_ranks_np(hm.clouds(), None, cell))                  # by store index
    got = run_host_program(exe, d, hm, t["xyz_ord"], cell, below=t["ord_idx"], tables=t)
    assert np.array_equal(got, ranks[t["ord_idx"].astype(np.int64)]), what
    return got


def test_the_lattice_and_an_ulp_either_side(program):
    P, _ = lattice01()
    hm = _grid({0: P[::2], 1: P[1::2]}, 1, 8)
    assert _depths(hm.nodes).max() >= 2
    up, down = ulp_neighbours(P)
    Q = np.concatenate([P, up[::3], down[::3], np.column_stack([up[::5, 0], P[::5, 1], down[::5, 2]]), BAD])
    ref = _compare(program, hm, Q, CELL, "lattice")
    assert ref.max() > 1 and (ref[:len(P)] >= 1).all() and np.all(ref[-len(BAD):] == 0)
    _compare(program, hm, Q[::4], CELL, "lattice, pose 1", pose_numbers=[1], caps=(None, 1))
    r = _compare_ranks(program, hm, CELL, "lattice ranks")
    assert (r > 0).any() and (r == 0).any()


def test_a_grid_with_missing_voxels_cells_of_every_size(program):
    rng = np.random.default_rng(2)
    vox = np.argwhere(rng.random((5, 5, 3)) < 0.45) - [2, 2, 1]                      # occupied voxels with gaps, negative too
    P = np.concatenate([v + rng.random((60, 3)) for v in vox])
    P[:300:3] = np.floor(P[:300:3] * 8) / 8                                        # on leaf and voxel walls
    hm = _grid({0: P[::2], 1: P[1::2]}, 1, 10)
    depth = _depths(hm.nodes)
    assert depth.max() >= 2 and len(vox) < 5 * 5 * 3
    smallest = hm.nodes["edge"].min()
    Q = np.concatenate([P[::2] + rng.normal(0.0, 0.02, (len(P[::2]), 3)), P[:200], rng.uniform(-3.0, 4.0, (400, 3)),
                        np.floor(P[:100]), np.floor(P[:100]) + [0.0, 0.5, 1.0], BAD])
    # larger than the leaves (the voxel edge itself), straddling voxel walls, the lattice's, smaller than the deepest leaf
    for cell in (1.0, 0.7, 0.3, CELL, smallest / 4.0, 0.07):
        ref = _compare(program, hm, Q, cell, "sparse grid", caps=(None, 3))
        assert ref.sum() > 0 and (ref == 0).any()
    assert _compare(program, hm, Q, 1.0, "sparse grid").max() >= 60
    _compare(program, hm, Q, 0.7, "sparse grid, pose 0", pose_numbers=[0], caps=(None, 1))
    for cell in (0.7, 0.125):
        _compare_ranks(program, hm, cell, f"sparse grid ranks {cell}")


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
    Q = np.concatenate([P[:600] + rng.normal(0.0, 0.01, (600, 3)), P[:200], split[:200], np.nextafter(split[:100], -9.0),
                        rng.uniform(-0.5, 4.0, (300, 3)), BAD])
    for cell in (1.0, 0.7, CELL, 0.01):
        ref = _compare(program, hm, Q, cell, "non-dyadic cube", caps=(None, 7))
        assert ref.sum() > 0 and (ref == 0).any()
    _compare_ranks(program, hm, 0.3, "non-dyadic cube ranks")
