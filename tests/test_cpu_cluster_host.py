"""The linking sink of the cluster kernels (octreelib_amd/csrc/cluster_link.h over the walk of nearest_walk.h and the
union-find of union_find.h) compiled for the CPU alone, with AddressSanitizer and UBSan, as the stand-alone program
tests/host/cluster_host.cpp, and compared with cluster_labels_np over host-built maps: root, size and smallest member of
every position exactly.  No GPU and nothing loaded into Python: the program gets tables of exactly their size from a
file, so a lookup outside one or a signed overflow ends it with an error instead of a wrong answer.  It is
single-threaded (the host branch of union_find.h uses plain loads and stores); linking the positions last to first
instead of first to last is the one other schedule it can show.  The test compiles the program once (a few seconds) and
starts it once per case."""

import numpy as np
import pytest

from octreelib_amd.clustering import cluster_labels_np
from oracle.octree_np import OGrid
from tests._cell import lattice01, ulp_neighbours
from tests._cluster import CHAIN_RADIUS, build_host_program, diagonal_chain, run_host_program
from tests.test_cpu_query import _depths, _grid_map
from tests.test_cpu_raycast_host import _cube_map


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("cluster_host")
    return build_host_program(d), d


def _grid(clouds, L, K):
    og = OGrid(L)
    for p, P in clouds.items():
        og.insert_points(p, P)
    og.subdivide(K)
    return _grid_map(og, L)


def _compare(program, hm, radius, what, pose_numbers=None):
    """The host build against the definition; returns the sizes of the clusters."""
    exe, d = program
    clouds = hm.clouds(pose_numbers)
    labels, sizes, first = cluster_labels_np(clouds, radius)
    label = np.concatenate(labels)
    assert (label >= 0).all()
    every = hm.clouds()
    off = np.concatenate([[0], np.cumsum([len(c) for _, c in every])]).astype(np.int64)
    place = {p: i for i, (p, _) in enumerate(clouds)}            # pose number -> position in the selection
    slot_place = np.array([place.get(p, -1) for p, _ in every])  # slot of the store -> position in the selection
    sel_off = np.concatenate([[0], np.cumsum([len(c) for _, c in clouds])]).astype(np.int64)
    for rev in (False, True):
        root, size, smallest, t = run_host_program(exe, d, hm, radius, pose_numbers, reversed_order=rev)
        n = len(root)
        assert n == len(label), what
        # the point of every position: (position of its pose in the selection, row)
        slot = np.repeat(t["rec"][:, 2].astype(np.int64), t["rec"][:, 1].astype(np.int64))
        row = t["ord_idx"].astype(np.int64) - off[slot]
        assert (slot_place[slot] >= 0).all()
        at = sel_off[slot_place[slot]] + row                      # its row in the definition's answer
        got_first = np.stack([slot_place[(smallest >> np.uint64(32)).astype(np.int64)],
                              (smallest & np.uint64(0xffffffff)).astype(np.int64)
                              - off[(smallest >> np.uint64(32)).astype(np.int64)]], axis=1)
        assert np.array_equal(size.astype(np.int64), sizes[label[at]]), (what, rev)
        assert np.array_equal(got_first, first[label[at]]), (what, rev)
        # the root of a component is its smallest POSITION, whatever the order of the unions
        assert (root <= np.arange(n)).all() and np.array_equal(root[root], root), (what, rev)
        for c in np.unique(label[at])[:50]:
            members = np.nonzero(label[at] == c)[0]
            assert (root[members] == members.min()).all(), (what, rev, int(c))
    return sizes


def test_the_chain_across_walls_and_poses(program):
    P = diagonal_chain()
    rng = np.random.default_rng(1)
    far = rng.random((200, 3)) * 0.5 + [2.0, -2.0, 1.0]
    hm = _grid({0: np.concatenate([P[0::3], far[:100]]), 1: P[1::3], 2: np.concatenate([far[100:], P[2::3]])}, 1, 4)
    assert _depths(hm.nodes).max() >= 2
    sizes = _compare(program, hm, CHAIN_RADIUS, "chain")
    assert 41 in sizes and 19 in sizes
    # without pose 1 every third link is missing: the chain falls into pairs
    sizes = _compare(program, hm, CHAIN_RADIUS, "chain, poses 0 and 2", pose_numbers=[0, 2])
    assert np.count_nonzero(sizes == 2) >= 18 and 41 not in sizes


def test_the_lattice_and_an_ulp_either_side(program):
    P, _ = lattice01(-4, 4)
    up, down = ulp_neighbours(P[np.all(P != 0.0, axis=1)])      # (no subnormal coordinates: the host build of the map
    X = np.concatenate([P, up[::5], down[::7]])                 #  places a point by a rounded difference)
    hm = _grid({0: X[::2], 1: X[1::2]}, 1, 8)
    assert _depths(hm.nodes).max() >= 2
    # fl(k 0.1) steps either side of 0.1: pairs of lattice neighbours straddle the sphere of radius 0.1
    s1 = _compare(program, hm, 0.1, "lattice")
    s2 = _compare(program, hm, 0.15, "lattice")
    assert len(s1) > 1 and s2.max() >= s1.max()
    _compare(program, hm, 0.1, "lattice, pose 1", pose_numbers=[1])


def test_a_cube_that_is_not_dyadic(program):
    rng = np.random.default_rng(5)
    c0, e0 = 0.1, 3.3
    blobs = [c0 + e0 * rng.random(3) * [1.0, 1.0, 0.3] + rng.normal(0.0, 0.03, (int(m), 3))
             for m in rng.integers(1, 60, 80)]
    P = np.concatenate(blobs)
    P = P[np.all((P - c0 >= 0) & (P - c0 < e0), axis=1)]
    P = np.concatenate([P, P[:50]])                                             # duplicates
    hm = _cube_map(P, [c0, c0, c0], e0, 20)
    assert _depths(hm.nodes).max() >= 2
    for r in (0.02, 0.08, 5.0):                                                 # (one cube has no cap on the radius)
        sizes = _compare(program, hm, r, "non-dyadic cube")
    assert len(sizes) == 1 and sizes[0] == len(P)
