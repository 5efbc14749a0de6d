"""query.prune_np - the definition of prune() and the oracle of the device tests - on hand-made tables where the answer
is written out here (tests/_prune_cases.py numbers the nodes: roots first, then level by level), and
RayEvidence.remapped."""

import numpy as np
import pytest

from octreelib_amd.query import PruneResult, RayEvidence, prune_np

from tests._prune_cases import CASES

A = lambda *parts: np.concatenate([np.atleast_1d(np.asarray(p, dtype=np.int64)) for p in parts])
R = lambda a, b: np.arange(a, b + 1)            # inclusive, as the ranges are written in the comments


def run(name):
    nodes, blocks, _segs, mode = CASES[name]
    before = ({k: v.copy() for k, v in nodes.items()}, {k: v.copy() for k, v in blocks.items()})
    out = prune_np(nodes, blocks, mode)
    for k in nodes:                                   # (the inputs are not written)
        assert np.array_equal(nodes[k], before[0][k])
    for k in blocks:
        assert np.array_equal(blocks[k], before[1][k])
    check_invariants(nodes, blocks, mode, out)
    return nodes, blocks, out


def check_invariants(nodes, blocks, mode, out):
    """What holds for every prune whatever the case."""
    new, o = out.nodes, out.old_node.astype(np.int64)
    n = len(o)
    assert all(len(new[k]) == n for k in new)
    assert np.all(np.diff(o) > 0)                                           # stable
    assert np.array_equal(out.node_map[o], np.arange(n))                    # a kept node maps to itself
    for k in ("depth", "edge"):
        assert new[k].tobytes() == nodes[k][o].tobytes()
    assert new["corner"].tobytes() == nodes["corner"][o].tobytes()
    V2 = int(np.count_nonzero(out.voxel_keep))
    assert np.array_equal(np.nonzero(new["parent"] < 0)[0], np.arange(V2))  # roots are the first V' nodes ...
    assert np.array_equal(new["voxel"][:V2], np.arange(V2))                 # ... in voxel order
    internal = np.nonzero(new["first_child"] >= 0)[0]
    for i in internal.tolist():                                             # eight consecutive children, all there
        c = int(new["first_child"][i])
        assert c + 8 <= n and np.all(new["parent"][c:c + 8] == i) and np.all(new["voxel"][c:c + 8] == new["voxel"][i])
    assert np.array_equal(new["epoch"][internal], nodes["epoch"][o][internal])
    assert np.all(new["epoch"][new["first_child"] < 0] == 0)
    for k in ("slot", "start", "size"):
        assert np.array_equal(out.blocks[k], blocks[k])
    assert np.all(out.blocks["node"] >= 0) and np.array_equal(o[out.blocks["node"]], blocks["node"])
    assert np.all(new["first_child"][out.blocks["node"]] < 0)               # blocks sit in leaves
    # the containing node: its cube holds the old node's cube
    m = out.node_map
    for i in np.nonzero(m >= 0)[0].tolist():
        c, e = new["corner"][m[i]], new["edge"][m[i]]
        assert np.all(nodes["corner"][i] >= c) and np.all(nodes["corner"][i] + nodes["edge"][i] <= c + e)
    gone_voxels = np.nonzero(~out.voxel_keep)[0]
    assert np.array_equal(m < 0, np.isin(nodes["voxel"], gone_voxels))
    if mode == 1:
        assert n >= 1 and out.voxel_keep.all()


def test_nothing_empty_is_the_identity():
    nodes, blocks, out = run("nothing_empty")
    N = len(nodes["parent"])
    assert np.array_equal(out.node_map, np.arange(N)) and np.array_equal(out.old_node, np.arange(N))
    assert out.collapsed == 0 and out.voxel_keep.all()
    for k in nodes:
        assert out.nodes[k].tobytes() == nodes[k].tobytes() and out.nodes[k].dtype == nodes[k].dtype
    assert np.array_equal(out.blocks["node"], blocks["node"])


def test_everything_empty_grid_leaves_no_voxel_and_no_node():
    nodes, _, out = run("all_empty_grid")
    assert len(out.old_node) == 0 and not out.voxel_keep.any() and out.collapsed == 0
    assert np.array_equal(out.node_map, np.full(len(nodes["parent"]), -1))
    assert all(len(v) == 0 for v in out.nodes.values()) and out.nodes["corner"].shape == (0, 3)


def test_everything_empty_cube_leaves_the_bare_root():
    nodes, _, out = run("all_empty_cube")
    assert len(nodes["parent"]) == 25
    assert np.array_equal(out.old_node, [0]) and out.collapsed == 1 and np.array_equal(out.voxel_keep, [True])
    assert np.array_equal(out.node_map, np.zeros(25))
    assert out.nodes["first_child"][0] == -1 and out.nodes["epoch"][0] == 0 and out.nodes["parent"][0] == -1


def test_empty_voxel_between_two_full_ones():
    _, blocks, out = run("empty_voxel_between")
    assert np.array_equal(out.node_map, [0, -1, 1]) and np.array_equal(out.old_node, [0, 2])
    assert np.array_equal(out.voxel_keep, [True, False, True]) and np.array_equal(out.nodes["voxel"], [0, 1])
    assert np.array_equal(out.nodes["corner"][:, 0], [0.0, 2.0])
    assert np.array_equal(out.blocks["node"], np.where(blocks["node"] == 2, 1, 0))


def test_empty_tree_between_two_full_ones():
    nodes, _, out = run("empty_tree_between")
    # roots 0 1 2; voxel 0's children 3..10; voxel 1 (a chain of two empty levels): 11..18, then 19..26
    assert len(nodes["parent"]) == 27
    assert np.array_equal(out.node_map, A(0, -1, 1, R(2, 9), [-1] * 16))
    assert np.array_equal(out.nodes["first_child"], A(2, -1, [-1] * 8)) and out.collapsed == 0


def test_internal_node_with_eight_empty_children_collapses_at_depth_1():
    nodes, _, out = run("collapse_depth1")
    # root 0, children 1..8, node 2 internal over the empty 9..16
    assert np.array_equal(out.old_node, R(0, 8)) and out.collapsed == 1
    assert np.array_equal(out.node_map, A(R(0, 8), [2] * 8))
    assert np.array_equal(out.nodes["first_child"], A(1, [-1] * 8))
    assert nodes["epoch"][2] == 1 and np.array_equal(out.nodes["epoch"], A(1, [0] * 8))


def test_internal_node_with_eight_empty_children_collapses_at_depth_3():
    nodes, _, out = run("collapse_depth3")
    # 0 | 1..8 | 9..16 under 2 | 17..24 under 9 | 25..32 under 17 (empty); a block in 1 and in 18
    assert len(nodes["parent"]) == 33 and nodes["depth"][17] == 3 and nodes["first_child"][17] == 25
    assert np.array_equal(out.old_node, R(0, 24)) and out.collapsed == 1
    assert np.array_equal(out.node_map, A(R(0, 24), [17] * 8))
    fc = np.full(25, -1)
    fc[[0, 2, 9]] = [1, 9, 17]
    assert np.array_equal(out.nodes["first_child"], fc)
    assert np.array_equal(np.nonzero(out.nodes["epoch"])[0], [0, 2, 9])


def test_empty_subtree_under_an_occupied_sibling_stays_as_a_leaf():
    nodes, _, out = run("empty_subtree_beside_occupied")
    # roots 0 1 2; 3..10 under 0; 11..18 under 3 (full); 19..26 under 4 (empty): 4 stays - the eight go together
    assert len(nodes["parent"]) == 27
    assert np.array_equal(out.old_node, A(0, 2, R(3, 10), R(11, 18))) and out.collapsed == 1
    assert np.array_equal(out.node_map, A(0, -1, 1, R(2, 9), R(10, 17), [3] * 8))
    assert np.array_equal(out.nodes["first_child"], A(2, -1, 10, [-1] * 15))
    assert np.array_equal(out.nodes["parent"], A(-1, -1, [0] * 8, [2] * 8))
    assert np.array_equal(out.nodes["voxel"], A(0, 1, [0] * 16))
    assert np.array_equal(out.voxel_keep, [True, False, True])


def test_two_level_ranges_of_the_same_depth():
    nodes, _, out = run("two_segments_per_depth")
    # roots 0..4 | build 0: 5..12 under 0, 13..20 under 4, 21..28 under 13 | build 1: 29..36 under 1, 37..44 under 3,
    # 45..52 under 29 (empty), 53..60 under 37
    assert len(nodes["parent"]) == 61
    assert np.array_equal(out.old_node, A(0, 1, 4, R(5, 36))) and out.collapsed == 1
    assert np.array_equal(out.node_map, A(0, 1, -1, -1, 2, R(3, 34), [-1] * 8, [27] * 8, [-1] * 8))
    fc = np.full(35, -1)
    fc[[0, 1, 2, 11]] = [3, 27, 11, 19]
    assert np.array_equal(out.nodes["first_child"], fc)
    assert np.array_equal(out.nodes["depth"], A([0] * 3, [1] * 16, [2] * 8, [1] * 8))   # ranges stay ranges
    assert np.array_equal(out.nodes["epoch"][[0, 1, 2, 11, 27]], [1, 2, 1, 1, 0])


def test_node_map_of_a_node_two_levels_under_a_collapsed_ancestor():
    nodes, _, out = run("two_levels_under_collapsed")
    # 0 | 1..8 | 9..16 under 2 | 17..24 under 9 | 25..32 under 17; the only block is in 1: 2 collapses
    assert nodes["parent"][17] == 9 and nodes["parent"][9] == 2
    assert np.array_equal(out.old_node, R(0, 8)) and out.collapsed == 1
    assert out.node_map[17] == 2 and out.node_map[9] == 2 and out.node_map[25] == 2
    assert np.array_equal(out.node_map, A(R(0, 8), [2] * 24))


def test_cube_keeps_its_root_and_the_occupied_branch():
    _, _, out = run("cube_one_leaf")
    # 0 | 1..8 | 9..16 under 1 | 17..24 under 9; blocks in 8
    assert np.array_equal(out.old_node, R(0, 8)) and out.collapsed == 1
    assert np.array_equal(out.node_map, A(R(0, 8), [1] * 16))


def test_ray_evidence_remapped():
    _, _, out = run("empty_subtree_beside_occupied")
    N = len(out.node_map)
    ev = RayEvidence(np.arange(N, dtype=np.uint32) * 3 + 1, np.arange(N, dtype=np.uint32) + 100)
    res = PruneResult(out.node_map, out.old_node, len(out.old_node), 2, N - len(out.old_node), 1, out.collapsed)
    got = ev.remapped(res)
    assert len(got) == len(out.old_node) and got.through.dtype == np.uint32 and got.hits.dtype == np.uint32
    assert np.array_equal(got.through, ev.through[out.old_node]) and np.array_equal(got.hits, ev.hits[out.old_node])
    assert got.through[3] == 3 * 4 + 1       # (the collapsed node keeps ITS counters - zero in real evidence: it was internal)
    assert np.array_equal(ev.through, np.arange(N, dtype=np.uint32) * 3 + 1)   # (not written)
    with pytest.raises(ValueError, match="evidence over"):
        RayEvidence(ev.through[:-1], ev.hits[:-1]).remapped(res)
