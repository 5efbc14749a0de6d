"""Hand-made forests for the prune tests (test_cpu_prune.py, test_cpu_prune_host.py): a node table numbered as the
library numbers it - roots [0, V) in voxel order, then level by level, the eight children of a node consecutive - a
block table and the level ranges, from a nested description.

A tree is an int (a leaf holding that many blocks, 0: empty) or a list of eight trees (an internal node; child
4 ix + 2 iy + iz).  `groups` splits the voxels into builds: the descendants of the voxels of group 0 are numbered level by
level first, then those of group 1 (a scheme extended by late voxels: two level ranges of the same depth)."""

import numpy as np

E8 = [0] * 8                      # eight empty leaves


def full(k=1):
    return [k] * 8                # eight leaves of k blocks


def make_forest(trees, groups=None, mode=0):
    V = len(trees)
    groups = [0] * V if groups is None else list(groups)
    voxel, depth, parent, first_child, epoch, corner, edge = [], [], [], [], [], [], []
    spec = []
    for v, t in enumerate(trees):
        voxel.append(v); depth.append(0); parent.append(-1); first_child.append(-1); epoch.append(0)
        corner.append((float(v), 0.0, 0.0)); edge.append(1.0); spec.append(t)
    segs = [(0, V, 0)]
    for g in sorted(set(groups)):
        level = [v for v in range(V) if groups[v] == g]
        d = 0
        while True:
            nxt = []
            a = len(voxel)
            for n in level:
                if not isinstance(spec[n], list):
                    continue
                assert len(spec[n]) == 8
                first_child[n] = len(voxel)
                epoch[n] = 1 + g
                for j, child in enumerate(spec[n]):
                    ix, iy, iz = (j >> 2) & 1, (j >> 1) & 1, j & 1
                    h = edge[n] / 2.0
                    nxt.append(len(voxel))
                    voxel.append(voxel[n]); depth.append(d + 1); parent.append(n); first_child.append(-1)
                    epoch.append(0); edge.append(h)
                    corner.append((corner[n][0] + ix * h, corner[n][1] + iy * h, corner[n][2] + iz * h))
                    spec.append(child)
            if not nxt:
                break
            d += 1
            segs.append((a, len(voxel), d))
            level = nxt
    node, slot, size = [], [], []
    for n, t in enumerate(spec):
        if not isinstance(t, list):
            for s in range(t):
                node.append(n); slot.append(s); size.append(3 + (n + s) % 4)
    # (blocks in storage order: shuffled deterministically, so that a block's position says nothing about its node)
    order = np.random.default_rng(len(node)).permutation(len(node))
    node, slot, size = (np.asarray(a, dtype=np.int32)[order] for a in (node, slot, size))
    start = (np.cumsum(size) - size).astype(np.int64)
    nodes = {"voxel": np.asarray(voxel, dtype=np.int32), "depth": np.asarray(depth, dtype=np.int32),
             "parent": np.asarray(parent, dtype=np.int32), "first_child": np.asarray(first_child, dtype=np.int32),
             "corner": np.asarray(corner, dtype=np.float64).reshape(-1, 3), "edge": np.asarray(edge, dtype=np.float64),
             "epoch": np.asarray(epoch, dtype=np.int32)}
    blocks = {"node": node, "slot": slot, "start": start, "size": size}
    return nodes, blocks, segs, mode


def deep(levels, leaf):
    """A chain: `levels` internal nodes, the first child split every time, `leaf` at the bottom, empty leaves beside."""
    t = leaf
    for _ in range(levels):
        t = [t] + [0] * 7
    return t


CASES = {
    "nothing_empty": make_forest([full(), 2, [1, 1, 1, 1, full(), 1, 1, 1]]),
    "all_empty_grid": make_forest([0, E8, deep(3, 0)]),
    "all_empty_cube": make_forest([deep(3, 0)], mode=1),
    "empty_voxel_between": make_forest([1, 0, 2]),
    "empty_tree_between": make_forest([full(), deep(2, 0), 1]),
    "collapse_depth1": make_forest([[1, E8, 1, 0, 0, 0, 0, 0]]),
    "collapse_depth3": make_forest([[1, [[E8, 1, 0, 0, 0, 0, 0, 0], 0, 0, 0, 0, 0, 0, 0], 0, 0, 0, 0, 0, 0]]),
    "empty_subtree_beside_occupied": make_forest([[full(), E8, 0, 0, 0, 0, 0, 0], 0, 1]),
    "two_segments_per_depth": make_forest([full(), [E8, 1, 0, 0, 0, 0, 0, 0], 0, deep(2, 0), [full(), 0, 0, 0, 0, 0, 0, 1]],
                                          groups=[0, 1, 0, 1, 0]),
    "two_levels_under_collapsed": make_forest([[1, [[E8, 0, 0, 0, 0, 0, 0, 0], 0, 0, 0, 0, 0, 0, 0], 0, 0, 0, 0, 0, 0]]),
    "cube_one_leaf": make_forest([[deep(2, 0), 0, 0, 0, 0, 0, 0, 3]], mode=1),
}


def random_forest(rng):
    def tree(d):
        if d < 3 and rng.random() < (0.7 if d == 0 else 0.35):
            return [tree(d + 1) for _ in range(8)]
        return int(rng.integers(0, 3)) if rng.random() < 0.5 else 0
    mode = int(rng.random() < 0.25)
    V = 1 if mode else int(rng.integers(1, 7))
    groups = None if mode or rng.random() < 0.5 else rng.integers(0, 2, V).tolist()
    if groups is not None and 0 not in groups:
        groups = None
    return make_forest([tree(0) for _ in range(V)], groups, mode)
