"""tests/_maskmodel.py against oracle/octree_np.py on a small two-pose scene: the model that the GPU tests of the
compaction kernels (tests/test_gpu_apply_mask.py) compare with is anchored to the oracle's apply_mask / filter - the
same leaves, the same points in the same order - and not to the kernels.  Needs no GPU."""

import numpy as np
import pytest

from oracle import octree_np as onp
from tests._maskmodel import INT64_MAX, apply_mask_model, check_tables, filter_count_model

K = 12


def _scene():
    rng = np.random.default_rng(11)
    clouds = [rng.random((300, 3)) * (2, 2, 1), rng.random((260, 3)) * (2, 1, 1) + (0, 0.5, 0)]
    g = onp.OGrid(1)
    for p, c in enumerate(clouds):
        g.insert_points(p, c)
    g.subdivide(K)
    return g, clouds


def _key(corner, edge):
    return (tuple((np.asarray(corner, dtype=np.float64) + 0.0).tolist()), float(edge))


def _tables_of(g, clouds):
    """The oracle's state as the flat tables of the library: one block per non-empty (leaf, pose), leaf-major and
    pose-minor; perm = index into the concatenation of the clouds; plus, per pose, the oracle's listing rank of every
    leaf (the order in which its apply_mask consumes a mask)."""
    off = np.concatenate(([0], np.cumsum([len(c) for c in clouds])))
    leaves = [g.leaf_table(p, non_empty=False) for p in range(len(clouds))]
    keys = sorted({_key(c, e) for tab in leaves for c, e, _ in tab})
    node_of = {k: i for i, k in enumerate(keys)}
    rank = [{node_of[_key(c, e)]: r for r, (c, e, _) in enumerate(tab)} for tab in leaves]
    rows = []
    for p, tab in enumerate(leaves):
        for c, e, idx in tab:
            if len(idx):
                rows.append((node_of[_key(c, e)], p, idx))
    rows.sort(key=lambda r: (r[0], r[1]))
    size = np.array([len(r[2]) for r in rows], dtype=np.int32)
    blocks = {
        "node": np.array([r[0] for r in rows], dtype=np.int32),
        "slot": np.array([r[1] for r in rows], dtype=np.int32),
        "start": (np.cumsum(size) - size).astype(np.int64),
        "size": size,
    }
    perm = np.concatenate([off[r[1]] + r[2] for r in rows]).astype(np.int64)
    xyz = np.vstack(clouds)[perm]
    check_tables(blocks, perm, xyz)
    return blocks, perm, xyz, off, rank, keys


def _pose_mask(blocks, mask, rank, pose):
    """The bytes of a storage-position mask in the order the oracle consumes them for one pose."""
    ids = [b for b in range(len(blocks["node"])) if blocks["slot"][b] == pose]
    ids.sort(key=lambda b: rank[pose][int(blocks["node"][b])])
    parts = [mask[blocks["start"][b] : blocks["start"][b] + blocks["size"][b]] for b in ids]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def _listing(blocks, perm, off, rank, keys, pose):
    ids = [b for b in range(len(blocks["node"])) if blocks["slot"][b] == pose]
    ids.sort(key=lambda b: rank[pose][int(blocks["node"][b])])
    return [(keys[int(blocks["node"][b])],
             (perm[blocks["start"][b] : blocks["start"][b] + blocks["size"][b]] - off[pose]).tolist()) for b in ids]


def _oracle_listing(g, pose):
    return [(_key(c, e), idx.tolist()) for c, e, idx in g.leaf_table(pose, non_empty=True)]


def _assert_model_is_oracle(g, clouds, got, off, rank, keys):
    blocks, perm, xyz, n, nb = got
    check_tables(blocks, perm, xyz)
    assert n == len(perm) == sum(g.n_points(p) for p in range(len(clouds)))
    assert nb == len(blocks["node"]) == sum(g.n_leaves(p) for p in range(len(clouds)))
    assert xyz.tobytes() == np.vstack(clouds)[perm].tobytes()
    for p in range(len(clouds)):
        assert _listing(blocks, perm, off, rank, keys, p) == _oracle_listing(g, p)


@pytest.mark.parametrize("content", ["half", "sparse", "dense", "ones", "zeros", "bytes"])
def test_apply_mask_model_equals_the_oracle(content):
    g, clouds = _scene()
    blocks, perm, xyz, off, rank, keys = _tables_of(g, clouds)
    assert len(np.unique(blocks["slot"])) == 2 and len(blocks["node"]) > 40
    assert not np.array_equal(perm, np.arange(len(perm)))
    rng = np.random.default_rng(5)
    n = len(perm)
    mask = {
        "half": lambda: (rng.random(n) < 0.5).astype(np.uint8),
        "sparse": lambda: (rng.random(n) < 0.05).astype(np.uint8),
        "dense": lambda: (rng.random(n) < 0.95).astype(np.uint8),
        "ones": lambda: np.ones(n, dtype=np.uint8),
        "zeros": lambda: np.zeros(n, dtype=np.uint8),
        "bytes": lambda: rng.choice(np.array([0, 1, 2, 0x7F, 0x80, 0xFF], dtype=np.uint8), n),
    }[content]()
    got = apply_mask_model(blocks, perm, xyz, mask)
    for p in range(len(clouds)):
        g.apply_mask(p, _pose_mask(blocks, mask, rank, p).astype(bool))
    _assert_model_is_oracle(g, clouds, got, off, rank, keys)
    if content == "sparse":
        assert got[4] < len(blocks["node"])        # whole blocks disappeared
    # a second mask, on the compacted tables
    mask2 = (rng.random(got[3]) < 0.6).astype(np.uint8)
    got2 = apply_mask_model(got[0], got[1], got[2], mask2)
    for p in range(len(clouds)):
        g.apply_mask(p, _pose_mask(got[0], mask2, rank, p).astype(bool))
    _assert_model_is_oracle(g, clouds, got2, off, rank, keys)


@pytest.mark.parametrize("slots", [(), (0,), (1,), (0, 1)])
@pytest.mark.parametrize("interval", ["all", "at_least", "below", "empty"])
def test_filter_model_equals_the_oracle(slots, interval):
    g, clouds = _scene()
    blocks, perm, xyz, off, rank, keys = _tables_of(g, clouds)
    c = int(np.sort(blocks["size"])[len(blocks["size"]) // 2])       # a size that blocks have
    lo, hi, crit = {
        "all": (0, INT64_MAX, lambda pts: True),
        "at_least": (c, INT64_MAX, lambda pts: len(pts) >= c),
        "below": (0, c - 1, lambda pts: len(pts) < c),
        "empty": (5, 4, lambda pts: False),
    }[interval]
    sel = np.zeros(len(clouds), dtype=np.uint8)
    sel[list(slots)] = 1
    got = filter_count_model(blocks, perm, xyz, sel, lo, hi)
    for m in g.managers.values():
        m.filter([crit], list(slots))
    _assert_model_is_oracle(g, clouds, got, off, rank, keys)
    if interval in ("at_least", "below") and slots:
        assert 0 < got[3] < len(perm)
    # on top of a pending mask: the filter's clearing and the mask go through one compaction
    g, clouds = _scene()
    rng = np.random.default_rng(9)
    pending = (rng.random(len(perm)) < 0.7).astype(np.uint8)
    got = filter_count_model(blocks, perm, xyz, sel, lo, hi, mask=pending)
    for m in g.managers.values():     # (the filter sees the leaves as they are before the mask is applied)
        m.filter([crit], list(slots))
    for p in range(len(clouds)):
        # leaves the filter emptied are skipped by the oracle's apply_mask: hand it the bytes of the others
        ids = [b for b in range(len(blocks["node"])) if blocks["slot"][b] == p]
        ids.sort(key=lambda b: rank[p][int(blocks["node"][b])])
        parts = [pending[blocks["start"][b] : blocks["start"][b] + blocks["size"][b]] for b in ids
                 if not sel[p] or lo <= blocks["size"][b] <= hi]
        g.apply_mask(p, np.concatenate(parts).astype(bool) if parts else np.zeros(0, dtype=bool))
    _assert_model_is_oracle(g, clouds, got, off, rank, keys)
