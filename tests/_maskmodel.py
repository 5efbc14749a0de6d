"""A plain NumPy statement of what apply_mask / filter_count leave behind (include/octreelib_hip.h:
octl_forest_apply_mask, octl_forest_apply_host_mask, octl_forest_filter_count), for the tests that compare the
compaction kernels with it.  Anchored to oracle/octree_np.py by tests/test_cpu_mask_model.py, never to the kernels."""

import numpy as np

INT64_MAX = (1 << 63) - 1


def _tables(blocks):
    return (np.asarray(blocks["node"], dtype=np.int64), np.asarray(blocks["slot"], dtype=np.int64),
            np.asarray(blocks["start"], dtype=np.int64), np.asarray(blocks["size"], dtype=np.int64))


def check_tables(blocks, perm, xyz):
    """The block table describes the leaf-ordered arrays exactly: blocks are non-empty, lie one behind the other
    and cover every storage position."""
    node, slot, start, size = _tables(blocks)
    assert len(node) == len(slot) == len(start) == len(size)
    assert (size > 0).all()
    assert np.array_equal(start, np.cumsum(size) - size)
    assert int(size.sum()) == len(perm) == len(xyz)


def apply_mask_model(blocks, perm, xyz, mask):
    """blocks {node, slot, start, size}, perm (n,), xyz (n,3) before the call and a uint8 mask over storage positions
    -> (blocks', perm', xyz', surviving points, surviving blocks).  A byte of 0 drops the point, any other keeps it."""
    check_tables(blocks, perm, xyz)
    node, slot, start, size = _tables(blocks)
    mask = np.asarray(mask, dtype=np.uint8)
    assert mask.shape == (len(perm),)
    keep = mask != 0
    cs = np.concatenate(([0], np.cumsum(keep, dtype=np.int64)))
    kept = cs[start + size] - cs[start]
    live = kept > 0
    size2 = kept[live]
    out = {
        "node": node[live].astype(np.int32),
        "slot": slot[live].astype(np.int32),
        "start": (np.cumsum(size2) - size2).astype(np.int64),
        "size": size2.astype(np.int32),
    }
    return out, np.asarray(perm)[keep], np.asarray(xyz)[keep], int(keep.sum()), int(live.sum())


def filter_mask_model(blocks, mask, slot_sel, lo, hi):
    """The mask after filter_count's first step: every block whose slot is selected and whose size lies outside
    [lo, hi] has its bytes cleared; the rest of `mask` (a pending RANSAC mask, or all ones) is left as it is."""
    node, slot, start, size = _tables(blocks)
    sel = np.asarray(slot_sel, dtype=np.uint8) != 0
    out = np.array(mask, dtype=np.uint8, copy=True)
    gone = sel[slot] & ~((size >= lo) & (size <= hi))
    per_pos = np.repeat(gone, size)
    assert len(per_pos) == len(out)
    out[per_pos] = 0
    return out


def filter_count_model(blocks, perm, xyz, slot_sel, lo, hi, mask=None):
    """filter_count as a whole: the filter's clearing on top of `mask` (None: all ones), then ONE compaction."""
    n = len(perm)
    base = np.ones(n, dtype=np.uint8) if mask is None else mask
    return apply_mask_model(blocks, perm, xyz, filter_mask_model(blocks, base, slot_sel, lo, hi))
