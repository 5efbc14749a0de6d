"""Directed blocks for what the one-wave instance of k_ransac (csrc/ransac.hip) rearranged to run five waves per SIMD:
the survivor list of the prescreen, which now lies in the s_loc buffer of the next block, and the next block's
prefetched point, which is parked in LDS in front of the survivors' exact fits and read back by the staging.

Every launch is evaluated with the prescreen on and with NO_RANSAC_PRESCREEN=1, and both are compared with the oracle:
mask, f32 plane bits, count and winner index, exactly.  The tables and blocks are crafted.  Every draw of a table is the
centre of a position of the block size it is made for ((g + 0.5) / n), so a row samples the same positions wherever the
block starts in the cloud.

A crafted block of n points (threshold 0.01):
  positions 0 .. n-3   core points on one plane, the first four spread over a square
  position n-2         the lifted point: over the centre of the first four, 0.012 off the plane
  position n-1         junk, half a unit off the plane
and the rows of its table:
  poor     (rows 0 .. 63) the junk point and five draws among the core points: a tilted plane that holds few points
  medium   the first four core points: the plane itself, which holds the n - 2 core points
  best     the first four and twice the lifted point: the plane raised by 0.004, which holds the lifted point too (n - 1)
  copy     a copy of ONE poor row: the one that holds the fewest points inside 1.25 times the threshold
A table for K surviving hypotheses has K - 1 medium rows from row 64 on, the best row behind them and copies in every
other row: the K rows beat group 0 and survive the prescreen, the best row - the LAST survivor - wins, so a list that
loses or misplaces its last entries shows in the winner index.  A copy row does not survive: the prescreen counts inside
a threshold widened by at most an eighth for the block's part of its bound (prescreen_constants refuses blocks beyond)
and by far less for the part of a well-conditioned plane, and the copied row holds no more points inside 1.25 times the
threshold than the best row of group 0 holds inside the threshold.  The claims (the best count of group 0, the count of
every medium and best row, the copied row's widened count) are asserted through the oracle's counts.
"""

import numpy as np
import pytest

from octreelib_amd.ransac import CudaRansac
from oracle import ransac_np as rnp
from tests._util import set_option

THR = 0.01
H = 1024
# none, one, the batch boundary, mid-list (the boundary of a list of 256 entries, had it been halved), the list's own
# boundary - 512 survivors fill the s_loc buffer it lies in to its last two bytes, the 513th has no place and sends every
# hypothesis through the exact path - and deep overflow
SURVIVORS = (0, 1, 64, 65, 256, 257, 512, 513, 600)
SIZES = (6, 23, 32, 63)
N_ROT = 20                 # block size of the rotation launch
ROT_BLOCKS = 200_000       # more than three times the largest grid (256 workgroups on each of 256 CUs): four blocks
                           # and more per workgroup, all of one size


def _block(rng, n, kind="crafted"):
    """n points (f64).  crafted: see above.  flat: every point on the plane.  split: positions 0-3, 8-14 and n-1 on
    the plane (what the poor rows of the rotation table draw from), the others a quarter of a unit above it."""
    o = rng.integers(0, 32, 3).astype(np.float64)
    xy = rng.random((n, 2)) * 0.5
    xy[:4] = np.array([[0.05, 0.05], [0.45, 0.08], [0.42, 0.44], [0.07, 0.40]]) + rng.random((4, 2)) * 0.02
    a, b = rng.uniform(-0.3, 0.3, 2)
    z = a * xy[:, 0] + b * xy[:, 1] + 0.05
    if kind == "crafted":
        xy[n - 2] = xy[:4].mean(axis=0)
        z[n - 2] = a * xy[n - 2, 0] + b * xy[n - 2, 1] + 0.05 + 0.012 * np.sqrt(1 + a * a + b * b)
        z[n - 1] += 0.5
    elif kind == "split":
        on = np.zeros(n, dtype=bool)
        on[[0, 1, 2, 3, 8, 9, 10, 11, 12, 13, 14, n - 1]] = True
        z[~on] += 0.25
    return np.column_stack([xy, z]) + o


def _table(rng, n, K, core=None):
    """(H, 6) table for blocks of n points with K survivors on a crafted block (see the module's text)."""
    core = np.arange(n - 2) if core is None else np.asarray(core)
    pos = np.zeros((H, 6), dtype=np.int64)
    for r in range(64):
        others = rng.choice(core[4:], size=min(2, len(core) - 4), replace=False) if len(core) > 4 else []
        draw = list(rng.permutation(4)) + list(rng.choice(4, size=1))     # the first four, one of them twice
        draw = draw[:5 - len(others)] + list(others)
        pos[r] = rng.permutation([n - 1] + draw)
    for r in range(64, H):
        pos[r] = pos[r % 64]
    for r in range(64, 64 + max(K - 1, 0)):
        pos[r] = rng.permutation([0, 1, 2, 3] + list(rng.choice(4, size=2, replace=False)))
    if K >= 1:
        pos[64 + K - 1] = rng.permutation([0, 1, 2, 3, n - 2, n - 2])
    return (pos + 0.5) / n


def _operator(table):
    op = CudaRansac(threshold=THR, hypotheses_number=H, initial_points_number=6)
    op.random_hypotheses[:] = table       # (the operator's own array: edited in place)
    return op


def _evaluate_both(op, cloud, sizes, waves):
    got = {}
    set_option("RANSAC_WAVES", waves)     # (1: blocks under 64 points on the one-wave instance, however few there are)
    for off in (0, 1):
        set_option("NO_RANSAC_PRESCREEN", off)
        got[off] = op.evaluate(cloud, sizes, details=True)
    set_option("NO_RANSAC_PRESCREEN", 0)
    set_option("RANSAC_WAVES", 0)
    return got


def _assert_same(got, oracle, what):
    o_mask, o_count, o_plane, o_index = oracle
    for off in (0, 1):
        mask, planes, counts, index = got[off]
        bad = np.flatnonzero((counts != o_count) | (index != o_index) |
                             (planes.view(np.uint32) != o_plane.view(np.uint32)).any(axis=1))
        assert len(bad) == 0, (what, off, bad[:10].tolist(), counts[bad[:10]].tolist(), o_count[bad[:10]].tolist(),
                               index[bad[:10]].tolist(), o_index[bad[:10]].tolist())
        assert np.array_equal(mask, o_mask), (what, off)


def _row_counts(cloud, sizes, table, rows, thr=THR):
    """exact inlier count of every given row on every block: the oracle's best count of a one-row table"""
    return np.array([rnp.evaluate(cloud, sizes, table[r:r + 1], thr, details=True)[1] for r in rows])


def _group0_best(cloud, sizes, table, thr=THR):
    return rnp.evaluate(cloud, sizes, table[:64], thr, details=True)[1]


_CACHE = {}


def _survivor_case(n, K):
    """one launch: three crafted blocks of n points under a table with K survivors"""
    if (n, K) not in _CACHE:
        rng = np.random.default_rng(1000 * n + K)
        blocks = [_block(rng, n) for _ in range(3)]
        cloud, sizes = np.vstack(blocks), np.full(3, n, dtype=np.int32)
        table = _table(rng, n, K)
        # every other later row: a copy of the poor row with the fewest points inside the widened threshold
        wide = _row_counts(cloud, sizes, table, range(64), 1.25 * THR).max(axis=1)
        src = int(np.argmin(wide))
        table[64 + K:] = table[src]
        oracle = rnp.evaluate(cloud, sizes, table, THR, details=True)[:4]
        _CACHE[(n, K)] = (cloud, sizes, table, oracle, src)
    return _CACHE[(n, K)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("K", SURVIVORS)
def test_survivor_counts(n, K):
    cloud, sizes, table, oracle, src = _survivor_case(n, K)
    # ---- the crafted blocks are what they claim (the oracle's counts) ----
    L = _group0_best(cloud, sizes, table)
    assert (L < n - 2).all(), (n, K, L)
    assert (table[64 + K:] == table[src]).all() and src < 64
    assert (_row_counts(cloud, sizes, table, [src], 1.25 * THR)[0] <= L).all(), (n, K)    # the copies do not survive
    if K > 1:
        med = _row_counts(cloud, sizes, table, range(64, 64 + K - 1))
        assert (med == n - 2).all(), (n, K)
    if K >= 1:
        assert (_row_counts(cloud, sizes, table, [64 + K - 1]) == n - 1).all(), (n, K)
        assert (oracle[1] == n - 1).all() and (oracle[3] == 64 + K - 1).all()     # the last survivor wins
    else:
        assert np.array_equal(oracle[1], L) and (oracle[3] < 64).all()
    # ---- the library ----
    _assert_same(_evaluate_both(_operator(table), cloud, sizes, 1), oracle, (n, K))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_tied_survivors_go_to_the_lowest_index(n):
    """70 survivors with the same count, more than a batch of them: the first one wins (cuda_ransac.py:125-146 resolved
    to the lowest index), whatever the later ones of the same count do."""
    rng = np.random.default_rng(77 + n)
    blocks = [_block(rng, n) for _ in range(3)]
    cloud, sizes = np.vstack(blocks), np.full(3, n, dtype=np.int32)
    table = _table(rng, n, 71)
    table[64 + 70] = table[64]                      # no best row: 71 medium rows
    oracle = rnp.evaluate(cloud, sizes, table, THR, details=True)[:4]
    assert (_group0_best(cloud, sizes, table) < n - 2).all()
    assert (_row_counts(cloud, sizes, table, range(64, 64 + 71)) == n - 2).all()
    assert (oracle[1] == n - 2).all() and (oracle[3] == 64).all()
    _assert_same(_evaluate_both(_operator(table), cloud, sizes, 1), oracle, ("tied", n))


def _two_stage(n, L):
    m1 = min(n, (n - L + 2 + 3) & ~3)
    return n - m1 >= 6


@pytest.mark.gpu
def test_rotation_mixes_block_kinds_in_one_workgroup():
    """One launch of 200 000 blocks of 20 points: every workgroup of the one-wave instance takes four consecutive blocks
    of the size-sorted list through its three rotating buffers - blocks that leave after group 0 (no prescreen, no
    survivors: the parked point goes straight to the staging), blocks with the two-stage count (the ring occupies the
    buffers the point is parked in afterwards) and blocks with the single-stage count and one survivor, in random order.
    The blocks are copies of 24 templates; a draw at the centre of a position samples the same point of a copy wherever
    it starts, so the oracle's results on the templates are the oracle's results on the copies - asserted for the first
    240 blocks of the launch, which the oracle evaluates in place."""
    n = N_ROT
    rng = np.random.default_rng(4242)
    kinds = ["flat", "split", "crafted"]
    templates = [_block(rng, n, kinds[i % 3]) for i in range(24)]
    # poor rows draw from what lies on the plane of a `split` block: positions 0-3, 8-14 and the last
    table = _table(rng, n, 1, core=[0, 1, 2, 3, 8, 9, 10, 11, 12, 13, 14])
    t_cloud, t_sizes = np.vstack(templates), np.full(24, n, dtype=np.int32)
    t_oracle = rnp.evaluate(t_cloud, t_sizes, table, THR, details=True)[:4]
    # ---- the templates are what they claim ----
    L = _group0_best(t_cloud, t_sizes, table)
    for i in range(24):
        if kinds[i % 3] == "flat":       # leaves after group 0
            assert L[i] == n and t_oracle[1][i] == n and t_oracle[3][i] == 0
        elif kinds[i % 3] == "split":    # two stages, nobody beats group 0
            assert L[i] == 12 and _two_stage(n, 12) and t_oracle[1][i] == 12 and t_oracle[3][i] < 64
        else:                            # one stage, the one survivor wins
            assert L[i] < n - 2 and not _two_stage(n, int(L[i])) and t_oracle[1][i] == n - 1 and t_oracle[3][i] == 64
    # ---- the launch ----
    pick = rng.integers(0, 24, ROT_BLOCKS)
    cloud = t_cloud.reshape(24, n, 3)[pick].reshape(-1, 3)
    sizes = np.full(ROT_BLOCKS, n, dtype=np.int32)
    oracle = (t_oracle[0].reshape(24, n)[pick].reshape(-1), t_oracle[1][pick], t_oracle[2][pick], t_oracle[3][pick])
    head = rnp.evaluate(cloud[:240 * n], sizes[:240], table, THR, details=True)[:4]
    assert np.array_equal(head[0], oracle[0][:240 * n]) and np.array_equal(head[1], oracle[1][:240])
    assert np.array_equal(head[2].view(np.uint32), oracle[2][:240].view(np.uint32)) and np.array_equal(head[3], oracle[3][:240])
    _assert_same(_evaluate_both(_operator(table), cloud, sizes, 0), oracle, "rotation")
