"""Directed blocks for the two-stage widened count of k_ransac's prescreen (csrc/ransac.hip).

Every launch below holds more than 24 576 blocks, so blocks under 64 points run on the one-wave instance - the one
with the two-stage count (smaller launches put every block on two or four waves).  Each launch is evaluated with the
prescreen on and with NO_RANSAC_PRESCREEN=1, and both are compared with the oracle: count, winner index, f32 plane bits
and mask.

The directed blocks are made of two parallel planes A and B (0.25 apart, threshold 0.01) and junk points far from
both: A points first, junk in the middle, B points last.  Three hypothesis tables decide who samples what:
  random     NumPy's table, as the benchmark uses it
  one_late   every hypothesis draws from the first 30 % of a block (A points), hypothesis 1000 alone from the last
             30 % (B points)
  all_late   hypotheses 0..63 draw from the first 30 %, every later one from the last 30 %: on a block with fewer B
             than A points all 960 later hypotheses miss nothing among the points the group-0 winner misses (the B
             points, counted first), stay undecided after stage 1 and fill the stage-2 queue fifteen times
With budget = n - L and m1 = min(n, (budget + 2 + 3) & ~3), a block takes two stages when n - m1 >= 6.
"""

import numpy as np
import pytest

from octreelib_amd.ransac import CudaRansac
from oracle import ransac_np as rnp
from tests._util import set_option

THR = 0.01
N_BLOCKS = 25_000


def _two_stage(n, L):
    m1 = min(n, (n - L + 2 + 3) & ~3)
    return n - m1 >= 6


# name -> (A points, junk points, B points).  The zones the crafted tables sample from (first / last 30 % of the
# positions, one position of margin) lie inside the A / B points of every block that names a B count; blocks with
# B = 0 end on A points.
DIRECTED = {
    "budget_0": (30, 0, 0),              # L = n: the block ends with group 0
    "late_wins_by_one": (15, 9, 16),
    "late_ties": (16, 8, 16),
    "late_loses_all_undecided": (20, 8, 14),
    "n63_late_wins_by_one": (25, 12, 26),
    "n63_late_ties": (26, 11, 26),
    "switch_two_stage": (10, 3, 7),      # n = 20, L = 10: m1 = 12, eight points left
    "switch_single_stage": (9, 4, 7),    # n = 20, L = 9: m1 = 16, four points left
    "n6": (6, 0, 0),
    "n7": (7, 0, 0),
    "n7_one_junk": (6, 1, 0),
}
COPIES = 4


def _plane_points(rng, m, base, offset):
    p = rng.random((m, 3)) * 0.5
    p[:, 2] = 0.1 * p[:, 0] + 0.2 * p[:, 1] + offset
    return p + base


def _build():
    rng = np.random.default_rng(20261016)
    blocks, names = [], []

    def base():
        return rng.integers(0, 32, 3).astype(np.float64)

    for name, (a, j, b) in DIRECTED.items():
        for _ in range(COPIES):
            o = base()
            junk = rng.random((j, 3)) * 0.5 + o
            junk[:, 2] = o[2] + 0.6 + rng.random(j) * 0.3
            blocks.append(np.vstack([_plane_points(rng, a, o, 0.05), junk, _plane_points(rng, b, o, 0.30)]))
            names.append(name)
    for _ in range(COPIES):
        # budget 1: A points with one junk point in the middle (no table samples it: positions 30 % .. 70 %)
        o = base()
        p = _plane_points(rng, 20, o, 0.05)
        p[10, 2] += 0.5
        blocks.append(p)
        names.append("budget_1")
        # every point twice
        o = base()
        half = np.vstack([_plane_points(rng, 14, o, 0.05), _plane_points(rng, 6, o, 0.30)])
        blocks.append(np.repeat(half, 2, axis=0))
        names.append("duplicates")
        blocks.append(np.vstack([half[:14], half[:14], half[14:], half[14:]]))
        names.append("duplicates_ab")
        # no plane of group 0 comes near any point (at most its own sample): scattered points 100 across, L = 0 or 1
        blocks.append(rng.random((24, 3)) * 100.0 + o)
        names.append("winner_misses_all")
    # generic leaves of 6 .. 63 points: a noisy plane with outliers, or uniform
    while len(blocks) < 1500:
        n = int(rng.choice([6, 7, 63, int(rng.integers(6, 64))]))
        o = base()
        p = rng.random((n, 3)) * 0.5
        if rng.random() < 0.8:
            z = 0.25 + rng.uniform(-0.4, 0.4) * (p[:, 0] - 0.25) + rng.uniform(-0.4, 0.4) * (p[:, 1] - 0.25)
            keep = rng.random(n) < 0.8
            p[keep, 2] = (z + rng.normal(0, 0.005, n))[keep]
        blocks.append(p + o)
        names.append("generic")
    # filler: small noisy planar leaves, so that the launch goes to the one-wave instance
    while len(blocks) < N_BLOCKS:
        n = int(rng.integers(6, 10))
        p = rng.random((n, 3)) * 0.5
        p[:, 2] = 0.25 + 0.3 * (p[:, 0] - 0.25) + rng.normal(0, 0.006, n)
        blocks.append(p + base())
        names.append("filler")
    sizes = np.array([len(b) for b in blocks], dtype=np.int32)
    return np.vstack(blocks), sizes, np.array(names)


def _table(kind):
    np.random.seed(7)
    op = CudaRansac(threshold=THR, hypotheses_number=1024, initial_points_number=6)
    tab = op.random_hypotheses       # (the operator's own array: edited in place)
    if kind != "random":
        rng = np.random.default_rng(99)
        # (one draw per twentieth of the block: six DIFFERENT points from 20 points on - a sample of one or two
        #  distinct points gives the reference's zero plane, which counts every point)
        tab[:] = (np.arange(6) + rng.random(tab.shape)) * 0.05
        late = [1000] if kind == "one_late" else list(range(64, 1024))
        tab[late] = 0.7 + (np.arange(6) + rng.random((len(late), 6))) * 0.05
    return op


_CACHE = {}


def _results(kind):
    if kind not in _CACHE:
        if "cloud" not in _CACHE:
            _CACHE["cloud"] = _build()
        cloud, sizes, names = _CACHE["cloud"]
        op = _table(kind)
        oracle = rnp.evaluate(cloud, sizes, op.random_hypotheses, THR, details=True)[:4]
        got = {}
        for off in (0, 1):
            set_option("NO_RANSAC_PRESCREEN", off)
            got[off] = op.evaluate(cloud, sizes, details=True)
        set_option("NO_RANSAC_PRESCREEN", 0)
        _CACHE[kind] = (oracle, got)
    return _CACHE["cloud"], _CACHE[kind]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "one_late", "all_late"])
def test_two_stage_count_matches_exact_path_and_oracle(kind):
    (cloud, sizes, names), ((o_mask, o_count, o_plane, o_index), got) = _results(kind)
    assert len(sizes) > 24_576 and sizes.max() < 64
    for off in (0, 1):
        mask, planes, counts, index = got[off]
        bad = np.flatnonzero((counts != o_count) | (index != o_index) |
                             (planes.view(np.uint32) != o_plane.view(np.uint32)).any(axis=1))
        assert len(bad) == 0, (kind, off, [(int(b), names[b]) for b in bad[:10]])
        assert np.array_equal(mask, o_mask), (kind, off)
    # prescreen on against prescreen off of the same library
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a.view(np.uint8) if a.dtype == np.bool_ else a.view(np.uint32),
                              b.view(np.uint8) if b.dtype == np.bool_ else b.view(np.uint32))


@pytest.mark.gpu
def test_directed_blocks_are_what_they_claim():
    """The oracle's winners on the directed blocks are the cases their names promise, on the side of the switch they
    promise; the library's agree (prescreen on)."""
    (cloud, sizes, names), ((_, c1, _, i1), got1) = _results("one_late")
    _, ((_, c2, _, i2), got2) = _results("all_late")
    assert np.array_equal(got1[0][2], c1) and np.array_equal(got1[0][3], i1)
    assert np.array_equal(got2[0][2], c2) and np.array_equal(got2[0][3], i2)

    def of(name):
        sel = np.flatnonzero(names == name)
        assert len(sel) == COPIES, name
        return sel

    def group0_best(name):
        a = DIRECTED[name][0]
        return a

    for b in of("budget_0"):
        assert c1[b] == sizes[b] and i1[b] == 0
    for b in of("budget_1"):
        assert c1[b] == sizes[b] - 1 and i1[b] == 0 and _two_stage(int(sizes[b]), int(c1[b]))
    for name in ("late_wins_by_one", "n63_late_wins_by_one"):
        for b in of(name):
            L = group0_best(name)
            assert _two_stage(int(sizes[b]), L)
            assert c1[b] == L + 1 and i1[b] == 1000       # the one late hypothesis, by exactly one inlier
            assert c2[b] == L + 1 and i2[b] == 64         # 960 of them: the lowest index
    for name in ("late_ties", "n63_late_ties"):
        for b in of(name):
            L = group0_best(name)
            assert _two_stage(int(sizes[b]), L)
            assert c1[b] == L and i1[b] == 0              # a tie goes to the lower index
            assert c2[b] == L and i2[b] == 0
    for b in of("late_loses_all_undecided"):
        a, j, nb = DIRECTED["late_loses_all_undecided"]
        m1 = (a + j + nb - a + 2 + 3) & ~3
        assert _two_stage(a + j + nb, a) and m1 - nb < (a + j + nb) - a   # misses within stage 1 stay under the budget
        assert c2[b] == a and i2[b] == 0
    for b in of("switch_two_stage"):
        assert c1[b] == 10 and _two_stage(20, 10)
    for b in of("switch_single_stage"):
        assert c1[b] == 9 and not _two_stage(20, 9) and _two_stage(20, 10)
    assert (c1[of("winner_misses_all")] <= 1).all() and (c1[of("winner_misses_all")] == 0).any()
    for b in of("n6"):
        assert sizes[b] == 6
    for b in of("n7_one_junk"):
        assert sizes[b] == 7
