"""k_ransac (csrc/ransac.hip) with its f32 FMAs as compiler-visible builtins: the compiler is free to reorder and
interleave the count loops (screen_group, screen_ub) and the prescreen's fits, so their results are pinned on every
remainder of the loops' 4-point body: the same as the exact path and as the oracle.

The count loops score four points per body and the remaining one to three points one at a time, and keep an inlier-bit
history word per 32 points; the prescreen fits three hypotheses per lane at a time.  Two launches:

  one_wave   25 000 blocks (more than 24 576: blocks under 64 points run on the one-wave instance, the one with the
             two-stage widened count), block sizes cycling over 6-13, 31-35 and 61-63: every remainder of the 4-point
             body, both sides of the 32-point history word, the largest block.  The oracle runs on the first 8 blocks
             of every size.
  small      600 blocks of 6, 7, 33, 63, 64, 65, 127, 128, 129, 255, 256 and 300 points: the two- and four-wave
             instances and k_ransac_big.  The oracle runs on every block.

Three blocks in four are a noisy plane with one to three junk points, the fourth is a scattered cloud - with
budget = n - L (L: the best count among hypotheses 0..63) and m1 = min(n, (budget + 2 + 3) & ~3) a block takes the
two-stage count when n - m1 >= 6 (tests/test_gpu_ransac_two_stage.py), and both kinds must occur.  Every launch is
evaluated with the prescreen on and with NO_RANSAC_PRESCREEN=1; the two must agree on every block (count, winner
index, f32 plane bits, mask) and with the oracle where it runs (the lowest index among the tied wins).
"""

import numpy as np
import pytest

from octreelib_amd.ransac import CudaRansac
from oracle import ransac_np as rnp
from tests._util import set_option

THR = 0.01
ONE_WAVE_SIZES = list(range(6, 14)) + list(range(31, 36)) + [61, 62, 63]
ONE_WAVE_BLOCKS = 25_000
ORACLE_PER_SIZE = 8
SMALL_SIZES = [6, 7, 33, 63, 64, 65, 127, 128, 129, 255, 256, 300]
SMALL_BLOCKS = 600


def _two_stage(n, L):
    m1 = min(n, (n - L + 2 + 3) & ~3)
    return n - m1 >= 6


def _cloud(sizes, seed):
    rng = np.random.default_rng(seed)
    blocks = []
    for b, n in enumerate(sizes):
        o = rng.integers(0, 32, 3).astype(np.float64)
        p = rng.random((n, 3)) * 0.5
        if b % 4 != 3:
            p[:, 2] = 0.25 + rng.uniform(-0.4, 0.4) * (p[:, 0] - 0.25) + rng.uniform(-0.4, 0.4) * (p[:, 1] - 0.25) \
                + rng.normal(0, 0.003, n)
            junk = rng.choice(n, size=min(n - 5, 1 + b % 3), replace=False)
            p[junk, 2] += 0.1 + rng.random(len(junk)) * 0.3
        blocks.append(p + o)
    return np.vstack(blocks)


_CLOUDS = {}


def _launch(name):
    if name not in _CLOUDS:
        if name == "one_wave":
            sizes = np.array([ONE_WAVE_SIZES[b % len(ONE_WAVE_SIZES)] for b in range(ONE_WAVE_BLOCKS)], dtype=np.int32)
            n_oracle = ORACLE_PER_SIZE * len(ONE_WAVE_SIZES)     # the first 8 blocks of every size
        else:
            sizes = np.array([SMALL_SIZES[b % len(SMALL_SIZES)] for b in range(SMALL_BLOCKS)], dtype=np.int32)
            n_oracle = SMALL_BLOCKS
        _CLOUDS[name] = (_cloud(sizes, 20261019 + len(sizes)), sizes, n_oracle)
    return _CLOUDS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [6, 3, 7])
@pytest.mark.parametrize("H", [1024, 100, 64])
@pytest.mark.parametrize("launch", ["one_wave", "small"])
def test_issue_forms_match_exact_path_and_oracle(launch, H, k):
    cloud, sizes, n_oracle = _launch(launch)
    if launch == "one_wave":
        assert len(sizes) > 24_576 and sizes.max() < 64
        assert all((sizes[:n_oracle] == n).sum() == ORACLE_PER_SIZE for n in ONE_WAVE_SIZES)
    np.random.seed(11)
    op = CudaRansac(threshold=THR, hypotheses_number=H, initial_points_number=k)
    table = op.random_hypotheses
    assert table.shape == (H, k)
    got = {}
    for off in (0, 1):
        set_option("NO_RANSAC_PRESCREEN", off)
        got[off] = op.evaluate(cloud, sizes, details=True)
    set_option("NO_RANSAC_PRESCREEN", 0)
    # prescreen on against prescreen off, every block
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a.view(np.uint8) if a.dtype == np.bool_ else a.view(np.uint32),
                              b.view(np.uint8) if b.dtype == np.bool_ else b.view(np.uint32))
    # both against the oracle on the launch's first n_oracle blocks (their starts are the launch's own)
    m_oracle = int(sizes[:n_oracle].sum())
    o_mask, o_count, o_plane, o_index = rnp.evaluate(cloud[:m_oracle], sizes[:n_oracle], table, THR, details=True)[:4]
    for off in (0, 1):
        mask, planes, counts, index = got[off]
        bad = np.flatnonzero((counts[:n_oracle] != o_count) | (index[:n_oracle] != o_index) |
                             (planes[:n_oracle].view(np.uint32) != o_plane.view(np.uint32)).any(axis=1))
        assert len(bad) == 0, (launch, H, k, off, [(int(b), int(sizes[b])) for b in bad[:10]])
        assert np.array_equal(mask[:m_oracle], o_mask), (launch, H, k, off)
    # the data reaches both branches of the widened count: L is the best count of hypotheses 0..63
    L = rnp.evaluate(cloud[:m_oracle], sizes[:n_oracle], table[:64], THR, details=True)[1]
    under64 = [(int(n), int(c)) for n, c in zip(sizes[:n_oracle], L) if k <= n < 64 and c < n]
    assert any(_two_stage(n, c) for n, c in under64)
    assert any(not _two_stage(n, c) for n, c in under64)
