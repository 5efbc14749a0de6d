"""Directed blocks for the certified exit's own table (csrc/ransac.hip, pos_table_entry: one word per (block size,
hypothesis) with the byte offsets of the first three distinct sample positions, and a flag where the hypothesis cannot
be vouched for whatever the points are).  The loop over the later hypotheses of a certified block reads nothing else, so
a wrong entry shows as a zero plane that is not fitted (a degenerate sample vouched for) or only as lost time (a proper
sample sent to the exact queue): the first kind is what these blocks are built to catch.

Blocks as in tests/test_gpu_ransac_cert_exit.py (its _directed), at n = 7, 16, 33 and 63, three copies each:
  far1 / far1_dyadic       one outlier                                                            b = 1, certified
  far2 / far2_dyadic       two outliers                                                           b = 2, certified from 16 points on
  dup_positions            three distinct positions of hypothesis 600, two distinct points
  collinear_below / above  the three distinct positions of hypothesis 800 nearly collinear, either side of the floor
and 250 generic leaves of 6 .. 63 points.  RANSAC_WAVES = 1 puts every block on the one-wave instance, however few there
are.  Tables: zero_one and zero_two of that test (later hypotheses that draw one or two distinct points: the zero plane
must win from an index of 64 or more on the dyadic blocks), with
  row 650   its third draw is the largest double below 1: a flagged draw, which the reference's sum with the block's start
            rounds to position n - the spill point behind the block
  row 760   at 63 points positions 62, 0 and 61: the top of the 10-bit offsets (62 x 16 = 992)
  row 80    (H = 100 only) one point six times: the zero plane from a later hypothesis of a table with two groups
H = 1024 (the benchmark's instance), H = 1000 (the same instance with lanes of the last group beyond the table: 1000 =
15 x 64 + 40) and H = 100 (one hypothesis per lane: no prescreen and no exit, but a table of 100 columns is built).
Every launch runs with the prescreen on and with NO_RANSAC_PRESCREEN = 1, which switches the exit off with it: count,
winner index, f32 plane bits and mask equal the oracle's, and each other's.
"""

import numpy as np
import pytest

from octreelib_amd.ransac import CudaRansac
from oracle import ransac_np as rnp
from tests import _plane_cert as pcm
from tests import test_gpu_ransac_cert_exit as ce
from tests._util import set_option

THR = ce.THR
SIZES = (7, 16, 33, 63)
COPIES = 3
N_GENERIC = 250
DIRECTED = ("far1", "far1_dyadic", "far2", "far2_dyadic", "dup_positions", "collinear_below", "collinear_above")
KINDS = ("zero_one", "zero_two")
HS = (1024, 1000, 100)
BELOW_ONE = float(np.nextafter(1.0, 0.0))

_CACHE = {}


def _table(kind, H):
    tab = ce._draws(kind).copy()
    tab[650, 2] = BELOW_ONE
    tab[760] = np.array([62.5, 0.5, 61.5, 62.5, 0.5, 61.5]) / 63.0
    if H == 100:
        tab[80] = 0.5
        tab[90, 2] = BELOW_ONE
    return np.ascontiguousarray(tab[:H])


def _cloud():
    if "cloud" not in _CACHE:
        blocks, names = [], []
        for k, name in enumerate(DIRECTED):
            for n in SIZES:
                for c in range(COPIES):
                    own = np.random.default_rng([20261101, k, n, c])
                    blocks.append(ce._directed(own, name, n) + own.integers(0, 32, 3).astype(np.float64))
                    names.append(name)
        rng = np.random.default_rng(20261101)
        for _ in range(N_GENERIC):
            n = int(rng.choice([7, 16, 33, 63, int(rng.integers(6, 64))]))
            p = rng.random((n, 3)) * 0.5
            z = 0.25 + rng.uniform(-0.4, 0.4) * (p[:, 0] - 0.25) + rng.uniform(-0.4, 0.4) * (p[:, 1] - 0.25)
            keep = rng.random(n) < 0.93
            p[keep, 2] = (z + rng.normal(0, 0.002, n))[keep]
            blocks.append(p + rng.integers(0, 32, 3).astype(np.float64))
            names.append("generic")
        # one block more: the spill point of the last checked block is the same with or without what follows
        blocks.append(rng.random((9, 3)) + 3.0)
        names.append("tail")
        sizes = np.array([len(b) for b in blocks], dtype=np.int32)
        _CACHE["cloud"] = (blocks, np.vstack(blocks), sizes, np.array(names))
    return _CACHE["cloud"]


def _oracle(kind, H):
    key = ("oracle", kind, H)
    if key not in _CACHE:
        _, cloud, sizes, _ = _cloud()
        mask, count, plane, index = rnp.evaluate(cloud, sizes, _table(kind, H), THR, details=True)[:4]
        m = int(sizes[:-1].sum())
        _CACHE[key] = (mask[:m], count[:-1], plane[:-1], index[:-1])
    return _CACHE[key]


def _library(kind, H):
    _, cloud, sizes, _ = _cloud()
    np.random.seed(ce.SEED)
    op = CudaRansac(threshold=THR, hypotheses_number=H, initial_points_number=6)
    op.random_hypotheses[:] = _table(kind, H)
    got = {}
    set_option("RANSAC_WAVES", 1)
    for off in (0, 1):
        set_option("NO_RANSAC_PRESCREEN", off)
        got[off] = op.evaluate(cloud, sizes, details=True)
    set_option("NO_RANSAC_PRESCREEN", 0)
    set_option("RANSAC_WAVES", 0)
    return got


def check_blocks(oracle_of):
    """The blocks and the tables are what the docstring promises: by the NumPy model of the certificate and by the oracle.
    (Also run without a GPU by tests/test_cpu_cert_table_blocks.py.)"""
    blocks, _, sizes, names = _cloud()
    assert sizes.max() == 63 and set(SIZES) <= set(sizes.tolist())
    for kind in KINDS:
        tab = _table(kind, 1024)
        # rows 0 .. 63 are NumPy's own: group 0 is that of the `random` table
        assert np.array_equal(tab[:64], ce._draws("random")[:64])
        for n in SIZES:
            # a flagged draw (sample_index_cached: fraction above 1 - 2^-20) that the reference's f64 sum with the block's
            # start rounds up to position n - the spill point - for every block but the cloud's first
            x = tab[650, 2] * n
            assert x - int(x) > 1.0 - 2.0 ** -20 and int(x + 1000.0) - 1000 == n, n
            assert (ce._pos(tab[650, [0, 1, 3, 4, 5]], n) < n).all()
        assert ce._pos(tab[760], 63).tolist() == [62, 0, 61, 62, 0, 61]
    certified = {1: set(), 2: set()}
    o1, o2, o100 = oracle_of("zero_one", 1024), oracle_of("zero_two", 1024), oracle_of("zero_one", 100)
    for i in np.flatnonzero(names != "tail"):
        name, n, pts = str(names[i]), int(sizes[i]), blocks[i]
        L = ce._group0(pts, ce._draws("random"))
        b, cert = n - L, pcm.certified(pts, THR, L)
        if cert:
            certified[b].add(n)
        if name in ("far1", "far1_dyadic"):
            assert (b, cert) == (1, True), (name, n, b, cert)
        if name in ("far2", "far2_dyadic") and n >= 16:
            assert (b, cert) == (2, True), (name, n, b, cert)
        if name in ("far1_dyadic", "far2_dyadic") and n >= 16:
            # the zero plane of a later hypothesis holds every point: one distinct point (700 of zero_one, 80 of the table
            # of 100 rows), two distinct points (700 of zero_two) - and nothing in front of it does
            assert o1[1][i] == n and o1[3][i] == 700 and not o1[2][i].any(), (name, n, o1[3][i])
            assert o2[1][i] == n and o2[3][i] == 700 and not o2[2][i].any(), (name, n, o2[3][i])
            assert o100[1][i] == n and o100[3][i] == 80, (name, n, o100[3][i])
        if name == "dup_positions":
            pos = ce._pos(ce._draws("zero_two")[600], n)
            assert np.array_equal(pts[pos[0]], pts[pos[1]]) and not pcm.vouched(pts, pos[None, :])[0]
            if n >= 16:
                assert len(set(pos.tolist())) == 3 and o2[1][i] == n and o2[3][i] == 600, (n, o2[3][i])
        if name.startswith("collinear"):
            pos = ce._pos(ce.H800, n)
            assert len(set(pos.tolist())) == 3
            assert bool(pcm.vouched(pts, pos[None, :])[0]) == name.endswith("above"), (name, n)
    # certified blocks of both kinds at every size the issue names (b = 2 from 16 points on: see far2 in the other test)
    assert certified[1] >= set(SIZES) and certified[2] >= {16, 33, 63}, certified


@pytest.mark.gpu
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("kind", KINDS)
def test_table_driven_exit_matches_exact_path_and_oracle(kind, H):
    _, cloud, sizes, names = _cloud()
    o_mask, o_count, o_plane, o_index = _oracle(kind, H)
    got = _library(kind, H)
    nb = len(o_count)
    for off in (0, 1):
        mask, planes, counts, index = got[off]
        bad = np.flatnonzero((counts[:nb] != o_count) | (index[:nb] != o_index) |
                             (planes[:nb].view(np.uint32) != o_plane.view(np.uint32)).any(axis=1))
        assert len(bad) == 0, (kind, H, off, [(int(b), names[b], int(sizes[b])) for b in bad[:10]])
        assert np.array_equal(mask[:len(o_mask)], o_mask), (kind, H, off)
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a.view(np.uint8) if a.dtype == np.bool_ else a.view(np.uint32),
                              b.view(np.uint8) if b.dtype == np.bool_ else b.view(np.uint32))


@pytest.mark.gpu
def test_blocks_are_what_they_claim():
    check_blocks(_oracle)
