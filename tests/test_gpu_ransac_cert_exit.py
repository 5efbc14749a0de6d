"""Directed blocks for the certified exit of k_ransac's one-wave instance (csrc/ransac.hip "the certified exit",
csrc/plane_cert.h): a block ends behind group 0 when the best count L of hypotheses 0..63 is n - 1 or n - 2 and no plane
can hold more than L of its points; only later hypotheses that may be the reference's zero plane are still fitted.

Every launch holds more than 24 576 blocks, so blocks under 64 points run on the one-wave instance.  Each launch is
evaluated with the prescreen on and with NO_RANSAC_PRESCREEN=1 (which switches the exit off with it); both are compared
with the oracle on count, winner index, f32 plane bits and mask.  The oracle is evaluated on the leading blocks - the
directed ones, the generic leaves and one block more, whose start in the batch cloud is the same with or without what
follows - and the filler behind them is compared between the two runs of the library.

Directed blocks, four copies each at n = 6, 7, 20 and 63 (threshold 0.01; "dyadic": coordinates are multiples of 2^-8 on
the plane z = x / 2 + y / 4, so that a sample of one or two distinct points cancels exactly into the zero plane):
  far1 / far1_dyadic      a plane and one outlier 0.5 away                        b = 1, certified
  out_0.9 / 1.1 / 3       the outlier 0.9, 1.1, 3 x thr from the plane            b = 0 / b = 1, not certified / b = 1,
                          not certified either: one point d away lifts the smallest eigenvalue by less than d^2, and the
                          certificate asks for n thrblk^2 - so the line lies near sqrt(n) thr, and the next two cases sit on it:
  hold_above / hold_below the outlier where the model's test stands at 1.15 / 0.87 of its line (left side over right side,
                          found by bisection per block: 1.3 x sqrt(n) thr away at 63 points, more below)          b = 1, certified / refused
  far2 / far2_dyadic      two outliers 0.5 and 0.375 away on either side          b = 2, certified
  b3                      three outliers                                          b = 3: the untouched path
  dup_positions           far1_dyadic with the points at two positions of hypothesis 600 (table zero_two) equal: three
                          distinct positions, two distinct points three times each - it wins with count n there
  collinear_below/above   far1 with the three distinct positions of hypothesis 800 (tables zero_one, zero_two) nearly
                          collinear: |cross product| = 0.9 / 1.1 x 2^-12 E^2, either side of the floor
  second_plane            (n = 20, 63; see below) n - 3 points on a line of the plane, one more on the plane, two outliers in
                          another plane through the line: that plane holds n - 1 points           b = 2, must refuse
  late_holds_all          (n = 20, 63) every point within thr of z = 0, the leading points on a plane tilted by 1 / 64
                          that misses one point                                                 b = 1, must refuse
Tables (NumPy's table of seed 13, edited; see SEED):
  random     as it is
  zero_one   hypothesis 700 draws one point six times (the zero plane; it must win with count n on the dyadic blocks);
             900 draws one point six times for n <= 20, two points three times each at n = 63: the lower index wins
  zero_two   hypothesis 700 ALONE is degenerate on an ordinary block: it draws two distinct points three times each (exact
             cancellation on dyadic coordinates) and nothing degenerate follows it; 600 draws positions (a, b, a, c, c, c) -
             a proper plane everywhere but on dup_positions, which makes the points at a and b equal
  one_late   hypotheses 0..63 - and every other but one - draw position 0 and one position from each of the next five
             twentieths of the block; hypothesis 1000 alone draws from the last 30 %: second_plane and late_holds_all
             put the plane group 0 finds in front and the better one behind
second_plane and late_holds_all exist at 20 and 63 points only: they need group 0 confined to one part of the block and
one later hypothesis to another, and one_late's twentieths fall on one or two positions below 20 points (a sample of
two points is the zero plane, which holds everything).  Blocks of 6 and 7 points would need a table of their own - a
fifth launch - and are not covered for these two cases; "must refuse" at 6 and 7 points is hold_below and out_1.1.
Six points leave little room in general: with three of six points off the plane (b3) another plane holds four, and two
outliers of six or seven (far2) may leave a leave-one-out set that is flat - the claims below say what holds there.
"""

import numpy as np
import pytest

from octreelib_amd.ransac import CudaRansac
from oracle import ransac_np as rnp
from tests import _plane_cert as pcm
from tests._util import set_option

THR = 0.01
N_BLOCKS = 25_000
N_CHECKED = 1_500          # directed blocks and generic leaves: compared with the oracle
SIZES = (6, 7, 20, 63)
COPIES = 4
KINDS = ("random", "zero_one", "zero_two", "one_late")
H800 = np.array([0.05, 0.4, 0.75, 0.05, 0.4, 0.75])


# NumPy's table of this seed: none of its hypotheses 0..63 draws fewer than three distinct positions at n = 6 or 7 (13 is
# the first seed with that property).  With seed 7, hypothesis 48 draws position 0 six times at n = 6: its zero plane holds
# every point and ends every block of six points behind group 0, whatever the block is.
SEED = 13


def _draws(kind):
    np.random.seed(SEED)
    tab = np.random.random((1024, 6))
    rng = np.random.default_rng(99)
    if kind == "zero_one":
        tab[700] = 0.5
        tab[900] = [0.30, 0.30, 0.30, 0.32, 0.32, 0.32]
        tab[800] = H800
    elif kind == "zero_two":
        tab[700] = [0.1, 0.1, 0.1, 0.9, 0.9, 0.9]
        tab[600] = [0.2, 0.25, 0.2, 0.6, 0.6, 0.6]
        tab[800] = H800
    elif kind == "one_late":
        tab[:] = (np.arange(6) + rng.random(tab.shape)) * 0.05
        tab[:, 0] = 0.0
        tab[1000] = 0.7 + (np.arange(6) + rng.random(6)) * 0.05
    return tab


def _pos(draws, n):
    return np.minimum((draws * n).astype(np.int64), n - 1)


def _plane(rng, m, dyadic):
    """m distinct points with x, y in [0, 0.5) on z = x / 2 + y / 4 (+ 0.05 when not dyadic)."""
    if dyadic:
        xy = rng.choice(128 * 128, m, replace=False)
        p = np.stack([(xy // 128) / 256.0, (xy % 128) / 256.0], 1)
        return np.column_stack([p, p[:, 0] / 2.0 + p[:, 1] / 4.0])
    p = rng.random((m, 2)) * 0.5
    return np.column_stack([p, p[:, 0] / 2.0 + p[:, 1] / 4.0 + 0.05])


NORMAL_Z = float(np.sqrt(1.0 + 0.25 + 0.0625))     # a z offset of d * NORMAL_Z moves a point d away from the plane


def _directed(rng, name, n):
    """The points of one directed block (before its integer base is added), or None where the case needs more points."""
    dy = name.endswith("dyadic") or name == "dup_positions"
    if name in ("far1", "far1_dyadic", "dup_positions", "collinear_below", "collinear_above"):
        p = _plane(rng, n, dy)
        out = n - 1 if name.startswith("collinear") else n // 2
        p[out, 2] += 0.5
        if name == "dup_positions":
            a, b = _pos(_draws("zero_two")[600], n)[:2]
            p[b] = p[a]
        if name.startswith("collinear"):
            a, b, c = _pos(H800, n)[:3]
            E = float(np.abs((p - p[0]).astype(np.float32)).max())
            d = p[b] - p[a]
            w = np.cross(d, [-0.5, -0.25, 1.0])             # in the plane, across the line
            f = 0.9 if name.endswith("below") else 1.1
            p[c] = p[a] + 0.5 * d + w / np.linalg.norm(w) * (f * 2.0 ** -12 * E * E / np.linalg.norm(d))
        return p
    if name.startswith("out_"):
        p = _plane(rng, n, False)
        p[n // 2, 2] += float(name[4:]) * THR * NORMAL_Z
        return p
    if name.startswith("hold_"):
        # the z offset of the outlier at which the model's test stands at `want` of its line (monotone in the offset);
        # t as for a block at the middle of the bases' range - the base moves thrblk by 0.3 %, the margin by 0.6 %
        want = 1.15 if name == "hold_above" else 0.87
        p = _plane(rng, n, False)
        t = pcm.block_constants(p + 16.0, THR)[1]
        lo, hi = THR, 1.0
        for _ in range(50):
            mid = 0.5 * (lo + hi)
            q = p.copy()
            q[n // 2, 2] += mid
            lo, hi = (mid, hi) if pcm.margin_all(q, t) < want else (lo, mid)
        p[n // 2, 2] += hi
        return p
    if name in ("far2", "far2_dyadic", "b3"):
        p = _plane(rng, n, dy)
        p[n // 2, 2] += 0.5
        p[n // 2 + 1, 2] -= 0.375
        if name == "b3":
            p[n // 2 - 1, 2] += 0.25
        return p
    if n < 20:
        return None
    late = _pos(_draws("one_late")[1000], n)
    if name == "second_plane":
        x = rng.choice(np.arange(1, 128), n - 3, replace=False) / 256.0
        line = np.column_stack([x, np.full(n - 3, 0.25), x / 2.0 + 0.0625])      # on z = x / 2 + y / 4
        p = np.empty((n, 3))
        rest = [i for i in range(1, n) if i not in (late[4], late[5])]
        p[0] = [0.125, 0.0, 0.0625]                                                # the one other point of the plane
        p[rest] = line
        p[late[4]] = [0.125, 0.25, 0.375]                                          # in the plane y = 0.25 through the line
        p[late[5]] = [0.375, 0.25, 0.5]
        return p
    assert name == "late_holds_all"
    xy = rng.choice(128 * 128, n, replace=False)
    p = np.column_stack([(xy // 128) / 256.0, (xy % 128) / 256.0, np.zeros(n)])
    lead = int(np.ceil(0.3 * n))
    p[:lead, 2] = p[:lead, 0] / 64.0
    p[n // 2] = [0.75, 0.125, 0.0]
    return p


DIRECTED = ("far1", "far1_dyadic", "out_0.9", "out_1.1", "out_3", "hold_above", "hold_below", "far2", "far2_dyadic", "b3", "dup_positions",
            "collinear_below", "collinear_above", "second_plane", "late_holds_all")


def _build():
    rng = np.random.default_rng(20261020)
    blocks, names = [], []

    def base():
        return rng.integers(0, 32, 3).astype(np.float64)

    # (every directed block from a generator of its own: a case added later leaves the others as they were)
    for k, name in enumerate(DIRECTED):
        for n in SIZES:
            for c in range(COPIES):
                own = np.random.default_rng([20261020, k, n, c])
                p = _directed(own, name, n)
                if p is not None:
                    blocks.append(p + own.integers(0, 32, 3).astype(np.float64))
                    names.append(name)
    # generic leaves of 6 .. 63 points: a noisy plane with outliers, or uniform
    while len(blocks) < N_CHECKED:
        n = int(rng.choice([6, 7, 63, int(rng.integers(6, 64))]))
        p = rng.random((n, 3)) * 0.5
        if rng.random() < 0.8:
            z = 0.25 + rng.uniform(-0.4, 0.4) * (p[:, 0] - 0.25) + rng.uniform(-0.4, 0.4) * (p[:, 1] - 0.25)
            keep = rng.random(n) < 0.9
            p[keep, 2] = (z + rng.normal(0, 0.002, n))[keep]
        blocks.append(p + base())
        names.append("generic")
    # filler: small noisy planar leaves, so that the launch goes to the one-wave instance
    while len(blocks) < N_BLOCKS:
        n = int(rng.integers(6, 10))
        p = rng.random((n, 3)) * 0.5
        p[:, 2] = 0.25 + 0.3 * (p[:, 0] - 0.25) + rng.normal(0, 0.004, n)
        blocks.append(p + base())
        names.append("filler")
    sizes = np.array([len(b) for b in blocks], dtype=np.int32)
    return blocks, np.vstack(blocks), sizes, np.array(names)


_CACHE = {}


def _cloud():
    if "cloud" not in _CACHE:
        _CACHE["cloud"] = _build()
    return _CACHE["cloud"]


def _oracle(kind):
    """The oracle on the leading N_CHECKED blocks (evaluated with one block more behind them: the spill point)."""
    key = ("oracle", kind)
    if key not in _CACHE:
        _, cloud, sizes, _ = _cloud()
        m = int(sizes[:N_CHECKED + 1].sum())
        mask, count, plane, index = rnp.evaluate(cloud[:m], sizes[:N_CHECKED + 1], _draws(kind), THR, details=True)[:4]
        mp = int(sizes[:N_CHECKED].sum())
        _CACHE[key] = (mask[:mp], count[:N_CHECKED], plane[:N_CHECKED], index[:N_CHECKED])
    return _CACHE[key]


def _library(kind):
    key = ("library", kind)
    if key not in _CACHE:
        _, cloud, sizes, _ = _cloud()
        np.random.seed(SEED)
        op = CudaRansac(threshold=THR, hypotheses_number=1024, initial_points_number=6)
        op.random_hypotheses[:] = _draws(kind)       # (the operator's own array: edited in place)
        got = {}
        for off in (0, 1):
            set_option("NO_RANSAC_PRESCREEN", off)
            got[off] = op.evaluate(cloud, sizes, details=True)
        set_option("NO_RANSAC_PRESCREEN", 0)
        _CACHE[key] = got
    return _CACHE[key]


def _group0(pts, draws):
    """Best exact count of hypotheses 0..63 of a block (the reference's arithmetic; no draw of these tables is risky)."""
    idx = _pos(draws[:64], len(pts))
    plane = rnp.plane_from_points(pts[idx]).astype(np.float32).astype(np.float64)
    dist = np.abs(((plane[:, 0:1] * pts[None, :, 0] + plane[:, 1:2] * pts[None, :, 1])
                   + plane[:, 2:3] * pts[None, :, 2]) + plane[:, 3:4])
    return int((dist < THR).sum(1).max())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_certified_exit_matches_exact_path_and_oracle(kind):
    _, cloud, sizes, names = _cloud()
    assert len(sizes) > 24_576 and sizes.max() < 64
    o_mask, o_count, o_plane, o_index = _oracle(kind)
    got = _library(kind)
    mp = len(o_mask)
    for off in (0, 1):
        mask, planes, counts, index = got[off]
        bad = np.flatnonzero((counts[:N_CHECKED] != o_count) | (index[:N_CHECKED] != o_index) |
                             (planes[:N_CHECKED].view(np.uint32) != o_plane.view(np.uint32)).any(axis=1))
        assert len(bad) == 0, (kind, off, [(int(b), names[b], int(sizes[b])) for b in bad[:10]])
        assert np.array_equal(mask[:mp], o_mask), (kind, off)
    # prescreen (and exit) on against off, every block of the launch
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a.view(np.uint8) if a.dtype == np.bool_ else a.view(np.uint32),
                              b.view(np.uint8) if b.dtype == np.bool_ else b.view(np.uint32))


def _claims():
    """Per directed block: (name, n, b under each table that matters, the model's certificate there)."""
    blocks, _, sizes, names = _cloud()
    out = []
    for i in np.flatnonzero((names != "generic") & (names != "filler")):
        row = {"i": int(i), "name": str(names[i]), "n": int(sizes[i])}
        for kind in KINDS:
            L = _group0(blocks[i], _draws(kind))
            row[kind] = (int(sizes[i]) - L, pcm.certified(blocks[i], THR, L))
        out.append(row)
    return out


def check_directed_blocks(oracle_of):
    """The directed blocks are what their names promise: b = n - L of group 0, the certificate by the NumPy model, the
    winner by the oracle.  (Also run without a GPU by tests/test_cpu_cert_exit_blocks.py.)"""
    blocks, _, sizes, names = _cloud()
    rows = _claims()
    assert len(rows) == (len(DIRECTED) - 2) * len(SIZES) * COPIES + 2 * 2 * COPIES
    seen = set()
    for r in rows:
        name, n, i = r["name"], r["n"], r["i"]
        seen.add((name, n))
        pts = blocks[i]
        if name in ("far1", "far1_dyadic", "dup_positions"):
            assert r["random"] == (1, True), r
        if name.startswith("collinear"):
            # (six or seven points: a hypothesis of group 0 may draw the three nearly collinear points alone, and its
            #  ill-conditioned plane through their line may turn to hold the outlier as well: b = 0)
            assert r["random"] == (1, True) or (n < 20 and r["random"] == (0, None)), r
        if name.startswith("hold_"):
            # on either side of the line, within 20 % of it; group 0 reaches n - 1 wherever it is tested (one_late: group 0
            # cannot sample position n / 2, so b = 1 for certain from 20 points on)
            m = pcm.margin_all(pts, pcm.block_constants(pts, THR)[1])
            assert (1.08 < m < 1.22) if name == "hold_above" else (0.80 < m < 0.94), (r, m)
            # (the distance from the plane of the other points, in units of sqrt(n) thr: above 1, more where the point has
            #  leverage - six points - or the plane's own two eigenvalues differ)
            off = pts - pts[0]
            d = abs(off[n // 2, 2] - off[n // 2, 0] / 2.0 - off[n // 2, 1] / 4.0) / NORMAL_Z
            print(f"{name} n = {n}: margin {m:.3f}, outlier {d / THR:.2f} thr = {d / (np.sqrt(n) * THR):.2f} sqrt(n) thr")
            if name == "hold_above":     # (a certified outlier is never nearer: it lifts the eigenvalue by less than d^2)
                assert d > np.sqrt(n) * THR, (r, d)
            if name == "hold_above":
                assert r["random"] == (1, True), r
            else:
                assert r["random"] in ((1, False), (0, None)), r     # (a tilted plane of group 0 may hold the outlier too)
            if n >= 20:
                assert r["one_late"] == (1, name == "hold_above"), r
        if name in ("far2", "far2_dyadic"):
            # (six or seven points less one leave three or four on the plane and two outliers: leave-one-out may refuse,
            #  and with six points some plane through an outlier may hold five)
            if n >= 20:
                assert r["random"] == (2, True), r
            else:
                assert r["random"][0] in ((2,) if n == 7 or name == "far2_dyadic" else (1, 2)), r
        if name == "b3":      # (three of six points off the plane: some other plane may hold four)
            assert (r["random"][0] == 3 and r["random"][1] is None) or (n == 6 and r["random"][0] in (1, 2)), r
        if name == "out_0.9":
            assert r["random"][0] == 0, r
        if name == "out_1.1":
            # under the random table a hypothesis of group 0 that samples the outlier tilts enough to hold it: b = 0;
            # under one_late group 0 cannot sample it (position n / 2; six and seven points: that table draws two or three
            # positions and is degenerate)
            assert r["random"][0] in (0, 1) and r["random"][1] is not True, r
            if n >= 20:
                assert r["one_late"] == (1, False), r
        if name == "out_3":
            # (one point d away lifts the smallest eigenvalue by less than d^2: 9 thr^2 is below n thrblk^2 from n = 9 on; at
            #  six and seven points 3 x thr is about the line itself - 7.5 against 6.1 thr^2 before the point's leverage - and
            #  the model says either)
            assert r["random"][0] in (0, 1), r
            if n >= 20:
                assert r["random"] == (1, False) and r["one_late"] == (1, False), r
        if name in ("far1_dyadic", "far2_dyadic", "dup_positions"):
            # the zero plane of hypothesis 700 holds every point; group 0 and the certificate are as under `random`
            for kind in ("zero_one", "zero_two"):
                assert r[kind] == r["random"] and (r[kind][1] is True or n < 20), r
                o = oracle_of(kind)
                # (small blocks: a hypothesis of the random table in front of 700 may draw two positions as well)
                first = 600 if (name == "dup_positions" and kind == "zero_two") else 700
                assert o[1][i] == n and not o[2][i].any() and (o[3][i] == first or (n < 20 and 64 <= o[3][i] < first)), (r, kind)
            if n >= 20:     # (no zero plane in the random table from 20 points on: the certified L is final)
                assert oracle_of("random")[1][i] == n - r["random"][0] and oracle_of("random")[3][i] < 64
        if name == "dup_positions":
            pos = _pos(_draws("zero_two")[600], n)
            assert np.array_equal(pts[pos[0]], pts[pos[1]])
            assert not pcm.vouched(pts, pos[None, :])[0]
            if n >= 20:
                assert len(set(pos.tolist())) == 3
        if name.startswith("collinear"):
            pos = _pos(H800, n)
            assert len(set(pos.tolist())) == 3
            assert bool(pcm.vouched(pts, pos[None, :])[0]) == name.endswith("above"), r
            for kind in ("zero_one", "zero_two"):
                assert r[kind] == r["random"], r
        if name == "second_plane":
            assert r["one_late"] == (2, False), r
            assert oracle_of("one_late")[1][i] == n - 1 and oracle_of("one_late")[3][i] == 1000, r
        if name == "late_holds_all":
            assert r["one_late"] == (1, False), r
            assert oracle_of("one_late")[1][i] == n and oracle_of("one_late")[3][i] == 1000, r
    assert seen == {(name, n) for name in DIRECTED for n in SIZES if n >= 20 or name not in ("second_plane", "late_holds_all")}
    # the generic leaves hold certified blocks of both kinds under the benchmark's kind of table
    draws = _draws("random")
    gen = [pcm.certified(blocks[i], THR, _group0(blocks[i], draws)) for i in np.flatnonzero(names == "generic")[:400]]
    b = [int(sizes[i]) - _group0(blocks[i], draws) for i in np.flatnonzero(names == "generic")[:400]]
    cert = [bb for bb, c in zip(b, gen) if c]
    print(f"generic leaves (400): tested {sum(c is not None for c in gen)}, certified at b = 1: {cert.count(1)}, "
          f"at b = 2: {cert.count(2)}")
    assert cert.count(1) >= 20 and cert.count(2) >= 10


@pytest.mark.gpu
def test_directed_blocks_are_what_they_claim():
    check_directed_blocks(_oracle)
    # ... and the library's winners on them are the oracle's (prescreen on)
    for kind in KINDS:
        o = _oracle(kind)
        got = _library(kind)[0]
        assert np.array_equal(got[2][:N_CHECKED], o[1]) and np.array_equal(got[3][:N_CHECKED], o[3])
