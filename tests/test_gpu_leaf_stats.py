"""Per-leaf point statistics on the device (octl_forest_leaf_stats, octl_debug_sym3_eigen; Grid / OctreeManager /
Octree.leaf_statistics).

The contract: with eps = 2^-53, R = max over a block of |p - p0|_inf (p0 = the block's first point in storage order)
and gamma = (ceil(n/64) + ceil(n/L) + 16) eps, the count is exact, every mean component is within 2 gamma R + eps |m|
of the exact mean and every covariance entry within 4 gamma R^2 of the exact population covariance; the eigen-
decomposition is orthonormal to 64 eps, its residuals and eigenvalues within 64 eps ||C||_F, ascending, under the
sign rule; and a block's results are the same bits however it is requested and whatever happens to other blocks."""

import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from octreelib_amd import MaxPoints
from octreelib_amd import _native as nat
from octreelib_amd._engine import Forest
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.leaf_stats import LeafStatistics, cov6_to_full, leaf_statistics_np
from octreelib_amd.octree import Octree, OctreeConfig
from octreelib_amd.octree_manager import OctreeManager

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
L = 64 * 64
_UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


# ---- helpers ---------------------------------------------------------------------------------------------------
def _gamma(n):
    return (math.ceil(n / 64) + math.ceil(n / L) + 16) * EPS


def _extent(P):
    P = np.asarray(P, dtype=np.longdouble)
    return float(np.abs(P - P[0]).max()) if len(P) else 0.0


def _exact(P):
    """Exact mean and population covariance (Fractions) of the f64 rows of P."""
    rows = [[Fraction(float(x)) for x in p] for p in np.asarray(P, dtype=np.float64)]
    n = len(rows)
    m = [sum(r[a] for r in rows) / n for a in range(3)]
    c = [sum((r[i] - m[i]) * (r[j] - m[j]) for r in rows) / n for i, j in _UPPER]
    return m, c


def _assert_within_bound(st, i, P, mean_ref, cov6_ref, what=""):
    """Bound 1 for row i of st against reference moments of the rows P (exact Fractions or longdouble)."""
    n = len(P)
    assert int(st.count[i]) == n, what
    R = _extent(P)
    g = _gamma(n)
    for a in range(3):
        m = mean_ref[a]
        err = abs(Fraction(float(st.mean[i, a])) - Fraction(m)) if isinstance(m, Fraction) else \
            abs(np.longdouble(st.mean[i, a]) - np.longdouble(m))
        assert float(err) <= 2 * g * R + EPS * abs(float(m)), (what, i, a, float(err), R)
    for k, (a, b) in enumerate(_UPPER):
        c = cov6_ref[k]
        err = abs(Fraction(float(st.covariance[i, a, b])) - Fraction(c)) if isinstance(c, Fraction) else \
            abs(np.longdouble(st.covariance[i, a, b]) - np.longdouble(c))
        assert float(err) <= 4 * g * R * R, (what, i, k, float(err), R)


def _assert_matches_leaves(st, leaves, what=""):
    """Rows line up with the leaves: counts equal, mean and covariance within bound 1 of a longdouble reference."""
    assert len(st) == len(leaves), what
    pts = [v.get_points() for v in leaves]
    ref = leaf_statistics_np(pts, dtype=np.longdouble, eigen=False)
    for i, P in enumerate(pts):
        c6 = [ref.covariance[i, a, b] for a, b in _UPPER]
        _assert_within_bound(st, i, P, ref.mean[i], c6, what)


def _assert_eigen(w, v, cov, gap_check=True):
    """Eigen contract for (n,3) values, (n,3,3) vectors of the (n,3,3) matrices cov (the device's own covariance)."""
    n = len(w)
    if n == 0:
        return
    fn = np.sqrt((cov ** 2).sum(axis=(1, 2)))
    assert np.all(w[:, 0] <= w[:, 1]) and np.all(w[:, 1] <= w[:, 2])
    assert np.abs(np.einsum("nki,nkj->nij", v, v) - np.eye(3)).max(axis=(1, 2)).max() <= 64 * EPS
    res = np.linalg.norm(np.einsum("nij,njk->nik", cov, v) - v * w[:, None, :], axis=1)
    assert np.all(res <= 64 * EPS * fn[:, None])
    # LAPACK on the matrices scaled by a power of two (exact): unscaled, it loses accuracy on entries far apart
    s = np.ldexp(1.0, -np.frexp(np.abs(cov).max(axis=(1, 2)))[1])
    s[~np.isfinite(s) | (fn == 0)] = 1.0
    we, ve = np.linalg.eigh(cov * s[:, None, None])
    we = we / s[:, None]
    assert np.all(np.abs(w - we) <= 64 * EPS * fn[:, None])
    for col in range(3):   # sign rule
        x = v[:, :, col]
        k = np.argmax(np.abs(x), axis=1)
        assert np.all(x[np.arange(n), k] > 0)
    if gap_check:
        gap = w[:, 1] - w[:, 0]
        sel = gap > 1e-6 * fn
        dots = np.abs(np.einsum("ni,ni->n", v[sel, :, 0], ve[sel, :, 0]))
        tol = 1e3 * EPS * fn[sel] / gap[sel] + 1e-12
        assert np.all(dots >= 1.0 - tol)


def _stats_bytes(st):
    return (st.count.tobytes(), st.mean.tobytes(), st.covariance.tobytes(), st.eigenvalues.tobytes(),
            st.eigenvectors.tobytes())


def _row(st, i):
    return (st.count[i].tobytes(), st.mean[i].tobytes(), st.covariance[i].tobytes(), st.eigenvalues[i].tobytes(),
            st.eigenvectors[i].tobytes())


def _launches():
    c = C.c_uint64(0)
    nat.load().octl_debug_launches(C.byref(c))
    return c.value


def _planar_grid(n=60000, K=64, seed=3, inliers=0.8):
    from octreelib_amd import synthetic

    P = synthetic.planar_cloud(n, (4, 4, 2), seed=seed, sigma=0.001, inlier_fraction=inliers)
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P)
    g.subdivide([MaxPoints(K)])
    return g, P


# ---- bound 1 against exact arithmetic ----------------------------------------------------------------------------
def test_small_blocks_against_fractions():
    g, _ = _planar_grid(n=20000, K=64, seed=5)
    st = g.leaf_statistics(0)
    leaves = g.get_leaf_points(0)
    assert len(st) == len(leaves) > 300
    pick = np.random.default_rng(0).choice(len(leaves), 300, replace=False)
    for i in pick.tolist():
        P = leaves[i].get_points()
        m, c = _exact(P)
        _assert_within_bound(st, i, P, m, c, "fraction")
    _assert_eigen(st.eigenvalues, st.eigenvectors, st.covariance)


# ---- bound 2: UTM-sized coordinates ------------------------------------------------------------------------------
def _utm_scene(seed, origin):
    rng = np.random.default_rng(seed)
    n = 40000
    xy = rng.random((n, 2)) * 2.0
    z = 0.3 + 0.2 * xy[:, 0] - 0.1 * xy[:, 1] + rng.normal(0.0, 0.001, n)
    return np.column_stack([xy, z]) + np.asarray(origin, dtype=np.float64)


def test_offset_robustness_grid():
    origin = (5.0e6, 5.0e6 + 17.0, 5.0e6 + 3.0)
    P = _utm_scene(11, origin)
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, P)
    g.subdivide([MaxPoints(200)])
    st = g.leaf_statistics(0)
    leaves = g.get_leaf_points(0)
    assert max(v.edge_length for v in leaves) <= 0.25
    _assert_matches_leaves(st, leaves, "utm grid")
    _assert_eigen(st.eigenvalues, st.eigenvectors, st.covariance)
    # the normals are the scene's plane normal (the leaves are thin slabs of it)
    nrm = np.array([-0.2, 0.1, 1.0]) / np.linalg.norm([-0.2, 0.1, 1.0])
    big = st.count >= 50
    assert np.median(np.abs(st.normal[big] @ nrm)) > 0.99


def test_offset_robustness_manager():
    origin = (5.0e6 - 1.0, 5.0e6 - 1.0, 5.0e6 - 1.0)
    P = _utm_scene(12, np.asarray(origin) + 1.0)
    m = OctreeManager(Octree, OctreeConfig(), np.asarray(origin), 4.0)
    m.insert_points(7, P)
    m.subdivide([MaxPoints(200)])
    st = m.leaf_statistics(7)
    _assert_matches_leaves(st, m.get_leaf_points(True, 7), "utm manager")
    _assert_eigen(st.eigenvalues, st.eigenvectors, st.covariance)


# ---- bound 3: the eigensolver alone ------------------------------------------------------------------------------
def _sym3(c6):
    ctx = nat.get_context()
    c6 = np.ascontiguousarray(c6, dtype=np.float64).reshape(-1, 6)
    w = np.empty((len(c6), 3))
    v = np.empty((len(c6), 3, 3))
    ctx.check(ctx.lib.octl_debug_sym3_eigen(ctx.handle, nat.ptr(c6), len(c6), nat.ptr(w), nat.ptr(v)))
    return w, v, cov6_to_full(c6)


def _from_eig(lam, seed):
    Q = np.linalg.qr(np.random.default_rng(seed).standard_normal((len(lam), 3, 3)))[0]
    A = np.einsum("nij,nj,nkj->nik", Q, lam, Q)
    return np.stack([A[:, a, b] for a, b in _UPPER], axis=1)


def test_sym3_eigen_adversarial():
    rng = np.random.default_rng(1)
    # zero: eigenvalues 0, identity columns
    w, v, _ = _sym3(np.zeros((1, 6)))
    assert np.all(w == 0) and np.array_equal(v[0], np.eye(3))
    # diagonal with repeated values: sorted, ties keep Jacobi's column order -> identity columns for a sorted diagonal
    w, v, A = _sym3([[1, 0, 0, 1, 0, 2.0], [2, 0, 0, 2, 0, 2.0], [3, 0, 0, 1, 0, 2.0]])
    assert np.array_equal(w, [[1, 1, 2], [2, 2, 2], [1, 2, 3]])
    assert np.array_equal(v[0], np.eye(3)) and np.array_equal(v[1], np.eye(3))
    assert np.array_equal(v[2], np.eye(3)[:, [1, 2, 0]])
    _assert_eigen(w, v, A, gap_check=False)
    cases = {
        "rank1": (lambda u: np.stack([u[:, a] * u[:, b] for a, b in _UPPER], axis=1))(rng.standard_normal((500, 3))),
        "rank2": _from_eig(np.tile([0.0, 1.0, 2.0], (500, 1)), 2),
        "planar": _from_eig(np.tile([1e-8, 1e-3, 2e-3], (500, 1)), 3),
        "equal_ulp": _from_eig(np.tile([1.0, 1.0, np.nextafter(1.0, 2.0)], (500, 1)), 4),
        "span": rng.standard_normal((2000, 6)) * 10.0 ** rng.uniform(-150, 150, (2000, 6)),
        "random": rng.standard_normal((100000, 6)),
    }
    for name, c6 in cases.items():
        w, v, A = _sym3(c6)
        _assert_eigen(w, v, A, gap_check=name not in ("equal_ulp", "span"))


# ---- bound 4: purity ---------------------------------------------------------------------------------------------
def test_same_bits_however_requested():
    g, _ = _planar_grid(n=30000, K=32, seed=7)
    f = g._forest
    ids = f.slot_blocks(0)
    full = f.leaf_stats(ids)
    assert _stats_bytes(full) == _stats_bytes(f.leaf_stats(ids))   # repeated call
    rev = f.leaf_stats(ids[::-1])
    rep = f.leaf_stats(np.concatenate([ids, ids[:50], ids[:50]]))
    for i in range(0, len(ids), max(1, len(ids) // 40)):
        alone = f.leaf_stats(ids[i : i + 1])
        assert _row(alone, 0) == _row(full, i)
        assert _row(rev, len(ids) - 1 - i) == _row(full, i)
    for i in range(50):
        assert _row(rep, len(ids) + i) == _row(full, i) == _row(rep, len(ids) + 50 + i)
    assert len(f.leaf_stats(np.empty(0, dtype=np.int32))) == 0


def _by_leaf(f, st, ids):
    blk = f.blocks
    return {(int(blk["node"][b]), int(blk["slot"][b])): _row(st, i) for i, b in enumerate(ids.tolist())}


def test_same_bits_after_other_leaves_change():
    g, _ = _planar_grid(n=40000, K=64, seed=9, inliers=0.97)
    f = g._forest
    ids = f.slot_blocks(0)
    before = _by_leaf(f, f.leaf_stats(ids), ids)
    sizes = f.blocks["size"][ids]
    # filter: the leaves with fewer than 20 points leave the tree
    g.filter([lambda p: len(p) >= 20])
    ids2 = f.slot_blocks(0)
    after = _by_leaf(f, f.leaf_stats(ids2), ids2)
    assert len(after) == int((sizes >= 20).sum()) and len(after) < len(before)
    for k, row in after.items():
        assert row == before[k]
    # an engine-level host mask that touches only other blocks: drop half of every third block's points
    blk = f.blocks
    mask = np.ones(f.n_ord, dtype=np.uint8)
    touched = set()
    for j, b in enumerate(ids2.tolist()):
        if j % 3 == 0 and blk["size"][b] >= 4:
            s, z = int(blk["start"][b]), int(blk["size"][b])
            mask[s : s + z // 2] = 0
            touched.add((int(blk["node"][b]), int(blk["slot"][b])))
    f.apply_host_mask(mask)
    ids3 = f.slot_blocks(0)
    after3 = _by_leaf(f, f.leaf_stats(ids3), ids3)
    untouched = [k for k in after3 if k not in touched]
    assert len(untouched) > 50
    for k in untouched:
        assert after3[k] == before[k]
    # RANSAC + apply_mask: the blocks whose mask kept every point keep their bits
    np.random.seed(0)
    table = np.random.random((256, 6))
    blk = f.blocks
    f.ransac_blocks(ids3, table, 0.01)
    m = f.device_mask()
    full_keep = {(int(blk["node"][b]), int(blk["slot"][b])) for b in ids3.tolist()
                 if m[int(blk["start"][b]) : int(blk["start"][b]) + int(blk["size"][b])].all()}
    # a pending mask is not applied by leaf_stats
    assert _by_leaf(f, f.leaf_stats(ids3), ids3) == after3
    f.apply_device_mask()
    ids4 = f.slot_blocks(0)
    after4 = _by_leaf(f, f.leaf_stats(ids4), ids4)
    kept = [k for k in after4 if k in full_keep]
    assert len(kept) > 10
    for k in kept:
        assert after4[k] == after3[k]


# ---- bound 5: layout ---------------------------------------------------------------------------------------------
def test_rows_line_up_multi_pose_grid():
    from octreelib_amd import synthetic

    g = Grid(GridConfig(voxel_edge_length=1))
    for p in range(3):
        g.insert_points(p, synthetic.planar_cloud(8000, (3, 3, 2), seed=1, stream=p))
    g.subdivide([MaxPoints(48)], pose_numbers=[0, 1])
    g.insert_points(5, synthetic.planar_cloud(6000, (3, 3, 2), seed=1, stream=5))   # late pose: incremental
    for p in (0, 1, 2, 5):
        st = g.leaf_statistics(p)
        _assert_matches_leaves(st, g.get_leaf_points(p), f"pose {p}")
        _assert_eigen(st.eigenvalues, st.eigenvectors, st.covariance)
    with pytest.raises(KeyError):
        g.leaf_statistics(4)
    g.insert_points(9, np.empty((0, 3)))
    assert len(g.leaf_statistics(9)) == 0


def test_rows_line_up_manager_subsets_and_octree():
    rng = np.random.default_rng(4)
    m = OctreeManager(Octree, OctreeConfig(), np.zeros(3), 8.0)
    for p in (3, 1, 2):
        m.insert_points(p, rng.random((5000, 3)) * 8.0)
    m.subdivide([MaxPoints(40)], pose_numbers=[1, 2])
    m.insert_points(1, rng.random((700, 3)) * 8.0)   # extend an existing pose
    for p in (3, 1, 2):
        _assert_matches_leaves(m.leaf_statistics(p), m.get_leaf_points(True, p), f"manager pose {p}")
    with pytest.raises(KeyError):
        m.leaf_statistics(0)
    t = Octree(OctreeConfig(), np.zeros(3), 4.0)
    assert len(t.leaf_statistics()) == 0
    t.insert_points(rng.random((6000, 3)) * 4.0)
    t.subdivide([MaxPoints(30)])
    st = t.leaf_statistics()
    _assert_matches_leaves(st, t.get_leaf_points(), "octree")
    _assert_eigen(st.eigenvalues, st.eigenvectors, st.covariance)


def test_rows_line_up_after_map_leaf_points():
    g, _ = _planar_grid(n=20000, K=64, seed=13)

    def fn(p):
        if len(p) % 3 == 0:
            return p[: len(p) // 2] + np.array([0.0, 0.0, 0.3])   # fewer rows, moved (some leave their cube)
        if len(p) % 3 == 1:
            return np.vstack([p, p[:1] + 2.0])                     # one displaced row more
        return p[::-1]

    g.map_leaf_points(fn)
    st = g.leaf_statistics(0)
    _assert_matches_leaves(st, g.get_leaf_points(0), "map_leaf_points")
    _assert_eigen(st.eigenvalues, st.eigenvectors, st.covariance)


# ---- bound 6: large blocks ---------------------------------------------------------------------------------------
def test_large_blocks():
    sizes = [1, 2, 3, 63, 64, 65, L - 1, L, L + 1, 2 * L + 1]
    rng = np.random.default_rng(21)
    parts = [rng.random((n, 3)) * 0.9 + np.array([2.0 * i, 0.0, 0.0]) + 0.05 for i, n in enumerate(sizes)]
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, np.vstack(parts)[rng.permutation(sum(sizes))])
    st = g.leaf_statistics(0)   # (no subdivide: one leaf per voxel)
    leaves = g.get_leaf_points(0)
    assert sorted(st.count.tolist()) == sorted(sizes)
    _assert_matches_leaves(st, leaves, "sizes")
    _assert_eigen(st.eigenvalues, st.eigenvectors, st.covariance, gap_check=False)
    # one unsubdivided voxel of 2 * 10^6 points
    g2 = Grid(GridConfig(voxel_edge_length=1))
    P = rng.random((2_000_000, 3)) * np.array([1.0, 1.0, 0.01]) + np.array([3.0, 4.0, 5.5])
    g2.insert_points(0, P)
    st2 = g2.leaf_statistics(0)
    assert st2.count.tolist() == [2_000_000]
    _assert_matches_leaves(st2, g2.get_leaf_points(0), "2M")
    _assert_eigen(st2.eigenvalues, st2.eigenvectors, st2.covariance)
    assert abs(st2.normal[0] @ np.array([0.0, 0.0, 1.0])) > 1 - 1e-6
    # the same block alone, and among the small ones of another call: the same bits
    f = g2._forest
    assert _row(f.leaf_stats([0]), 0) == _row(st2, 0) == _row(f.leaf_stats([0, 0, 0]), 2)


# ---- bound 7: float32 input --------------------------------------------------------------------------------------
def test_float32_input_same_bits():
    from octreelib_amd import synthetic

    P32 = synthetic.planar_cloud(30000, (3, 3, 3), seed=2).astype(np.float32)
    out = []
    for P in (P32, P32.astype(np.float64)):
        g = Grid(GridConfig(voxel_edge_length=1))
        g.insert_points(0, P)
        g.subdivide([MaxPoints(64)])
        out.append(_stats_bytes(g.leaf_statistics(0)))
    assert out[0] == out[1]


# ---- bound 8: errors, launches, the plug path --------------------------------------------------------------------
def test_errors():
    f = Forest(0, np.zeros(3), 1.0)
    try:
        ids = np.zeros(1, dtype=np.int32)
        cnt = np.empty(1, dtype=np.int64)
        with pytest.raises(RuntimeError):
            f.ctx.check(f.lib.octl_forest_leaf_stats(f.handle, nat.ptr(ids), 1, nat.ptr(cnt), None, None, None, None))
        f.add_pose(np.random.default_rng(0).random((100, 3)) * 3)
        nb = len(f.blocks["size"])
        with pytest.raises(ValueError, match="out of range"):
            f.leaf_stats([nb])
        with pytest.raises(ValueError, match="out of range"):
            f.leaf_stats([0, -1])
        assert len(f.leaf_stats([0])) == 1
    finally:
        f.close()
    # the classes build on demand: one leaf per voxel before any subdivide
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, np.random.default_rng(1).random((1000, 3)) * 4)
    st = g.leaf_statistics(0)
    assert len(st) == len(g.get_leaf_points(0)) == 64 and int(st.count.sum()) == 1000


@pytest.mark.parametrize("K", [None, 4])
def test_launches_constant(K):
    from octreelib_amd import synthetic

    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, synthetic.uniform_cloud(500_000, (64, 64, 32), seed=3))
    if K is not None:
        g.subdivide([MaxPoints(K)])
    f = g._forest
    ids = f.slot_blocks(0)
    assert len(ids) >= 100_000
    f.leaf_stats(ids[:1])   # (warm: scratch allocated)
    counts = []
    for sel in (ids[:1], ids, ids[:0]):
        a = _launches()
        f.leaf_stats(sel)
        counts.append(_launches() - a)
    assert counts[0] == counts[1] and 1 <= counts[0] <= 4 and counts[2] == 0, counts


class _PlugManager(OctreeManager):
    pass


def test_plug_path_matches_device():
    from octreelib_amd import synthetic

    P = synthetic.planar_cloud(6000, (2, 2, 2), seed=8)
    dev = Grid(GridConfig(voxel_edge_length=1))
    plug = Grid(GridConfig(voxel_edge_length=1, octree_manager_type=_PlugManager))
    for g in (dev, plug):
        g.insert_points(0, P)
        g.subdivide([MaxPoints(64)])
    a, b = dev.leaf_statistics(0), plug.leaf_statistics(0)
    assert isinstance(b, LeafStatistics) and np.array_equal(a.count, b.count)
    leaves = plug.get_leaf_points(0)
    for i, v in enumerate(leaves):
        Q = v.get_points()
        _assert_within_bound(a, i, Q, b.mean[i], [b.covariance[i, x, y] for x, y in _UPPER], "plug")
    with pytest.raises(KeyError):
        plug.leaf_statistics(3)
