"""NotPlanar (octreelib_amd.criteria): the host callable that defines the planarity criterion, its recognition for
the device path, and the oracle arm the GPU tests compare with (tests/test_gpu_planarity.py)."""

import os
import sys

import numpy as np
import pytest

from octreelib_amd import MaxPoints, NotPlanar, synthetic
from octreelib_amd.criteria import try_count_threshold, try_planar_threshold
from oracle import octree_np as onp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _direct(points, max_variance, min_points, ddof):
    """The criterion straight from its definition."""
    p = np.asarray(points, dtype=np.float64)
    n = len(p)
    if n < min_points:
        return False
    m = p.sum(axis=0) / n
    c = np.zeros((3, 3))
    for row in p - m:
        c += np.outer(row, row)
    return bool(np.linalg.eigvalsh(c / (n - ddof))[0] > max_variance)


def _clouds():
    rng = np.random.default_rng(11)
    flat = rng.random((500, 3))
    flat[:, 2] = 0.25 + 1e-4 * rng.standard_normal(500)
    line = np.outer(rng.random(200), [1.0, 2.0, -1.0]) + [5.0, 5.0, 5.0]
    return {
        "random": rng.random((400, 3)),
        "planar": flat,
        "collinear": line,
        "duplicates": np.tile([[0.3, 0.4, 0.5]], (64, 1)),
        "few": rng.random((7, 3)),
        "empty": np.empty((0, 3)),
        "far": rng.random((300, 3)) * 0.5 + 5e6,
    }


@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("max_variance", [1e-9, 1e-6, 1e-3, 0.05])
def test_call_matches_direct_formula(max_variance, ddof):
    crit = NotPlanar(max_variance, 8, ddof)
    for name, pts in _clouds().items():
        assert crit(pts) == _direct(pts, max_variance, 8, ddof), name
    # the expected answers, not only agreement
    c = _clouds()
    assert NotPlanar(1e-3)(c["random"]) and not NotPlanar(1e-3)(c["planar"])
    assert not NotPlanar(1e-9)(c["collinear"]) and not NotPlanar(1e-9)(c["duplicates"])
    assert not NotPlanar(1e-9)(c["few"]) and not NotPlanar(1e-9)(c["empty"])
    assert NotPlanar(1e-9, min_points=4)(c["few"])


def test_far_from_origin_is_shift_invariant():
    rng = np.random.default_rng(3)
    p = rng.random((256, 3)) * 0.25
    a = NotPlanar(1e-3).smallest_eigenvalue(p)
    b = NotPlanar(1e-3).smallest_eigenvalue(p + 4194304.0)   # (a power of two: the shifted rows are exact)
    assert abs(a - b) <= 1e-12 * a


@pytest.mark.parametrize("args", [(0.0,), (-1.0,), (float("nan"),), (float("inf"),), (1e-3, 3), (1e-3, 2.5),
                                  (1e-3, 8, 2), (1e-3, 8, -1)])
def test_constructor_rejects(args):
    with pytest.raises(ValueError):
        NotPlanar(*args)


def test_constructor_accepts():
    c = NotPlanar(2.5e-4)
    assert (c.max_variance, c.min_points, c.ddof) == (2.5e-4, 8, 0)
    c = NotPlanar(1, min_points=4, ddof=1)
    assert (c.max_variance, c.min_points, c.ddof) == (1.0, 4, 1)


@pytest.mark.parametrize("ddof", [0, 1])
def test_depth_bound(ddof):
    """No node with e^2 / 3 <= max_variance splits, whatever the points: the worst cloud of a cube (its corners,
    duplicated) stays below, and a cube of duplicates of ONE point never splits at all."""
    e = 0.5
    corners = np.array([[x, y, z] for x in (0, e) for y in (0, e) for z in (0, e)], dtype=float)
    for reps in (1, 2, 100):
        worst = np.tile(corners, (reps, 1))
        assert not NotPlanar(e * e / 3, min_points=4, ddof=ddof)(worst)
    t = onp.OTree(np.zeros(3), 1.0)
    t.insert_points(np.tile([[0.3, 0.4, 0.5]], (1000, 1)))
    t.subdivide([NotPlanar(1e-300, ddof=ddof)])
    assert t.n_nodes == 1


# ---- recognition -------------------------------------------------------------------------------------------------
class _Renamed(NotPlanar):
    pass


class _Overriding(NotPlanar):
    def __call__(self, points):
        return len(points) > 3


def test_recognition():
    p = NotPlanar(2.5e-4, 8)
    assert try_planar_threshold([p]) == (-1, 2.5e-4, 8, 0)
    assert try_planar_threshold([p, MaxPoints(2000)]) == (2000, 2.5e-4, 8, 0)
    assert try_planar_threshold([MaxPoints(2000), lambda points: len(points) > 500, p]) == (500, 2.5e-4, 8, 0)
    assert try_planar_threshold([lambda pts: len(pts) >= 100, NotPlanar(1e-3, 16, 1)]) == (99, 1e-3, 16, 1)
    assert try_planar_threshold([_Renamed(1e-3, 9)]) == (-1, 1e-3, 9, 0)
    # several planar rules: the OR reduces to one when they differ in the threshold only
    assert try_planar_threshold([NotPlanar(1e-3), NotPlanar(5e-4), MaxPoints(7)]) == (7, 5e-4, 8, 0)
    assert try_planar_threshold([NotPlanar(1e-3, 8), NotPlanar(5e-4, 16)]) is None
    assert try_planar_threshold([NotPlanar(1e-3, 8, 0), NotPlanar(1e-3, 8, 1)]) is None


def test_recognition_refuses():
    p = NotPlanar(2.5e-4, 8)
    assert try_planar_threshold([lambda points: p(points)]) is None        # a wrapping lambda: the host path
    assert try_planar_threshold([_Overriding(1e-3)]) is None
    assert try_planar_threshold([p, _Overriding(1e-3)]) is None
    assert try_planar_threshold([p, lambda points: points.std() > 1]) is None
    shadowed = NotPlanar(1e-3)
    shadowed.__call__ = lambda points: True
    assert try_planar_threshold([shadowed]) is None
    # no planar criterion at all: not this function's business
    assert try_planar_threshold([MaxPoints(5)]) is None
    assert try_planar_threshold([]) is None


def test_count_lists_unchanged():
    for crit, want in (([MaxPoints(5)], 5), ([lambda points: len(points) > 64], 64), ([], -1),
                       ([MaxPoints(9), lambda points: len(points) >= 4], 3)):
        assert try_count_threshold(crit) == want
    assert try_count_threshold([NotPlanar(1e-3)]) is None
    assert try_count_threshold([lambda points: NotPlanar(1e-3)(points)]) is None


# ---- the oracle arm, pinned against the reference ------------------------------------------------------------------
def _oracle_table(og, pose):
    return sorted((c.tobytes(), e.tobytes(), tuple(sorted(i.tolist()))) for c, e, i in og.leaf_table(pose))


def test_oracle_builds_planar_trees():
    """The scene and figures the GPU tests rely on: evaluated nodes, leaves, and how close any statistic comes to the
    threshold (the GPU comparison is exact only because nothing is within 1e-9 e^2 of it)."""
    pts = synthetic.planar_cloud(60000, dims=(4, 4, 4), seed=1)
    crit = NotPlanar(2.5e-4, 8)
    seen = []

    def spy(points):
        if len(points) >= crit.min_points:
            seen.append(crit.smallest_eigenvalue(points))
        return crit(points)

    og = onp.OGrid(1)
    og.insert_points(0, pts)
    og.subdivide([spy, lambda points: len(points) > 2000])
    assert og.n_points(0) == len(pts)
    assert len(seen) == 4147 and og.n_nodes(0) == 13480 and og.n_leaves(0) == 8764
    plain = onp.OGrid(1)
    plain.insert_points(0, pts)
    plain.subdivide([crit, MaxPoints(2000)])
    assert _oracle_table(plain, 0) == _oracle_table(og, 0)


def _reference():
    sys.path.insert(0, os.path.join(ROOT, "tools", "refshim"))
    import refshim

    if not os.path.isdir(refshim.REFERENCE_ROOT):
        pytest.skip("the reference implementation is not on this machine")
    refshim.install()
    from octreelib.grid import Grid, GridConfig
    from octreelib.octree import Octree, OctreeConfig
    from octreelib.octree_manager import OctreeManager

    return Grid, GridConfig, Octree, OctreeConfig, OctreeManager


@pytest.mark.reference
@pytest.mark.parametrize("ddof", [0, 1])
def test_reference_and_oracle_agree(ddof):
    Grid, GridConfig, Octree, OctreeConfig, OctreeManager = _reference()
    crit = [NotPlanar(2.5e-4, 8, ddof), MaxPoints(800)]
    clouds = {p: synthetic.planar_cloud(6000, dims=(2, 2, 2), seed=1, stream=p) for p in (0, 1)}
    ref = Grid(GridConfig(octree_manager_type=OctreeManager, octree_type=Octree, octree_config=OctreeConfig(),
                          voxel_edge_length=1))
    og = onp.OGrid(1)
    for p, pts in clouds.items():
        ref.insert_points(p, pts)
        og.insert_points(p, pts)
    ref.subdivide(crit)
    og.subdivide(crit)
    for p, pts in clouds.items():
        index = {pts[i].tobytes(): i for i in range(len(pts))}
        got = sorted((np.asarray(v.corner_min, dtype=np.float64).tobytes(), np.float64(v.edge_length).tobytes(),
                      tuple(sorted(index[r.tobytes()] for r in v.get_points()))) for v in ref.get_leaf_points(p))
        assert got == _oracle_table(og, p)
        assert ref.n_nodes(p) == og.n_nodes(p) and ref.n_leaves(p) == og.n_leaves(p)
        assert ref.n_points(p) == og.n_points(p) == len(pts)
    assert og.n_nodes(0) > 50
