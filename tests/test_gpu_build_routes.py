"""
Which route a build request takes through forest_build (octreelib_amd/csrc/build.hip), and what it costs.

The parity tests compare results; nothing else pins the ROUTE of a request - incremental insertion, bucket build
(complete, with voxels left to the level loop, handed back), the general level-synchronous route (roots made on the
device, union with the previous scheme's voxels on the host, fresh single cube, prefix partition and its fallback),
planar - or what the route leaves behind for the calls that follow (fast_order_valid: does order.hip run;
max_block_hint: which kernel variants RANSAC and the leaf statistics pick).  A slip there changes speed and no result.

Every scenario runs in a context of its own (the hints and the speculation state of other tests cannot reach it) and
asserts
  (a) the result against the NumPy oracle,
  (b) the set of timing labels of the build,
  (c) the kernel launches and host waits of the build (octl_debug_launches, octl_debug_host_syncs),
  (d) every field of BuildInfo,
  (e) labels, launches and waits of a follow-up leaf_stats + RANSAC + apply_mask on the built forest ("ransac_order"
      shows fast_order_valid; "leaf_chunks" shows a max_block_hint above the chunk size of leaf_stats.hip).
(b)-(e) are literals, recorded on an MI355X from the forest_build that was one function of 640 lines (three runs,
identical), exact.  The follow-up consumes the order the build left behind, so (a) is checked on a second, identical
build in a second context.
"""

import contextlib
import ctypes as C

import numpy as np
import pytest

from tests._util import _oracle_nodes, assert_same_leaves, canon_from_list
from tests.test_gpu_parity import crit, index_map, views_table

pytestmark = pytest.mark.gpu

OUTSIDE = "outside the cube of a node that is being subdivided"


# ---- measuring -----------------------------------------------------------------------------------------------------
def _counter(name):
    from octreelib_amd import _native as nat

    c = C.c_uint64(0)
    getattr(nat.load(), name)(C.byref(c))
    return c.value


@contextlib.contextmanager
def _own_context(options):
    from octreelib_amd import _native as nat

    ctx = nat.Context(0)
    try:
        for name, value in options.items():
            ctx.set_option(name, value)
        with nat.use_context(ctx):
            yield ctx
    finally:
        ctx.close()


def _measure(ctx, action, raises=None):
    """(timing labels, kernel launches, host waits) of action()."""
    ctx.sync()
    ctx.set_profiling(True)
    try:
        l0, s0 = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
        if raises is None:
            action()
        else:
            with pytest.raises(raises[0], match=raises[1]):
                action()
        l1, s1 = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
        labels = sorted(ctx.timings())
    finally:
        ctx.set_profiling(False)
    return " ".join(labels), l1 - l0, s1 - s0


INFO_FIELDS = ("n_points", "n_voxels", "n_nodes", "n_internal", "n_blocks", "max_depth", "n_levels")


def _info(forest):
    i = forest.info
    return tuple(int(getattr(i, k)) for k in INFO_FIELDS)


def _follow_up(forest):
    nb = int(forest.info.n_blocks)
    if nb:
        forest.leaf_stats(np.arange(nb, dtype=np.int32))
    forest.ransac_all(10, np.random.default_rng(5).random((64, 6)), 0.01)
    forest.apply_device_mask()
    forest.n_ord        # (settles the mask's count)


# ---- comparing with the oracle ---------------------------------------------------------------------------------------
def _check_grid(grid, og, poses, ordered=True):
    for p, pts in poses.items():
        got = canon_from_list(views_table(grid.get_leaf_points(p), index_map(pts)))
        assert_same_leaves(got, canon_from_list(og.leaf_table(p)), ordered=ordered)
        assert [grid.n_nodes(p), grid.n_leaves(p), grid.n_points(p)] == [og.n_nodes(p), og.n_leaves(p), og.n_points(p)]


def _check_tree(leaves, counts, tree):
    """Leaves of one pose of a single cube (Octree, or one pose of an OctreeManager) against its oracle OTree."""
    from oracle import octree_np as onp

    got = canon_from_list(views_table(leaves, index_map(tree.points)))
    assert_same_leaves(got, canon_from_list(onp.tree_leaf_table(tree)))
    assert list(counts) == [tree.n_nodes, tree.n_leaves, tree.n_points]


def _grid_cloud(n, stream=0):
    from octreelib_amd import synthetic

    return synthetic.planar_cloud(n, (3, 3, 3), seed=1, stream=stream)


def _deep_cluster():
    """40 points inside a cube of edge 2^-10: no K below 40 separates them within the bucket kernel's levels."""
    return np.array([1.25, 1.25, 1.25]) + np.random.default_rng(2).random((40, 3)) * 2.0 ** -10


# ---- the scenarios: setup() -> (forest, [(step, action)], check) -----------------------------------------------------
def _grid_fresh(cloud, K=24):
    from octreelib_amd.grid import Grid, GridConfig
    from oracle import octree_np as onp

    grid = Grid(GridConfig(voxel_edge_length=1))
    grid.insert_points(0, cloud)

    def check():
        og = onp.OGrid(1)
        og.insert_points(0, cloud)
        og.subdivide(K)
        _check_grid(grid, og, {0: cloud})

    return grid._forest, [("build", lambda: grid.subdivide(crit(K)))], check


def _grid_complete():
    return _grid_fresh(_grid_cloud(2000))


def _grid_pending():
    return _grid_fresh(np.vstack([_grid_cloud(2000), _deep_cluster()]))


def _in_voxel_0(pts):
    return len(pts) > 0 and bool((np.floor(pts[0]) == 0.0).all())


def _grid_again(empty_voxel=False):
    from octreelib_amd.grid import Grid, GridConfig
    from oracle import octree_np as onp

    cloud = _grid_cloud(2000)
    keep = [lambda pts: not _in_voxel_0(pts)]
    grid = Grid(GridConfig(voxel_edge_length=1))
    grid.insert_points(0, cloud)
    grid.subdivide(crit(24))
    if empty_voxel:
        grid.filter(keep)
        grid.n_points(0)

    def check():
        og = onp.OGrid(1)
        og.insert_points(0, cloud)
        og.subdivide(24)
        if empty_voxel:
            og.filter(keep)
        og.subdivide(10)
        _check_grid(grid, og, {0: cloud})
        if empty_voxel:     # the voxel that lost its points is still there, as a root without points
            assert int(grid._forest.info.n_voxels) == 27 == len(og.managers)
            assert og.managers[(0, 0, 0)].n_nodes(0) == 1 and og.managers[(0, 0, 0)].n_points(0) == 0

    return grid._forest, [("build", lambda: grid.subdivide(crit(10)))], check


def _grid_empty_voxel():
    return _grid_again(empty_voxel=True)


def _grid_poses(subdivide_first):
    """A second pose into a Grid that has (6) or has not (8: after a query) been subdivided."""
    from octreelib_amd.grid import Grid, GridConfig
    from oracle import octree_np as onp

    poses = {0: _grid_cloud(2000), 1: _grid_cloud(1200, stream=1)}
    grid = Grid(GridConfig(voxel_edge_length=1))
    grid.insert_points(0, poses[0])
    if subdivide_first:
        grid.subdivide(crit(24))
    assert grid.n_points(0) == 2000
    grid.insert_points(1, poses[1])

    def check():
        og = onp.OGrid(1)
        og.insert_points(0, poses[0])
        if subdivide_first:
            og.subdivide(24)
        og.insert_points(1, poses[1])
        _check_grid(grid, og, poses)

    return grid._forest, [("build", grid._forest.ensure_built)], check


def _grid_late_pose():
    return _grid_poses(True)


def _grid_unsplit_again():
    return _grid_poses(False)


def _manager_extend():
    from octreelib_amd.octree import Octree, OctreeConfig
    from octreelib_amd.octree_manager import OctreeManager
    from oracle import octree_np as onp

    rng = np.random.default_rng(7)
    a, b, more = rng.random((1500, 3)), rng.random((1000, 3)), rng.random((300, 3))
    m = OctreeManager(Octree, OctreeConfig(), np.zeros(3), 1.0)
    m.insert_points(0, a)
    m.insert_points(1, b)
    m.subdivide(crit(24))
    m.insert_points(0, more)      # more points for a pose that is there: every stored point is placed again

    def check():
        om = onp.OManager(np.zeros(3), 1.0)
        om.insert_points(0, a)
        om.insert_points(1, b)
        om.subdivide(24)
        om.insert_points(0, more)
        om.subdivide(10)
        for p in (0, 1):
            _check_tree(m.get_leaf_points(True, p), [m.n_nodes(p), m.n_leaves(p), m.n_points(p)], om.octrees[p])

    return m._forest, [("build", m._forest.ensure_built), ("subdivide", lambda: m.subdivide(crit(10)))], check


def _octree(cloud, K):
    from octreelib_amd.octree import Octree, OctreeConfig
    from oracle import octree_np as onp

    oc = Octree(OctreeConfig(), np.zeros(3), np.float64(1))
    oc.insert_points(cloud)

    def check():
        ot = onp.OTree(np.zeros(3), np.float64(1))
        ot.insert_points(cloud)
        ot.subdivide(K)
        _check_tree(oc.get_leaf_points(), [oc.n_nodes, oc.n_leaves, oc.n_points], ot)

    return oc._forest, [("build", lambda: oc.subdivide(crit(K)))], check


def _octree_even(K=24):
    return _octree(np.random.default_rng(9).random((3000, 3)), K)


def _octree_prefix():
    return _octree_even(K=8)      # 3000 >= 2 * 8 * 8^2: the top two levels come from the prefix partition


def _octree_uneven():
    # nearly everything in one octant: a depth-1 node with 5 points does not split, the top tree steps aside
    rng = np.random.default_rng(10)
    return _octree(np.vstack([rng.random((2995, 3)) * 0.5, 0.5 + rng.random((5, 3)) * 0.5]), 8)


def _grid_planar():
    from octreelib_amd import MaxPoints, NotPlanar
    from octreelib_amd.grid import Grid, GridConfig
    from oracle import octree_np as onp

    cloud = _grid_cloud(4000)
    plane = NotPlanar(2.5e-4, 8, 0)
    criteria = [plane, MaxPoints(200)]
    grid = Grid(GridConfig(voxel_edge_length=1))
    grid.insert_points(0, cloud)

    def check():
        og = onp.OGrid(1)
        og.insert_points(0, cloud)
        og.subdivide(criteria)
        nodes, evaluated = _oracle_nodes([m.scheme for m in og.managers.values()], plane, 200)
        assert evaluated > 27
        _check_grid(grid, og, {0: cloud})
        # the split statistics are there: one row per node, the counts the oracle's nodes hold
        f = grid._forest
        cnt, lam = f.split_stats()
        nd = f.nodes
        assert len(cnt) == int(f.info.n_nodes) == len(nodes)
        for i in range(len(cnt)):
            _e, n, _lam, internal, _rows = nodes[((nd["corner"][i] + 0.0).tobytes(), float(nd["edge"][i]))]
            assert int(cnt[i]) == n and bool(nd["first_child"][i] >= 0) == internal
            assert np.isnan(lam[i]) == (n < plane.min_points)

    return grid._forest, [("build", lambda: grid.subdivide(criteria))], check


SCENARIOS = {
    "01 grid, bucket build complete": (_grid_complete, {}),
    "02 grid, bucket build leaves a voxel to the level loop": (_grid_pending, {}),
    "03 grid, general route, roots on the device": (_grid_complete, {"NO_BUCKET_BUILD": 1}),
    "04a grid again, bucket build over the previous scheme": (_grid_again, {}),
    "04b grid again, general route, union on the host": (_grid_again, {"NO_BUCKET_HISTORY": 1}),
    "05a grid again, a voxel lost its points: bucket build hands back": (_grid_empty_voxel, {}),
    "05b grid again, a voxel lost its points: general route": (_grid_empty_voxel, {"NO_BUCKET_HISTORY": 1}),
    "06 grid, late pose: incremental insertion": (_grid_late_pose, {}),
    "07 manager, pose extended: keep_scheme re-placement": (_manager_extend, {}),
    "08 grid, second pose before any subdivide: unsplit again": (_grid_unsplit_again, {}),
    "09a octree": (_octree_even, {}),
    "09b octree, general route, fresh single cube": (_octree_even, {"NO_BUCKET_BUILD": 1}),
    "09c octree, prefix partition": (_octree_prefix, {"NO_BUCKET_BUILD": 1, "CUBE_PREFIX_MIN": 1000}),
    "10 octree, prefix partition steps aside": (_octree_uneven, {"NO_BUCKET_BUILD": 1, "CUBE_PREFIX_MIN": 1000}),
    "11 grid, planar": (_grid_planar, {}),
}

# recorded on an MI355X at the parent of the commit that split forest_build into steps.  Per measured step: (timing labels,
# kernel launches, host waits); "info": BuildInfo in the order of INFO_FIELDS
EXPECTED = {
    "01 grid, bucket build complete": {
        "build": ("bucket_build bucket_nodes bucket_scan part_hist part_scatter", 17, 4),
        "info": (2000, 27, 259, 29, 213, 2, 2),
        "follow-up": ("apply_mask leaf_eigen leaf_moments ransac ransac_prepare", 7, 3),
    },
    "02 grid, bucket build leaves a voxel to the level loop": {
        "build": (
            "blocks bucket_build bucket_nodes bucket_scan finalize level_children level_hist level_prepare "
            "level_rekey level_scan level_scatter part_hist part_scatter", 131, 17),
        "info": (2040, 27, 339, 39, 224, 11, 11),
        "follow-up": ("apply_mask leaf_eigen leaf_moments ransac ransac_order ransac_prepare", 43, 4),
    },
    "03 grid, general route, roots on the device": {
        "build": (
            "blocks finalize init_level0 keygen level_children level_hist level_prepare level_scan level_scatter "
            "linkey roots sort_hist sort_scan sort_scatter", 49, 15),
        "info": (2000, 27, 259, 29, 213, 2, 2),
        "follow-up": ("apply_mask leaf_chunks leaf_eigen leaf_moments ransac ransac_order ransac_prepare", 24, 5),
    },
    "04a grid again, bucket build over the previous scheme": {
        "build": ("bucket_build bucket_nodes bucket_scan part_hist part_scatter", 9, 4),
        "info": (2000, 27, 1019, 124, 553, 3, 3),
        "follow-up": (
            "apply_mask leaf_eigen leaf_moments ransac ransac_order ransac_prepare sort_hist sort_scan "
            "sort_scatter", 27, 3),
    },
    "04b grid again, general route, union on the host": {
        "build": (
            "blocks finalize init_level0 keygen level_children level_hist level_prepare level_scan level_scatter "
            "linkey roots sort_hist sort_scan sort_scatter", 51, 21),
        "info": (2000, 27, 1019, 124, 553, 3, 3),
        "follow-up": (
            "apply_mask leaf_chunks leaf_eigen leaf_moments ransac ransac_order ransac_prepare sort_hist "
            "sort_scan sort_scatter", 30, 4),
    },
    "05a grid again, a voxel lost its points: bucket build hands back": {
        "build": (
            "blocks bucket_build bucket_nodes bucket_scan finalize init_level0 keygen level_children level_hist "
            "level_prepare level_scan level_scatter linkey part_hist part_scatter roots sort_hist sort_scan "
            "sort_scatter", 59, 24),
        "info": (1919, 27, 979, 119, 529, 3, 3),
        "follow-up": (
            "apply_mask leaf_chunks leaf_eigen leaf_moments ransac ransac_order ransac_prepare sort_hist "
            "sort_scan sort_scatter", 30, 5),
    },
    "05b grid again, a voxel lost its points: general route": {
        "build": (
            "blocks finalize init_level0 keygen level_children level_hist level_prepare level_scan level_scatter "
            "linkey roots sort_hist sort_scan sort_scatter", 51, 21),
        "info": (1919, 27, 979, 119, 529, 3, 3),
        "follow-up": (
            "apply_mask leaf_chunks leaf_eigen leaf_moments ransac ransac_order ransac_prepare sort_hist "
            "sort_scan sort_scatter", 30, 5),
    },
    "06 grid, late pose: incremental insertion": {
        "build": ("inc_append inc_place inc_sort sort_hist sort_scan sort_scatter", 21, 13),
        "info": (3200, 27, 259, 29, 416, 2, 2),
        "follow-up": ("apply_mask leaf_chunks leaf_eigen leaf_moments ransac ransac_order ransac_prepare", 24, 4),
    },
    "07 manager, pose extended: keep_scheme re-placement": {
        "build": (
            "blocks finalize init_level0 keygen level_children level_hist level_prepare level_scan level_scatter "
            "linkey roots", 49, 17),
        "subdivide": ("bucket_build bucket_nodes bucket_scan part_hist part_scatter", 9, 3),
        "info": (2800, 1, 689, 86, 1016, 4, 4),
        "follow-up": (
            "apply_mask leaf_eigen leaf_moments ransac ransac_order ransac_prepare sort_hist sort_scan "
            "sort_scatter", 29, 5),
    },
    "08 grid, second pose before any subdivide: unsplit again": {
        "build": ("inc_append inc_place inc_sort sort_hist sort_scan sort_scatter", 18, 13),
        "info": (3200, 27, 27, 0, 54, 0, 0),
        "follow-up": ("apply_mask leaf_chunks leaf_eigen leaf_moments ransac ransac_order ransac_prepare", 20, 3),
    },
    "09a octree": {
        "build": ("bucket_build bucket_nodes bucket_scan part_hist part_scatter", 17, 4),
        "info": (3000, 1, 585, 73, 511, 3, 3),
        "follow-up": ("apply_mask leaf_eigen leaf_moments ransac ransac_prepare", 7, 3),
    },
    "09b octree, general route, fresh single cube": {
        "build": (
            "blocks finalize init_level0 level_children level_hist level_prepare level_scan level_scatter", 52, 14),
        "info": (3000, 1, 585, 73, 511, 3, 3),
        "follow-up": ("apply_mask leaf_chunks leaf_eigen leaf_moments ransac ransac_order ransac_prepare", 26, 4),
    },
    "09c octree, prefix partition": {
        "build": (
            "blocks finalize init_level0 level_children level_hist level_prepare level_scan level_scatter "
            "prefix_hist prefix_scatter", 47, 24),
        "info": (3000, 1, 1089, 136, 812, 4, 4),
        "follow-up": ("apply_mask leaf_chunks leaf_eigen leaf_moments ransac ransac_order ransac_prepare", 28, 4),
    },
    "10 octree, prefix partition steps aside": {
        "build": (
            "blocks finalize init_level0 level_children level_hist level_prepare level_scan level_scatter "
            "prefix_hist prefix_scatter", 76, 28),
        "info": (3000, 1, 1177, 147, 871, 5, 5),
        "follow-up": ("apply_mask leaf_chunks leaf_eigen leaf_moments ransac ransac_order ransac_prepare", 30, 4),
    },
    "11 grid, planar": {
        "build": (
            "blocks finalize init_level0 keygen level_children level_hist level_prepare level_scan level_scatter "
            "linkey node_lambda node_moments roots sort_hist sort_scan sort_scatter", 70, 35),
        "info": (4000, 27, 1803, 222, 1023, 3, 3),
        "follow-up": ("apply_mask leaf_chunks leaf_eigen leaf_moments ransac ransac_order ransac_prepare", 26, 6),
    },
}


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_build_route(name):
    setup, options = SCENARIOS[name]
    got = {}
    with _own_context(options) as ctx:
        forest, steps, _ = setup()
        try:
            for step, action in steps:
                got[step] = _measure(ctx, action)
            got["info"] = _info(forest)
            got["follow-up"] = _measure(ctx, lambda: _follow_up(forest))
        finally:
            forest.close()
    print(f"\nROUTE {name!r}: {got!r},")
    with _own_context(options):
        forest, steps, check = setup()
        try:
            for _, action in steps:
                action()
            assert _info(forest) == got["info"]
            check()
        finally:
            forest.close()
    assert got == EXPECTED[name]


# ---- 12. a point outside the cube of a node that splits: the block-table tail's roll-back, from both of its callers --
# (tests/test_gpu_parity.py::test_point_outside_cube_only_fails_when_its_node_splits pins the error itself for the
#  default route; neither the route, nor the state left behind, nor the general route's tail)
EXPECTED_OUTSIDE = {
    "behind the bucket build": {
        "build": (
            "blocks bucket_build bucket_nodes bucket_scan finalize level_children level_hist level_prepare "
            "level_rekey level_scan level_scatter part_hist part_scatter", 50, 6),
        "again": ("bucket_build bucket_nodes bucket_scan part_hist part_scatter", 9, 4),
        "info": (200, 1, 81, 10, 68, 3, 3),
    },
    "behind the general route": {
        "build": (
            "blocks finalize init_level0 level_children level_hist level_prepare level_scan level_scatter", 44, 6),
        "again": (
            "blocks finalize init_level0 keygen level_children level_hist level_prepare level_scan level_scatter "
            "linkey roots sort_hist sort_scan sort_scatter", 51, 15),
        "info": (200, 1, 81, 10, 68, 3, 3),
    },
}


@pytest.mark.parametrize("tail", ["behind the bucket build", "behind the general route"])
def test_point_outside_the_cube_of_a_split_node_rolls_back(tail):
    from octreelib_amd import _native as nat
    from octreelib_amd.octree import Octree, OctreeConfig
    from oracle import octree_np as onp

    cloud = np.vstack([np.random.default_rng(12).random((200, 3)), [[1.5, 0.2, 0.2]]])
    mask = np.arange(len(cloud)) < 200
    options = {} if tail == "behind the bucket build" else {"NO_BUCKET_BUILD": 1}
    got = {}
    with _own_context(options) as ctx:
        oc = Octree(OctreeConfig(), np.zeros(3), np.float64(1))
        try:
            oc.insert_points(cloud)
            got["build"] = _measure(ctx, lambda: oc.subdivide(crit(8)), raises=(nat.DomainError, OUTSIDE))
            assert (oc.n_points, oc.n_leaves, oc.n_nodes) == (201, 1, 1)      # the points are there, no scheme
            oc.apply_mask(mask)                                               # the data corrected ...
            got["again"] = _measure(ctx, lambda: oc.subdivide(crit(8)))       # ... the same request completes
            got["info"] = _info(oc._forest)
            ot = onp.OTree(np.zeros(3), np.float64(1))
            ot.insert_points(cloud)
            ot.apply_mask(mask)
            ot.subdivide(8)
            _check_tree(oc.get_leaf_points(), [oc.n_nodes, oc.n_leaves, oc.n_points], ot)
        finally:
            oc._forest.close()
    print(f"\nROUTE {tail!r}: {got!r},")
    assert got == EXPECTED_OUTSIDE[tail]
