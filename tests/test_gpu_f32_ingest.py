"""float32 clouds on the device path (octl_forest_*_f32, k_ingest_f32).

The contract: inserting an f32 array P leaves exactly what inserting P.astype(np.float64) leaves - node tables,
voxel keys, block table, permutation, get_points bytes, counters, RANSAC masks and planes, exception types and
messages.  Every test here runs both arms and compares them bit for bit."""

import ctypes as C

import numpy as np
import pytest

from tests._util import assert_same_leaves, canon_from_list

pytestmark = pytest.mark.gpu


# ---- helpers ---------------------------------------------------------------------------------------------------
def _tables(f):
    """Every host-visible table of a forest (test_gpu_parity.py compares the same set)."""
    return ({k: v.copy() for k, v in f.nodes.items()}, {k: v.copy() for k, v in f.blocks.items()}, f.perm.copy(),
            f.voxels.copy(), f.order.copy(), f.xyz.copy())


def _assert_same_tables(a, b):
    for x, y in zip(a[:2], b[:2]):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(x[k], y[k]), k
    for x, y in zip(a[2:5], b[2:5]):
        assert np.array_equal(x, y)
    assert a[5].tobytes() == b[5].tobytes()   # leaf-ordered coordinates, bit for bit (-0.0, subnormals)


def _f64(c):
    return np.asarray(c).astype(np.float64)


def _outcome(fn):
    try:
        return ("ok", fn())
    except Exception as e:  # noqa: BLE001 - the exception itself is what is compared
        return (type(e), str(e))


def _boundary_cloud(L, n_cells, seed, corner=0.0, subnormals=True, magnitude=0.0):
    """f32 points on and next to voxel and child boundaries: integers, halves, quarters, eighths of the voxel edge and
    their f32 nextafter neighbours on both sides, -0.0, f32 subnormals; no two points equal."""
    rng = np.random.default_rng(seed)
    base = []
    for k in range(n_cells):
        for o in (0.0, 0.5, 0.25, 0.75, 0.125, 0.375):
            v = np.float32(magnitude + corner + (k + o) * L)
            base += [v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))]
    base = np.array(base, dtype=np.float32)
    if corner == 0.0 and magnitude == 0.0:
        tiny = np.array([-0.0, 1e-45, 1e-42, 1.17e-38, 3e-39], dtype=np.float32)
        base = np.concatenate([base[base >= 0], tiny if subnormals else tiny[:1]])
    if not subnormals:
        base = base[(base == 0) | (np.abs(base) >= np.finfo(np.float32).tiny)]
    base = base[(base >= np.float32(magnitude + corner)) & (base < np.float32(magnitude + corner + n_cells * L))]
    pts = rng.choice(base, size=(6000, 3))
    _, first = np.unique(pts + np.float32(0.0), axis=0, return_index=True)   # (-0.0 and 0.0 are one point)
    pts = pts[np.sort(first)]
    # at most 8 points per cell of 2^-40 voxel edges (the subnormals next to 0 would otherwise need a split deeper
    # than the 63 levels the library allows): a count threshold of 8 or more splits no deeper than 40 levels
    q = np.floor((pts.astype(np.float64) - (magnitude + corner)) / L * 2.0 ** 40)
    _, inv = np.unique(q, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    rank = np.zeros(len(pts), dtype=np.int64)
    seen = {}
    for i, g in enumerate(inv.tolist()):
        rank[i] = seen.get(g, 0)
        seen[g] = rank[i] + 1
    pts = pts[rank < 8]
    rng.shuffle(pts)
    return np.ascontiguousarray(pts, dtype=np.float32)


def _grid_run(clouds, L, K, table, convert):
    """Grid: insert every pose, subdivide, RANSAC of every block with details, then map_leaf_points_cuda_ransac; the
    state after each phase."""
    from octreelib_amd import MaxPoints
    from octreelib_amd.grid import Grid, GridConfig

    g = Grid(GridConfig(voxel_edge_length=L))
    try:
        for p, c in enumerate(clouds):
            g.insert_points(p, convert(c))
        g.subdivide([MaxPoints(K)])
        out = [_tables(g._forest)]
        out.append([g.get_points(p).tobytes() for p in range(len(clouds))])
        out.append([(g.n_nodes(p), g.n_leaves(p), g.n_points(p)) for p in range(len(clouds))])
        nb = len(g._forest.blocks["node"])
        plane, count, index = g._forest.ransac_blocks(np.arange(nb, dtype=np.int32), table, 0.01, details=True)
        out.append((plane.tobytes(), count.tobytes(), index.tobytes(), g._forest.device_mask().tobytes()))
        g.map_leaf_points_cuda_ransac(hypotheses=table)
        out.append(_tables(g._forest))
        out.append([g.get_points(p).tobytes() for p in range(len(clouds))])
        out.append([(g.n_nodes(p), g.n_leaves(p), g.n_points(p)) for p in range(len(clouds))])
        return out
    finally:
        if g._forest is not None:
            g._forest.close()


def _assert_same_runs(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, tuple) and len(x) == 6 and isinstance(x[0], dict):
            _assert_same_tables(x, y)
        else:
            assert x == y


def _table(seed=4, H=256):
    rng = np.random.default_rng(seed)
    return rng.random((H, 6))


# ---- 1. values -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 5])
def test_grid_boundary_values_match_the_f64_twin(L):
    # (subnormals: test_subnormals_and_negative_zero_come_through - a subdivide of a cluster of them next to 0 stops
    #  at the library's depth guard in the f64 path as well)
    a = _boundary_cloud(L, 4, seed=L, subnormals=False)
    b = _boundary_cloud(L, 3, seed=L + 10, subnormals=False)
    table = _table()
    want = _grid_run([a, b], L, 8, table, _f64)
    got = _grid_run([a, b], L, 8, table, lambda c: c)
    _assert_same_runs(got, want)
    assert np.frombuffer(got[1][0], dtype=np.float64).size == 3 * len(a)


def test_subnormals_and_negative_zero_come_through():
    from octreelib_amd.grid import Grid, GridConfig

    pts = np.array([[1e-45, 0.5, 0.5], [-0.0, 1e-42, 0.25], [3e-39, -0.0, 1e-40]], dtype=np.float32)
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, pts)
    got = g._forest.xyz
    want = pts.astype(np.float64)
    tiny = np.abs(want) < np.finfo(np.float32).tiny
    assert ((want != 0) & tiny).sum() == 4   # (the four f32 subnormals are not zero in f64)
    order = g._forest.perm
    assert got.tobytes() == want[order].tobytes()
    g._forest.close()


def test_utm_magnitudes_match_the_f64_twin():
    # ~5e6 m northing, ~4e5 m easting: f32 keeps 0.5 m / 0.03 m there; L = 5 and L = 1
    for L in (5, 1):
        a = _boundary_cloud(L, 4, seed=3, magnitude=5.0e6)
        a[:, 0] -= np.float32(4.6e6)     # (easting ~4e5; still f32 values)
        table = _table(seed=8)
        _assert_same_runs(_grid_run([a], L, 6, table, lambda c: c), _grid_run([a], L, 6, table, _f64))


def test_grid_small_scene_against_the_oracle():
    from octreelib_amd import MaxPoints
    from octreelib_amd.grid import Grid, GridConfig
    from oracle import octree_np as onp

    pts = _boundary_cloud(1, 3, seed=21, subnormals=False)
    grid = Grid(GridConfig(voxel_edge_length=1))
    grid.insert_points(0, pts)
    grid.subdivide([MaxPoints(8)])
    og = onp.OGrid(1)
    p64 = pts.astype(np.float64)
    og.insert_points(0, p64)
    og.subdivide(8)
    index = {p.tobytes(): i for i, p in enumerate(p64)}
    got = canon_from_list([(v.corner_min, v.edge_length, [index[p.tobytes()] for p in v.get_points()])
                           for v in grid.get_leaf_points(0)])
    want = canon_from_list(og.leaf_table(0))
    assert_same_leaves(got, want, ordered=False)
    assert grid.n_points(0) == og.n_points(0) and grid.n_nodes(0) == og.n_nodes(0)
    grid._forest.close()


def _cube_runs(kind, clouds, convert, corner=(-4.0, -4.0, -4.0), edge=8.0, K=8):
    from octreelib_amd import MaxPoints
    from octreelib_amd.octree import Octree, OctreeConfig
    from octreelib_amd.octree_manager import OctreeManager

    if kind == "octree":
        t = Octree(OctreeConfig(), np.array(corner), edge)
        for c in clouds:
            t.insert_points(convert(c))
        t.subdivide([MaxPoints(K)])
        out = [_tables(t._forest), t.get_points().tobytes(), (t.n_nodes, t.n_leaves, t.n_points),
               [(v.corner_min.tobytes(), np.float64(v.edge_length).tobytes(), v.get_points().tobytes())
                for v in t.get_leaf_points()]]
        t._forest.close()
        return out
    m = OctreeManager(Octree, OctreeConfig(), np.array(corner), edge)
    for p, c in enumerate(clouds):
        m.insert_points(p % 2, convert(c))   # (poses 0, 1, then extends of both)
    m.subdivide([MaxPoints(K)])
    out = [_tables(m._forest)]
    for p in range(min(2, len(clouds))):
        out += [m.get_points(p).tobytes(), (m.n_nodes(p), m.n_leaves(p), m.n_points(p)),
                [(v.corner_min.tobytes(), np.float64(v.edge_length).tobytes(), v.get_points().tobytes())
                 for v in m.get_leaf_points(pose_number=p)]]
    m._forest.close()
    return out


@pytest.mark.parametrize("kind", ["octree", "manager"])
def test_cube_with_negative_corner_matches_the_f64_twin(kind):
    clouds = [_boundary_cloud(1, 8, seed=s, corner=-4.0, subnormals=False) for s in (31, 32, 33)]
    _assert_same_runs(_cube_runs(kind, clouds, lambda c: c), _cube_runs(kind, clouds, _f64))


# ---- 2. layouts ------------------------------------------------------------------------------------------------
def _layout_cloud(n, seed):
    from octreelib_amd import synthetic

    return synthetic.planar_cloud(n + 1, (6, 6, 6), seed=seed).astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 4097, 1_000_003])
def test_layouts_behind_an_odd_pose_and_unaligned_views(n):
    """The target already holds 3 points (odd: the new pose lands 8 bytes off 16-byte alignment), then f32 poses from
    a view that starts at row 1 (4-byte aligned host source), a strided view, an f32 DeviceCloud and an f32 device
    pointer 12 bytes into its buffer (unaligned device source).  Against the same poses in f64."""
    import octreelib_amd as oa
    from octreelib_amd._engine import Forest

    big = _layout_cloud(2 * n + 2, seed=n % 7 + 1)
    odd = np.array([[0.5, 0.5, 0.5], [1.5, 2.5, 3.5], [4.25, 0.75, 5.5]])
    row1 = big[1:n + 1]
    strided = big[::2][:n]
    dev = big[n:2 * n + 1]           # n + 1 rows: the device pointer skips the first

    def run(f32):
        f = Forest(0, np.zeros(3), 1.0)
        f.add_pose(odd)
        f.add_pose(row1 if f32 else _f64(row1))
        f.add_pose(strided if f32 else _f64(strided))
        cloud = oa.upload_async(dev if f32 else _f64(dev))
        f.add_pose(cloud)
        # an unaligned device source: 12 bytes (one f32 point) into the buffer
        slot = C.c_int32(-1)
        if f32:
            fn, off = f.lib.octl_forest_add_pose_device_f32, 12
        else:
            fn, off = f.lib.octl_forest_add_pose_device, 24
        f.ctx.check(fn(f.handle, C.c_void_p(cloud.ptr.value + off), n, C.byref(slot)))
        f._register_slot(n)
        f.subdivide(32)
        t = _tables(f)
        f.close()
        cloud.release()
        return t

    _assert_same_tables(run(True), run(False))


def test_mixed_poses_extends_and_a_late_pose_through_the_incremental_path():
    import octreelib_amd as oa
    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd.grid import Grid, GridConfig
    from octreelib_amd.octree import Octree, OctreeConfig
    from octreelib_amd.octree_manager import OctreeManager

    c = [synthetic.planar_cloud(20_001 + 1000 * j, (5, 5, 5), seed=2, stream=j).astype(np.float32) for j in range(5)]
    table = _table(seed=11)

    def grid_arm(f32):
        g = Grid(GridConfig(voxel_edge_length=1))
        g.insert_points(0, _f64(c[0]))                               # f64 host
        g.insert_points(1, c[1] if f32 else _f64(c[1]))              # f32 host
        g.insert_points(2, oa.upload_async(c[2] if f32 else _f64(c[2])))   # f32 DeviceCloud
        g.subdivide([MaxPoints(48)])
        first = _tables(g._forest)
        g.insert_points(3, c[3] if f32 else _f64(c[3]))              # a late pose: the incremental path
        g.subdivide([MaxPoints(48)])
        g.map_leaf_points_cuda_ransac(hypotheses=table)
        out = [first, _tables(g._forest), [g.get_points(p).tobytes() for p in range(4)]]
        g._forest.close()
        return out

    def manager_arm(f32):
        m = OctreeManager(Octree, OctreeConfig(), np.zeros(3), 8.0)
        m.insert_points(0, c[0] if f32 else _f64(c[0]))
        m.insert_points(1, _f64(c[1]))
        m.insert_points(0, oa.upload_async(c[2] if f32 else _f64(c[2])))   # extend, device source
        m.insert_points(1, c[3] if f32 else _f64(c[3]))                    # extend, host source
        m.subdivide([MaxPoints(40)])
        m.insert_points(0, c[4][1:] if f32 else _f64(c[4][1:]))            # extend after a subdivide
        m.subdivide([MaxPoints(40)])
        out = [_tables(m._forest), [m.get_points(p).tobytes() for p in range(2)]]
        m._forest.close()
        return out

    def octree_arm(f32):
        t = Octree(OctreeConfig(), np.zeros(3), 8.0)
        for j in range(4):
            src = c[j][::3] if j == 1 else c[j]
            t.insert_points((oa.upload_async(src) if j == 2 else src) if f32 else _f64(src))
            if j == 1:
                t.subdivide([MaxPoints(40)])
        t.subdivide([MaxPoints(40)])
        out = [_tables(t._forest), t.get_points().tobytes()]
        t._forest.close()
        return out

    for arm in (grid_arm, manager_arm, octree_arm):
        a, b = arm(True), arm(False)
        _assert_same_tables(a[0], b[0])
        if arm is grid_arm:
            _assert_same_tables(a[1], b[1])
        assert a[-1] == b[-1]


# ---- 3. errors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["nan", "inf", "-inf", "window"])
def test_domain_errors_are_those_of_the_f64_path(bad):
    from octreelib_amd import MaxPoints
    from octreelib_amd.grid import Grid, GridConfig
    from octreelib_amd.octree import Octree, OctreeConfig

    pts = _layout_cloud(500, seed=3)
    pts[217, 1] = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf, "window": np.float32(3.0e9)}[bad]

    def grid_arm(cloud):
        def go():
            g = Grid(GridConfig(voxel_edge_length=1))
            try:
                g.insert_points(0, cloud)
                g.subdivide([MaxPoints(16)])
                return g.n_points(0)
            finally:
                g._forest.close()
        return _outcome(go)

    def tree_arm(cloud):
        def go():
            t = Octree(OctreeConfig(), np.zeros(3), 8.0)
            try:
                t.insert_points(cloud)
                t.subdivide([MaxPoints(16)])
                return t.n_points()
            finally:
                t._forest.close()
        return _outcome(go)

    for arm in (grid_arm, tree_arm):
        want = arm(_f64(pts))
        assert want[0] != "ok"   # (the f64 path raises here)
        assert arm(pts) == want


# ---- 4. it is really the f32 path ------------------------------------------------------------------------------
def test_the_f32_path_is_taken():
    import octreelib_amd as oa
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig

    pts = _layout_cloud(10_000, seed=5)
    ctx = nat.get_context()
    ctx.set_profiling(True)
    try:
        ctx.timings()   # (drop whatever was recorded before)
        g = Grid(GridConfig(voxel_edge_length=1))
        g.insert_points(0, pts)
        g.insert_points(1, _f64(pts) + 0.5)
        g._forest.ensure_built()
        t = ctx.timings()
        assert t["ingest_f32"][1] == 1 and t["ingest"][1] >= 1
        g._forest.close()
    finally:
        ctx.set_profiling(False)

    cloud = oa.upload_async(pts)
    assert cloud.dtype == np.float32 and cloud.nbytes == 12 * len(pts) and len(cloud) == len(pts)
    c64 = oa.upload_async(_f64(pts))
    assert c64.dtype == np.float64 and c64.nbytes == 24 * len(pts)
    # an f32 DeviceCloud is copied (widened) even as the first pose: it may go after the next synchronising call
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, cloud)
    assert not g._forest.reads_in_place(cloud)
    nat.get_context().sync()
    cloud.release()
    g2 = Grid(GridConfig(voxel_edge_length=1))
    g2.insert_points(0, c64)
    from octreelib_amd import MaxPoints

    for grid in (g, g2):
        grid.subdivide([MaxPoints(32)])
    assert g.get_points(0).tobytes() == g2.get_points(0).tobytes()
    assert (g.n_nodes(0), g.n_leaves(0), g.n_points(0)) == (g2.n_nodes(0), g2.n_leaves(0), g2.n_points(0))
    g._forest.close()
    g2._forest.close()
    c64.release()


# ---- 5. pipelines ----------------------------------------------------------------------------------------------
def test_upload_async_and_scan_pipeline_over_f32_rings():
    import octreelib_amd as oa
    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd.grid import Grid, GridConfig

    clouds = [synthetic.planar_cloud(200_000 - 17_000 * j, (8, 8, 8), seed=1, stream=j).astype(np.float32)
              for j in range(3)]
    table = _table(seed=6, H=512)

    def fit(grid, i):
        grid.subdivide([MaxPoints(64)])
        grid.map_leaf_points_cuda_ransac(hypotheses=table)
        return grid.n_points(0), grid.n_leaves(0), grid.get_points(0).tobytes()

    def ring_loop(dtype):
        ring = [oa.pinned_empty((200_000, 3), dtype) for _ in range(2)]
        out = []
        ring[0][: len(clouds[0])] = clouds[0]
        nxt = oa.upload_async(ring[0][: len(clouds[0])])
        for i in range(6):
            cur = nxt
            if i + 1 < 6:
                c = clouds[(i + 1) % 3]
                cur.wait()                     # (the other ring buffer's previous upload is done: refill it)
                ring[(i + 1) % 2][: len(c)] = c
                nxt = oa.upload_async(ring[(i + 1) % 2][: len(c)])
            g = Grid(GridConfig(voxel_edge_length=1))
            g.insert_points(0, cur)
            out.append(fit(g, i))
            g._forest.close()
            cur.release()
        return out

    want = ring_loop(np.float64)
    got = ring_loop(np.float32)
    assert got == want

    def pipeline(dtype):
        ring = [oa.pinned_empty((200_000, 3), dtype) for _ in range(5)]

        def scans():
            for i in range(9):
                c = clouds[i % 3]
                ring[i % 5][: len(c)] = c
                yield ring[i % 5][: len(c)]

        with oa.ScanPipeline(2) as pipe:
            return list(pipe.map(scans(), fit))

    assert pipeline(np.float32) == pipeline(np.float64) == [want[i % 3] for i in range(9)]


# ---- 6. full size ----------------------------------------------------------------------------------------------
def test_full_size_planar_scan_is_identical_to_its_f64_twin():
    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd.grid import Grid, GridConfig

    pts = synthetic.planar_cloud(10_000_000, (32, 32, 32), seed=1).astype(np.float32)
    np.random.seed(0)
    table = np.random.random((1024, 6))

    def run(cloud):
        g = Grid(GridConfig(voxel_edge_length=1))
        g.insert_points(0, cloud)
        g.subdivide([MaxPoints(64)])
        before = _tables(g._forest)
        g.map_leaf_points_cuda_ransac(hypotheses=table)
        after = _tables(g._forest)
        counts = (g.n_nodes(0), g.n_leaves(0), g.n_points(0))
        g._forest.close()
        return before, after, counts

    a = run(pts)
    b = run(_f64(pts))
    _assert_same_tables(a[0], b[0])
    _assert_same_tables(a[1], b[1])
    assert a[2] == b[2] and a[2][2] < 10_000_000
