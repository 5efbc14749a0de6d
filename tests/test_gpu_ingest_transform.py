"""Clouds inserted under a transform on the device (octl_forest_add_pose_xf / _extend_pose_xf, k_ingest_xf).

The contract: inserting P under (transforms, segment) leaves exactly what inserting transform_rows_np(transforms, P,
segment) leaves - store bytes, node tables, voxel keys, block table, permutation, get_points bytes, counters, RANSAC
masks and planes, later query answers, exception types and messages.  Every test here runs both arms - the device
transform and the host-transformed twin - and compares them bit for bit (the shape of tests/test_gpu_f32_ingest.py)."""

import ctypes as C

import numpy as np
import pytest

from octreelib_amd.registration import se3_exp, transform_rows_np
from tests.test_gpu_f32_ingest import _assert_same_runs, _assert_same_tables, _boundary_cloud, _outcome, _table, _tables

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 3, 4, 5, 7, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 20_006]
UTM = np.array([5.0e6, 4.0e5, 100.0])
XF_F32, XF_DEVICE = 1, 2


# ---- helpers ---------------------------------------------------------------------------------------------------
def _counter(name):
    from octreelib_amd import _native as nat

    c = C.c_uint64(0)
    nat.get_context().check(getattr(nat.load(), name)(C.byref(c)))
    return c.value


def _rigid(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return se3_exp(np.concatenate([rng.normal(size=3) * 0.7, rng.normal(size=3) * scale]))


def _translation(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def _quarter_turn(shift):
    """x' = -y + shift, y' = x, z' = z: exact in f64, boundaries land on boundaries."""
    T = np.eye(4)
    T[:2, :2] = [[0.0, -1.0], [1.0, 0.0]]
    T[0, 3] = shift
    return T


def _table12(T):
    return np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(-1, 4, 4)[:, :3, :].reshape(-1, 12))


class _Arm:
    """How one arm hands a cloud over: "twin" transforms on the host and inserts the result, the others insert the
    cloud itself under the transform - as a host array of its own dtype, as f64 / f32 host array, or as DeviceCloud."""

    def __init__(self, kind):
        self.kind = kind
        self.clouds = []

    def __call__(self, insert, cloud, transform=None, segment=None):
        import octreelib_amd as oa

        if transform is None:
            return insert(cloud)
        if self.kind == "twin":
            return insert(transform_rows_np(transform, cloud, segment))
        if self.kind == "f64":
            cloud = np.asarray(cloud).astype(np.float64)
        elif self.kind == "f32":
            assert cloud.dtype == np.float32
        elif self.kind == "device":
            cloud = oa.upload_async(cloud)
            self.clouds.append(cloud)
        return insert(cloud, transform=transform, segment=segment)

    def release(self):
        from octreelib_amd import _native as nat

        if self.clouds:
            nat.get_context().sync()
        for c in self.clouds:
            c.release()
        self.clouds = []


def _same(a, b):
    """Two outcomes (_outcome of a function that returns a list of runs): the same error, or the same runs."""
    assert a[0] == b[0], (a[0], b[0])
    if a[0] == "ok":
        _assert_same_runs(a[1], b[1])
    else:
        assert a == b


# ---- 1. sizes and layouts --------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_size_first_and_behind_an_odd_store(dtype, source):
    """Each size as the first pose of an empty grid and behind poses of 1 and 3 rows (the new rows then start 8 bytes
    off a 16-byte boundary): store, permutation, tables and get_points against the twin."""
    from octreelib_amd import MaxPoints
    from octreelib_amd.grid import Grid, GridConfig

    rng = np.random.default_rng(1)
    big = (rng.random((max(SIZES), 3)) * 6.0 - 1.0).astype(dtype)
    big[1] = [-0.0, 0.0, -0.0]
    front3 = np.array([[0.5, 0.5, 0.5], [1.5, 2.5, 3.5], [4.25, 0.75, 5.5]])
    T = _rigid(2)

    def run(arm, n, front):
        g = Grid(GridConfig(voxel_edge_length=1))
        try:
            p = 0
            if front is not None:
                g.insert_points(p, front)
                p += 1
            arm(lambda c, **kw: g.insert_points(p, c, **kw), big[:n], T)
            g.subdivide([MaxPoints(32)])
            return [_tables(g._forest), [g.get_points(q).tobytes() for q in range(p + 1)],
                    [(g.n_nodes(q), g.n_leaves(q), g.n_points(q)) for q in range(p + 1)]]
        finally:
            g._forest.close()
            arm.release()

    kind = "device" if source == "device" else ("f32" if dtype == np.float32 else "f64")
    for n in SIZES:
        for front in (None, front3[:1], front3):
            if n == 0 and front is None:
                continue     # (an empty grid: nothing to compare; n = 0 behind a pose stays)
            want = _outcome(lambda: run(_Arm("twin"), n, front))
            got = _outcome(lambda: run(_Arm(kind), n, front))
            assert want[0] == "ok", (n, want)
            _same(got, want)
            assert len(np.frombuffer(got[1][1][-1], dtype=np.float64)) == 3 * n


def test_an_empty_cloud_still_creates_the_pose():
    from octreelib_amd._engine import Forest

    f = Forest(0, np.zeros(3), 1.0)
    a = _counter("octl_debug_launches")
    f.add_pose(np.empty((0, 3)))                          # (the forest's first append resets its voxel box: one launch)
    plain = _counter("octl_debug_launches") - a
    f.close()
    f = Forest(0, np.zeros(3), 1.0)
    a = _counter("octl_debug_launches")
    s0 = f.add_pose(np.empty((0, 3)), _rigid(1))
    assert _counter("octl_debug_launches") - a == plain   # (what an empty pose costs without a transform)
    a = _counter("octl_debug_launches")
    s1 = f.add_pose(np.empty((0, 3), dtype=np.float32), np.stack([_rigid(1)] * 2), np.empty(0, dtype=np.int64))
    f.extend_pose(0, np.empty((0, 3)), _rigid(1))
    assert _counter("octl_debug_launches") == a           # (n = 0 launches nothing)
    assert (s0, s1, f.n_slots) == (0, 1, 2)
    f.add_pose(np.array([[0.5, 0.5, 0.5]]))
    f.subdivide(8)
    assert f.xyz.tobytes() == np.array([[0.5, 0.5, 0.5]]).tobytes()
    f.close()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_device_pointers_one_row_into_their_buffer(f32):
    """Through the C ABI: a device source that starts one row into its buffer is 8-byte (f64) / 4-byte (f32) aligned
    only; behind an even and an odd store; rigid and piecewise."""
    import octreelib_amd as oa
    from octreelib_amd import _native as nat
    from octreelib_amd._engine import Forest

    rng = np.random.default_rng(3)
    dtype = np.float32 if f32 else np.float64
    Ts = np.stack([_rigid(s) for s in (4, 5, 6)])
    flags = XF_DEVICE | (XF_F32 if f32 else 0)
    row = 12 if f32 else 24
    for n in (1, 2, 3, 5, 257, 4097):
        big = (rng.random((n + 1, 3)) * 5.0).astype(dtype)
        seg = np.ascontiguousarray(rng.integers(0, 3, n), dtype=np.uint16)
        for odd in (False, True):
            cloud = oa.upload_async(big)
            got = Forest(0, np.zeros(3), 1.0)
            want = Forest(0, np.zeros(3), 1.0)
            try:
                for f in (got, want):
                    f.add_pose(np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.75]])[:1 if odd else 2])
                src = C.c_void_p(cloud.ptr.value + row)
                assert src.value % 16 == (12 if f32 else 8)
                slot = C.c_int32(-1)
                t1, t3 = _table12(Ts[0]), _table12(Ts)
                got.ctx.check(got.lib.octl_forest_add_pose_xf(got.handle, src, n, flags, nat.ptr(t1), 1, None,
                                                              C.byref(slot)))
                got._register_slot(n)
                got.ctx.check(got.lib.octl_forest_add_pose_xf(got.handle, src, n, flags, nat.ptr(t3), 3, nat.ptr(seg),
                                                              C.byref(slot)))
                got._register_slot(n)
                got.ctx.check(got.lib.octl_forest_extend_pose_xf(got.handle, 1, src, n, flags, nat.ptr(t3), 3,
                                                                 nat.ptr(seg)))
                got.slot_sizes[1] += n
                want.add_pose(transform_rows_np(Ts[0], big[1:]))
                want.add_pose(transform_rows_np(Ts, big[1:], seg))
                want.extend_pose(1, transform_rows_np(Ts, big[1:], seg))
                got.subdivide(16)
                want.subdivide(16)
                _assert_same_tables(_tables(got), _tables(want))
            finally:
                got.close()
                want.close()
                cloud.release()


# ---- 2. twin runs ----------------------------------------------------------------------------------------------
def _grid_run(arm, clouds, transforms, L, K, table):
    """Grid: every pose inserted under its transform, subdivide, RANSAC of every block with details, then
    map_leaf_points_cuda_ransac; the state after each phase (tests/test_gpu_f32_ingest.py: _grid_run)."""
    from octreelib_amd import MaxPoints
    from octreelib_amd.grid import Grid, GridConfig

    g = Grid(GridConfig(voxel_edge_length=L))
    try:
        for p, (c, T) in enumerate(zip(clouds, transforms)):
            arm(lambda x, **kw: g.insert_points(p, x, **kw), c, T)
        out = [_tables(g._forest)]                       # (after insert: the top-level voxels)
        g.subdivide([MaxPoints(K)])
        out.append(_tables(g._forest))
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
        arm.release()


def _grid_transforms(name, L):
    if name == "identity":
        return [np.eye(4), np.eye(4)[:3], np.eye(4)]
    if name == "rigid":
        return [_rigid(11, 2.0), _rigid(12, 2.0)[:3], _rigid(13, 2.0)]
    if name == "utm":
        return [_translation(UTM), _translation(UTM + [L, 0, 0]), _translation(UTM - [0, L, 0])]
    return [_quarter_turn(4.0 * L), _quarter_turn(3.0 * L), _quarter_turn(8.0 * L)]


@pytest.mark.parametrize("name", ["identity", "rigid", "utm", "quarter_turn"])
@pytest.mark.parametrize("L", [1, 5])
def test_grid_of_three_poses_matches_the_twin(L, name):
    clouds = [_boundary_cloud(L, 4, seed=L + 20, subnormals=False), _boundary_cloud(L, 3, seed=L + 21, subnormals=False),
              _boundary_cloud(L, 4, seed=L + 22, subnormals=False)[:1500]]
    Ts = _grid_transforms(name, L)
    table = _table(seed=5)
    want = _grid_run(_Arm("twin"), clouds, Ts, L, 8, table)
    assert np.frombuffer(want[2][0], dtype=np.float64).size == 3 * len(clouds[0])
    if name == "identity":     # (the sign of -0.0 is lost on both sides)
        assert np.signbit(clouds[0]).any() and not np.signbit(np.frombuffer(want[2][0], dtype=np.float64)).any()
    for kind in ("f32", "f64", "device"):
        _assert_same_runs(_grid_run(_Arm(kind), clouds, Ts, L, 8, table), want)


def _cube_cloud(seed, n=2500):
    """f32 points inside the cube [0.1, 3.4)^3 away from its faces, a third of the coordinates on the splitting planes
    of the first three levels."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.35, 3.15, (n, 3))
    planes = 0.1 + 3.3 * np.arange(1, 8) / 8.0
    snap = rng.random((n, 3)) < 0.33
    p[snap] = rng.choice(planes, int(snap.sum()))
    p = np.unique(p.astype(np.float32), axis=0)
    rng.shuffle(p)
    return np.ascontiguousarray(p)


def _cube_transforms(name):
    c = np.full(3, 0.1 + 3.3 / 2)
    if name == "identity":
        return np.zeros(3), [np.eye(4)] * 3
    if name == "rigid":      # small rotations about the cube's centre: the cloud stays inside
        rng = np.random.default_rng(17)
        return np.zeros(3), [se3_exp(np.concatenate([rng.normal(size=3) * 0.05, rng.normal(size=3) * 0.05]), c)
                             for _ in range(3)]
    if name == "utm":
        return UTM, [_translation(UTM)] * 3
    return np.zeros(3), [_quarter_turn(3.5)] * 3


def _cube_run(kind, arm, clouds, transforms, corner, K=8):
    from octreelib_amd import MaxPoints
    from octreelib_amd.octree import Octree, OctreeConfig
    from octreelib_amd.octree_manager import OctreeManager

    try:
        if kind == "octree":
            t = Octree(OctreeConfig(), corner, 3.3)
            try:
                for c, T in zip(clouds, transforms):
                    arm(lambda x, **kw: t.insert_points(x, **kw), c, T)
                t.subdivide([MaxPoints(K)])
                return [_tables(t._forest), t.get_points().tobytes(), (t.n_nodes, t.n_leaves, t.n_points),
                        [(v.corner_min.tobytes(), np.float64(v.edge_length).tobytes(), v.get_points().tobytes())
                         for v in t.get_leaf_points()]]
            finally:
                t._forest.close()
        m = OctreeManager(Octree, OctreeConfig(), corner, 3.3)
        try:
            for p, (c, T) in enumerate(zip(clouds, transforms)):
                arm(lambda x, **kw: m.insert_points(p % 2, x, **kw), c, T)     # (poses 0, 1, then an extend of 0)
            m.subdivide([MaxPoints(K)])
            out = [_tables(m._forest)]
            for p in range(2):
                out += [m.get_points(p).tobytes(), (m.n_nodes(p), m.n_leaves(p), m.n_points(p)),
                        [(v.corner_min.tobytes(), np.float64(v.edge_length).tobytes(), v.get_points().tobytes())
                         for v in m.get_leaf_points(pose_number=p)]]
            return out
        finally:
            m._forest.close()
    finally:
        arm.release()


@pytest.mark.parametrize("name", ["identity", "rigid", "utm", "quarter_turn"])
@pytest.mark.parametrize("kind", ["octree", "manager"])
def test_non_dyadic_cube_matches_the_twin(kind, name):
    clouds = [_cube_cloud(s) for s in (41, 42, 43)]
    shift, Ts = _cube_transforms(name)
    corner = shift + 0.1
    want = _cube_run(kind, _Arm("twin"), clouds, Ts, corner)
    for arm in ("f32", "f64", "device"):
        _assert_same_runs(_cube_run(kind, _Arm(arm), clouds, Ts, corner), want)


# ---- 3. extend: the store is rotated in front of the later poses ----------------------------------------------------
def test_extends_under_transforms_rotate_the_store():
    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd.octree import Octree, OctreeConfig
    from octreelib_amd.octree_manager import OctreeManager

    A, B, Cc = (synthetic.planar_cloud(n, (4, 4, 4), seed=6, stream=j) for j, n in enumerate((3001, 1234, 2000)))
    T0, T1 = _rigid(31, 0.3), _rigid(32, 0.3)
    seg = np.sort(np.random.default_rng(7).integers(0, 2, len(B)))

    def manager(arm):
        m = OctreeManager(Octree, OctreeConfig(), np.full(3, -8.0), 24.0)
        try:
            arm(lambda x, **kw: m.insert_points(0, x, **kw), A, T0)
            m.insert_points(1, Cc)
            arm(lambda x, **kw: m.insert_points(0, x, **kw), B.astype(np.float32), np.stack([T1, T0]), seg)
            m.subdivide([MaxPoints(40)])
            first = _tables(m._forest)
            arm(lambda x, **kw: m.insert_points(1, x, **kw), A[::3], T1)       # an extend after a subdivide
            m.subdivide([MaxPoints(40)])
            return [first, _tables(m._forest), [m.get_points(p).tobytes() for p in (0, 1)]]
        finally:
            m._forest.close()
            arm.release()

    def octree(arm):
        t = Octree(OctreeConfig(), np.full(3, -8.0), 24.0)
        try:
            arm(lambda x, **kw: t.insert_points(x, **kw), A, T0)
            arm(lambda x, **kw: t.insert_points(x, **kw), B, T1)
            t.subdivide([MaxPoints(40)])
            arm(lambda x, **kw: t.insert_points(x, **kw), Cc.astype(np.float32), T0)
            return [_tables(t._forest), t.get_points().tobytes()]
        finally:
            t._forest.close()
            arm.release()

    for fn in (manager, octree):
        want = fn(_Arm("twin"))
        for kind in ("host", "device"):
            _assert_same_runs(fn(_Arm(kind)), want)


# ---- 4. piecewise --------------------------------------------------------------------------------------------------
def _segments(pattern, m, n, rng):
    if pattern == "shuffled":
        return rng.integers(0, m, n)
    if pattern == "runs":      # sorted runs of 63, 64, 65 and 1 rows: run ends inside and on wave boundaries
        lengths = np.resize([63, 64, 65, 1], n)
        s = np.repeat(np.arange(len(lengths)), lengths)[:n]
        return np.minimum(s, m - 1) if m <= 3 else s % m
    if pattern == "equal":
        return np.full(n, m // 2)
    return np.full(n, m - 1)


@pytest.mark.parametrize("pattern", ["shuffled", "runs", "equal", "last"])
@pytest.mark.parametrize("m", [1, 2, 3, 64, 1024])
def test_piecewise_tables_and_segment_patterns(m, pattern):
    import octreelib_amd as oa
    from octreelib_amd._engine import Forest

    rng = np.random.default_rng(100 * m + len(pattern))
    n = 5003
    Ts = np.stack([_rigid(200 + j, 1.5) for j in range(min(m, 8))])
    Ts = Ts[np.arange(m) % len(Ts)].copy()
    Ts[:, :3, 3] += rng.normal(size=(m, 3)) * 0.01        # (no two table rows equal)
    seg = _segments(pattern, m, n, rng)
    for dtype in (np.float64, np.float32):
        P = (rng.random((n, 3)) * 6.0).astype(dtype)
        moved = transform_rows_np(Ts, P, seg)
        want = Forest(0, np.zeros(3), 1.0)
        got = Forest(0, np.zeros(3), 1.0)
        cloud = oa.upload_async(P[7:])
        try:
            want.add_pose(moved)
            want.add_pose(moved[:1001])
            want.add_pose(moved[7:])
            got.add_pose(P, Ts, seg)                                       # host, even store
            got.add_pose(P[:1001], Ts[:, :3, :], seg.astype(np.int32)[:1001])   # 3x4 stack, another index dtype
            slot = got.add_pose(cloud, Ts, seg[7:])                      # device, odd store (n + 1001 rows in front)
            assert slot == 2
            want.subdivide(24)
            got.subdivide(24)
            _assert_same_tables(_tables(got), _tables(want))
        finally:
            want.close()
            got.close()
            cloud.release()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_an_index_beyond_the_table_is_clamped(f32):
    """The Python layer refuses such an index; through the C ABI the kernel reads the table's last row instead."""
    from octreelib_amd import _native as nat
    from octreelib_amd._engine import Forest

    rng = np.random.default_rng(9)
    n, m = 3000, 5
    P = (rng.random((n, 3)) * 4.0).astype(np.float32 if f32 else np.float64)
    Ts = np.stack([_rigid(300 + j) for j in range(m)])
    raw = np.ascontiguousarray(rng.integers(0, m, n), dtype=np.uint16)
    raw[::5] = rng.integers(m, 65536, len(raw[::5]))
    raw[-1] = 65535
    got, want = Forest(0, np.zeros(3), 1.0), Forest(0, np.zeros(3), 1.0)
    try:
        slot = C.c_int32(-1)
        tab = _table12(Ts)
        got.ctx.check(got.lib.octl_forest_add_pose_xf(got.handle, nat.ptr(P), n, XF_F32 if f32 else 0, nat.ptr(tab), m,
                                                      nat.ptr(raw), C.byref(slot)))
        got._register_slot(n)
        want.add_pose(transform_rows_np(Ts, P, np.minimum(raw, m - 1)))
        got.subdivide(16)
        want.subdivide(16)
        _assert_same_tables(_tables(got), _tables(want))
        with pytest.raises(ValueError, match=r"segment entries must lie in \[0, 5\)"):
            got.add_pose(P, Ts, raw)
    finally:
        got.close()
        want.close()


def test_the_entries_refuse_bad_arguments():
    from octreelib_amd import _native as nat
    from octreelib_amd._engine import Forest

    f = Forest(0, np.zeros(3), 1.0)
    P = np.random.default_rng(1).random((10, 3))
    seg = np.zeros(10, dtype=np.uint16)
    one = _table12(np.eye(4))
    many = np.tile(one, (1025, 1))
    bad = one.copy()
    bad[0, 7] = np.nan
    slot = C.c_int32(-1)

    def add(n_pts, pts, tab, m, s, flags=0):
        return f.lib.octl_forest_add_pose_xf(f.handle, nat.ptr(pts), n_pts, flags, nat.ptr(tab), m, nat.ptr(s),
                                             C.byref(slot))

    try:
        assert add(10, P, one, 0, None) == nat.OCTL_E_INVALID
        assert add(10, P, many, 1025, seg) == nat.OCTL_E_INVALID
        assert add(10, P, many, 2, None) == nat.OCTL_E_INVALID
        assert add(10, None, one, 1, None) == nat.OCTL_E_INVALID
        assert add(10, P, None, 1, None) == nat.OCTL_E_INVALID
        assert add(10, P, bad, 1, None) == nat.OCTL_E_INVALID
        assert add(10, P, one, 1, None, flags=8) == nat.OCTL_E_INVALID
        assert f.lib.octl_forest_extend_pose_xf(f.handle, 0, nat.ptr(P), 10, 0, nat.ptr(one), 1, None) == nat.OCTL_E_INVALID
        assert f.n_slots == 0
        assert add(10, P, many, 1024, seg) == 0 and slot.value == 0
        assert f.lib.octl_forest_extend_pose_xf(f.handle, 0, nat.ptr(P), 10, 0, nat.ptr(bad), 1, None) == nat.OCTL_E_INVALID
    finally:
        f.close()


# ---- 5. the domain ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["window", "huge_entry", "nan_row", "outside_cube"])
def test_domain_outcomes_are_those_of_the_twin(case):
    """A point moved out of the domain raises at subdivide, as for the twin; insert_points itself does not."""
    from octreelib_amd import MaxPoints
    from octreelib_amd.grid import Grid, GridConfig
    from octreelib_amd.octree import Octree, OctreeConfig

    rng = np.random.default_rng(5)
    P = rng.random((500, 3)) * 3.0 + 0.25
    T = np.eye(4)
    if case == "window":
        T = _translation([0.0, 3.0e9, 0.0])          # beyond 2^30 voxels of edge 1
    elif case == "huge_entry":
        T[1, 2] = 1e300
        P[17] = [1e10, -1e10, 1e10]                  # (1e300 * 1e10 overflows: an infinity in the moved row)
    elif case == "nan_row":
        P[217, 1] = np.nan
        T = _rigid(3)
    else:
        T = _translation([0.0, 0.0, 5.0])            # out of the cube [0, 4)^3

    def grid_arm(arm):
        def go():
            g = Grid(GridConfig(voxel_edge_length=1))
            try:
                arm(lambda x, **kw: g.insert_points(0, x, **kw), P, T)
                inserted = True
                g.subdivide([MaxPoints(16)])
                return inserted, g.n_points(0), g.get_points(0).tobytes()
            finally:
                g._forest.close()
                arm.release()
        return _outcome(go)

    def tree_arm(arm):
        def go():
            t = Octree(OctreeConfig(), np.zeros(3), 4.0)
            try:
                arm(lambda x, **kw: t.insert_points(x, **kw), P, T)
                t.subdivide([MaxPoints(16)])
                return t.n_points, t.get_points().tobytes()
            finally:
                t._forest.close()
                arm.release()
        return _outcome(go)

    for fn in ((tree_arm,) if case == "outside_cube" else (grid_arm, tree_arm)):
        want = fn(_Arm("twin"))
        assert want[0] != "ok" and issubclass(want[0], Exception), want     # (the twin raises at subdivide)
        for kind in ("f64", "device"):
            assert fn(_Arm(kind)) == want
    # the insert itself does not raise
    g = Grid(GridConfig(voxel_edge_length=1))
    t = Octree(OctreeConfig(), np.zeros(3), 4.0)
    try:
        g.insert_points(0, P, transform=T)
        t.insert_points(P.astype(np.float32), transform=T)
    finally:
        g._forest.close()
        t._forest.close()


# ---- 6. launch shape -------------------------------------------------------------------------------------------------
def test_launches_and_host_waits_do_not_depend_on_n():
    """One kernel whatever n and whatever the store's parity; a host source costs the one wait that hands the buffer
    back, a device source none.  Measured on a context of its own, in stores that do not have to grow: a growing
    buffer waits for the stream, with or without a transform, and whether it grows depends on the blocks a context's
    pool happens to hold - a fresh context has none, nothing is handed back to it before the end, so every store is
    allocated with its 25 % of slack, which the pose in front of the measured one is large enough to make sufficient."""
    import octreelib_amd as oa
    from octreelib_amd import _native as nat
    from octreelib_amd._engine import Forest

    rng = np.random.default_rng(2)
    big = rng.random((20_006, 3)) * 5.0
    front = rng.random((120_001, 3)) * 5.0
    T = _rigid(8)
    Ts = np.stack([_rigid(9), _rigid(10)])
    ctx = nat.Context(nat.default_device())
    forests, clouds = [], []
    up = lambda p: oa.upload_async(p, ctx)
    forms = {
        "host": (lambda p: p, T, False), "host_f32": (lambda p: p.astype(np.float32), T, False),
        "device": (up, T, False), "device_f32": (lambda p: up(p.astype(np.float32)), T, False),
        "host_piecewise": (lambda p: p, Ts, True), "host_f32_piecewise": (lambda p: p.astype(np.float32), Ts, True),
        "device_piecewise": (up, Ts, True), "plain": (lambda p: p, None, False),
    }

    def forest(rows):
        f = Forest(0, np.zeros(3), 1.0, ctx=ctx)
        forests.append(f)
        f.add_pose(front[:rows])
        return f

    def one(f, make, transform, piecewise, n):
        src = make(big[:n])
        if isinstance(src, oa.DeviceCloud):
            clouds.append(src)
            src.wait()
        ctx.sync()
        a, b = _counter("octl_debug_launches"), _counter("octl_debug_host_syncs")
        f.add_pose(src, transform, (np.arange(n) % 2) if piecewise else None)
        got = (_counter("octl_debug_launches") - a, _counter("octl_debug_host_syncs") - b)
        ctx.sync()
        return got

    try:
        warm = forest(len(front))
        for make, transform, piecewise in forms.values():      # (the staging buffers reach their size here)
            one(warm, make, transform, piecewise, len(big))
        for odd in (0, 1):
            for name, (make, transform, piecewise) in forms.items():
                counts = [one(forest(len(front) - 1 + odd), make, transform, piecewise, n) for n in (100, 20_006)]
                assert counts[0] == counts[1], (name, odd, counts)
                if name == "plain":
                    # transform=None is store_append, untouched: the copy, then one launch - or two behind an odd
                    # store (the first row alone, then the aligned rest) - and the wait that hands the buffer back
                    assert counts[0] == (1 + odd, 1), (odd, counts)
                else:
                    assert counts[0] == (1, 0 if name.startswith("device") else 1), (name, odd, counts)
    finally:
        for f in forests:
            f.close()
        ctx.sync()
        for c in clouds:
            c.release()
        ctx.close()


def test_the_new_kernel_is_what_ran():
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig

    P = np.random.default_rng(4).random((10_000, 3)) * 4.0
    ctx = nat.get_context()
    ctx.set_profiling(True)
    try:
        ctx.timings()
        g = Grid(GridConfig(voxel_edge_length=1))
        g.insert_points(0, P, transform=_rigid(1))
        g.insert_points(1, P.astype(np.float32), transform=_rigid(2))
        g.insert_points(2, P)
        g._forest.ensure_built()
        t = ctx.timings()
        assert t["ingest_xf"][1] == 1 and t["ingest_xf_f32"][1] == 1 and t["ingest"][1] >= 1
        g._forest.close()
    finally:
        ctx.set_profiling(False)


# ---- 7. state ----------------------------------------------------------------------------------------------------------
def test_device_cloud_is_copied_tables_go_stale_and_late_poses_go_incremental():
    import octreelib_amd as oa
    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd import _native as nat
    from octreelib_amd.grid import Grid, GridConfig

    c = [synthetic.planar_cloud(20_001 + 500 * j, (5, 5, 5), seed=3, stream=j) for j in range(3)]
    T = _rigid(21, 0.2)
    # a DeviceCloud under a transform as the first pose is not read in place
    cloud = oa.upload_async(c[0])
    g = Grid(GridConfig(voxel_edge_length=1))
    g.insert_points(0, cloud, transform=T)
    assert not g._forest.reads_in_place(cloud) and g._forest._in_place is None
    nat.get_context().sync()
    cloud.release()                                     # (allowed: the copy has been consumed)
    twin = Grid(GridConfig(voxel_edge_length=1))
    twin.insert_points(0, transform_rows_np(T, c[0]))
    for grid in (g, twin):
        grid.insert_points(1, c[1])
        grid.subdivide([MaxPoints(48)])
    _assert_same_tables(_tables(g._forest), _tables(twin._forest))
    # derived tables made before an insert are stale after it
    before = g.leaf_planes()
    assert g.leaf_planes() is before
    g.insert_points(2, c[2].astype(np.float32), transform=T)
    twin.insert_points(2, transform_rows_np(T, c[2].astype(np.float32)))
    after, ref = g.leaf_planes(), twin.leaf_planes()
    assert after is not before and int(after.count.sum()) == int(before.count.sum()) + len(c[2])
    assert after.node.tobytes() == ref.node.tobytes() and after.count.tobytes() == ref.count.tobytes()
    assert after.mean.tobytes() == ref.mean.tobytes() and after.covariance.tobytes() == ref.covariance.tobytes()
    # ... and the late pose took the route its twin took
    a, b = g._forest.info, twin._forest.info
    assert [getattr(a, k) for k, _ in nat.BuildInfo._fields_] == [getattr(b, k) for k, _ in nat.BuildInfo._fields_]
    _assert_same_tables(_tables(g._forest), _tables(twin._forest))
    launches = []
    for grid in (g, twin):
        x = _counter("octl_debug_launches")
        if grid is g:
            grid.insert_points(3, c[0][::2], transform=T)
        else:
            grid.insert_points(3, transform_rows_np(T, c[0][::2]))
        y = _counter("octl_debug_launches")
        grid._forest.ensure_built()
        launches.append(_counter("octl_debug_launches") - y)
        assert y - x >= 1
    assert launches[0] == launches[1]                   # (the same build route: the incremental insertion)
    _assert_same_tables(_tables(g._forest), _tables(twin._forest))
    g._forest.close()
    twin._forest.close()


# ---- 8. differential fuzz ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(20))
def test_random_sequences_device_transform_against_host_twin(seed):
    """Random sequences of plain inserts, inserts and extends under a transform (rigid and piecewise; host f64, host
    f32, DeviceCloud), subdivide, RANSAC + apply_mask, transform_poses and nearest on two arms: the device transform
    and the host-transformed twin.  Even seeds drive a Grid (which has RANSAC and no extend), odd seeds an
    OctreeManager (which has extend); after every step the outcome and the tables are compared."""
    import octreelib_amd as oa
    from octreelib_amd import MaxPoints, synthetic
    from octreelib_amd.grid import Grid, GridConfig
    from octreelib_amd.octree import Octree, OctreeConfig
    from octreelib_amd.octree_manager import OctreeManager

    rng = np.random.default_rng(7000 + seed)
    is_grid = seed % 2 == 0
    L = int(rng.choice([1, 2]))
    table = _table(seed=seed, H=64)

    def make():
        if is_grid:
            return Grid(GridConfig(voxel_edge_length=L))
        return OctreeManager(Octree, OctreeConfig(), np.full(3, -32.0), 64.0)

    objs = {"dev": make(), "twin": make()}
    uploaded = []

    def small_T():
        return se3_exp(np.concatenate([rng.normal(size=3) * 0.5, rng.normal(size=3) * 0.5]))

    def plan_insert(extend):
        n = int(rng.integers(1, 2001))
        P = synthetic.planar_cloud(n + 1, (3, 3, 3), seed=seed, stream=int(rng.integers(0, 1 << 20)))[:n]
        mode = str(rng.choice(["plain", "rigid", "piecewise"])) if not extend else str(rng.choice(["rigid", "piecewise"]))
        form = str(rng.choice(["f64", "f32", "device"]))
        if form == "f32":
            P = P.astype(np.float32)
        T = seg = None
        if mode == "rigid":
            T = small_T()
        elif mode == "piecewise":
            m = int(rng.choice([1, 2, 7, 100]))
            T = np.stack([small_T() for _ in range(m)])
            seg = np.sort(rng.integers(0, m, n)) if rng.random() < 0.5 else rng.integers(0, m, n)
        return P, T, seg, form

    n_poses = 0

    def do_insert(pose, P, T, seg, form):
        def on(arm):
            obj = objs[arm]
            if arm == "twin":
                return obj.insert_points(pose, P if T is None else transform_rows_np(T, P, seg))
            src = P
            if form == "device":
                src = oa.upload_async(P)
                uploaded.append(src)
            if T is None:
                return obj.insert_points(pose, src)
            return obj.insert_points(pose, src, transform=T, segment=seg)
        return on

    def state(obj):
        return _tables(obj._forest), [obj.get_points(p).tobytes() for p in range(n_poses)]

    def step(on):
        a, b = _outcome(lambda: on("dev")), _outcome(lambda: on("twin"))
        assert a[0] == b[0], (a, b)
        if a[0] != "ok":
            assert a == b
        elif a[1] is not None:
            for x, y in zip(a[1], b[1]):
                assert np.array_equal(x, y, equal_nan=True)
        sa, sb = _outcome(lambda: state(objs["dev"])), _outcome(lambda: state(objs["twin"]))
        assert sa[0] == sb[0], (sa, sb)
        if sa[0] == "ok":
            _assert_same_tables(sa[1][0], sb[1][0])
            assert sa[1][1] == sb[1][1]
        else:
            assert sa == sb
        return a[0] == "ok"

    try:
        P, T, seg, form = plan_insert(True)          # (the first pose always goes in under a transform)
        assert step(do_insert(0, P, T, seg, form))
        n_poses = 1
        k = int(rng.integers(8, 64))
        assert step(lambda arm: objs[arm].subdivide([MaxPoints(k)]))
        ok = 0
        for _ in range(int(rng.integers(5, 9))):
            op = str(rng.choice(["insert", "extend", "subdivide", "ransac", "transform_poses", "nearest"]))
            if op == "insert":
                P, T, seg, form = plan_insert(False)
                if step(do_insert(n_poses, P, T, seg, form)):
                    ok += 1
                    n_poses += 1
            elif op == "extend" and not is_grid:
                P, T, seg, form = plan_insert(True)
                ok += step(do_insert(int(rng.integers(0, n_poses)), P, T, seg, form))
            elif op == "subdivide":
                k = int(rng.integers(8, 64))
                ok += step(lambda arm: objs[arm].subdivide([MaxPoints(k)]))
            elif op == "ransac" and is_grid:
                ok += step(lambda arm: objs[arm].map_leaf_points_cuda_ransac(hypotheses=table))
            elif op == "transform_poses":
                Ts = [small_T() for _ in range(n_poses)]
                ok += step(lambda arm: objs[arm].transform_poses(Ts))
                ok += step(lambda arm: objs[arm].subdivide([MaxPoints(k)]))
            elif op == "nearest":
                Q = rng.random((200, 3)) * 3.0

                def near(arm):
                    r = objs[arm].nearest(Q, k=2, max_distance=0.4)
                    return r.pose, r.index, r.distance2, r.count
                ok += step(near)
        print(f"seed {seed}: {'grid' if is_grid else 'manager'}, {n_poses} poses, {ok} further steps ok")
    finally:
        for o in objs.values():
            o._forest.close()
        from octreelib_amd import _native as nat

        nat.get_context().sync()
        for c in uploaded:
            c.release()
