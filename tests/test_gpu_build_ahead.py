"""
The partition front of a build on the context's ahead stream: the first kernels of scan i+1's build run
next to the RANSAC and the mask of scan i.  Results must not depend on it, and the library must fall back to the one
stream whenever anything it cannot vouch for was enqueued since the forest's previous build.

Every scenario is a script of library calls that runs twice, each time in a context of its own: with the ahead stream
allowed for every size (BUILD_AHEAD_MIN_POINTS = 0) and with NO_BUILD_AHEAD = 1.  "Equal" is bit for bit: node table
(in the numbering-free form of tests/test_gpu_parity.py), block table, permutation, the RANSAC mask where the script
reads it, kept points and blocks after settle.  Clouds: 170 k - 390 k points over 7^3 voxels (sizes that ask for the
same number of buckets, so that one cloud's key geometry is a hint for the next), K = 24: thousands of leaves, a
RANSAC launch (H = 1024, k = 6) that is still running when the next front is enqueued.
"""

import ctypes as C

import numpy as np
import pytest

from tests._util import assert_same_leaves, canon_from_list
from tests.test_gpu_parity import _canon_build

pytestmark = pytest.mark.gpu

H, KPTS, THR, K = 1024, 6, 0.01, 24
DIMS = (7, 7, 7)


def _table():
    return np.random.default_rng(11).random((H, KPTS))


_CLOUDS = {}


def _cloud(n, stream, shift=0.0):
    """Draw `stream` of the one planar scene (computed once per size and draw), moved by `shift` voxels along x."""
    from octreelib_amd import synthetic

    key = (n, stream)
    if key not in _CLOUDS:
        _CLOUDS[key] = synthetic.planar_cloud(n, DIMS, seed=1, stream=stream)
    return _CLOUDS[key] + np.array([shift, 0.0, 0.0]) if shift else _CLOUDS[key]


def _builds_ahead():
    from octreelib_amd import _native as nat

    c = C.c_uint64(0)
    nat.load().octl_debug_builds_ahead(C.byref(c))
    return c.value


class _Session:
    """One context, raw library calls: the scan loop of bench.py (clear / add_pose_adopt / build / ransac_all /
    apply_mask_async on one forest), which the engine's Forest - one object per map - does not spell."""

    def __init__(self, ahead, **options):
        from octreelib_amd import _native as nat

        self.nat, self.ctx, self.ahead = nat, nat.Context(0), ahead
        self.lib = self.ctx.lib
        self.ctx.set_option("BUILD_AHEAD_MIN_POINTS", 0)
        self.ctx.set_option("NO_BUILD_AHEAD", 0 if ahead else 1)
        for name, value in options.items():
            self.ctx.set_option(name, value)
        self.forests, self.bufs, self.pins = [], [], []
        self.table, self.e0 = _table(), np.zeros(8, np.int32)
        self.info = nat.BuildInfo()

    def forest(self):
        h = C.c_void_p()
        self.ctx.check(self.lib.octl_forest_create(self.ctx.handle, 0, self.nat.ptr(np.zeros(3)), 1.0, C.byref(h)))
        self.forests.append(h)
        return h

    def dev(self, pts=None, nbytes=0):
        d = C.c_void_p()
        self.ctx.check(self.lib.octl_dev_alloc(self.ctx.handle, max(nbytes, pts.nbytes if pts is not None else 16),
                                               C.byref(d)))
        if pts is not None:
            self.ctx.check(self.lib.octl_dev_upload(self.ctx.handle, d, self.nat.ptr(pts), pts.nbytes))
        self.bufs.append(d)
        return d

    def pinned(self, nbytes):
        h = C.c_void_p()
        self.ctx.check(self.lib.octl_host_alloc(self.ctx.handle, nbytes, C.byref(h)))
        self.pins.append(h)
        return h

    def insert(self, fh, d, n):
        self.ctx.check(self.lib.octl_forest_clear(fh))
        self.ctx.check(self.lib.octl_forest_add_pose_adopt(fh, d, n, None))

    def build(self, fh):
        self.ctx.check(self.lib.octl_forest_build(fh, K, None, 0, 0, 0, C.byref(self.info)))

    def ransac(self, fh, n_poses=1):
        self.ctx.check(self.lib.octl_forest_ransac_all(fh, 10, self.nat.ptr(self.e0[:n_poses]), n_poses,
                                                       self.nat.ptr(self.table), H, KPTS, THR))

    def mask(self, fh):
        n = C.c_int64(0)
        self.ctx.check(self.lib.octl_forest_get_mask(fh, 0, None, C.byref(n)))
        m = np.empty(n.value, np.uint8)
        self.ctx.check(self.lib.octl_forest_get_mask(fh, n.value, self.nat.ptr(m), C.byref(n)))
        return m

    def step(self, fh, d, n, read_mask=False):
        """One scan; returns (did its front run ahead, the RANSAC mask when asked for)."""
        a = _builds_ahead()
        self.insert(fh, d, n)
        self.build(fh)
        ran_ahead = _builds_ahead() - a
        self.ransac(fh)
        m = self.mask(fh) if read_mask else None
        self.ctx.check(self.lib.octl_forest_apply_mask_async(fh))
        return ran_ahead, m

    def tables(self, fh):
        """Everything a caller can see of the forest, after settle."""
        lib, ctx, ptr = self.lib, self.ctx, self.nat.ptr
        kept, n = C.c_int64(0), C.c_int64(0)
        ctx.check(lib.octl_forest_settle(fh, C.byref(kept)))
        ctx.check(lib.octl_forest_get_blocks(fh, 0, None, None, None, None, C.byref(n)))
        nb = n.value
        blk = {"node": np.empty(nb, np.int32), "slot": np.empty(nb, np.int32), "start": np.empty(nb, np.int64),
               "size": np.empty(nb, np.int32)}
        ctx.check(lib.octl_forest_get_blocks(fh, nb, ptr(blk["node"]), ptr(blk["slot"]), ptr(blk["start"]),
                                             ptr(blk["size"]), C.byref(n)))
        ctx.check(lib.octl_forest_get_nodes(fh, 0, None, None, None, None, None, None, None, C.byref(n)))
        nn = n.value
        nd = {k: np.empty(nn, np.int32) for k in ("voxel", "depth", "parent", "first_child", "epoch")}
        nd["corner"], nd["edge"] = np.empty((nn, 3)), np.empty(nn)
        ctx.check(lib.octl_forest_get_nodes(fh, nn, ptr(nd["voxel"]), ptr(nd["depth"]), ptr(nd["parent"]),
                                            ptr(nd["first_child"]), ptr(nd["corner"]), ptr(nd["edge"]), ptr(nd["epoch"]),
                                            C.byref(n)))
        ctx.check(lib.octl_forest_get_perm(fh, 0, None, C.byref(n)))
        perm = np.empty(n.value, np.int64)
        ctx.check(lib.octl_forest_get_perm(fh, n.value, ptr(perm), C.byref(n)))
        return {"nodes": nd, "blocks": blk, "perm": perm, "kept": kept.value, "n_blocks": nb}

    def close(self):
        for fh in self.forests:
            self.lib.octl_forest_destroy(fh)
        for d in self.bufs:
            self.lib.octl_dev_free(self.ctx.handle, d)
        for h in self.pins:
            self.lib.octl_host_free(self.ctx.handle, h)
        self.ctx.close()


def _assert_equal(a, b):
    assert (a["kept"], a["n_blocks"]) == (b["kept"], b["n_blocks"])
    na, ba = _canon_build((a["nodes"], a["blocks"]))
    nb, bb = _canon_build((b["nodes"], b["blocks"]))
    assert na == nb and ba == bb
    assert np.array_equal(a["perm"], b["perm"])


def _both(script, **options):
    """script(session) -> result, with the ahead stream and without; (ahead result, serial result)."""
    out = []
    for ahead in (True, False):
        s = _Session(ahead, **options)
        try:
            out.append(script(s))
            s.ctx.sync()
        finally:
            s.close()
    return out


def _leaves(t):
    nd, blk, perm = t["nodes"], t["blocks"], t["perm"]
    return canon_from_list([(nd["corner"][b], nd["edge"][b], perm[st:st + sz]) for b, st, sz in
                            zip(blk["node"].tolist(), blk["start"].tolist(), blk["size"].tolist()) if sz > 0])


_ORACLE = {}


def _oracle_leaves(n, stream, shift=0.0):
    """The leaves the NumPy oracle leaves of one scan of _cloud(n, stream, shift): insert, subdivide(K), RANSAC with the
    tests' table, apply_mask.  Computed once per cloud and shared."""
    from oracle import octree_np as onp
    from oracle import ransac_np as rnp

    key = (n, stream, shift)
    if key not in _ORACLE:
        pts = _cloud(n, stream, shift)
        og = onp.OGrid(1)
        og.insert_points(0, pts)
        og.subdivide(K)
        rows = og.leaf_table(0)
        mask = rnp.evaluate(np.vstack([pts[i] for _, _, i in rows]),
                            np.array([len(i) for _, _, i in rows], dtype=np.int32), _table(), THR)
        og.apply_mask(0, mask)
        _ORACLE[key] = canon_from_list(og.leaf_table(0))
    return _ORACLE[key]


# The clouds of the scan loops below: two draws of the scene and one moved by three voxels, which the previous scan's
# key geometry (its box padded by one voxel) does not fit - that hint is rejected with the RANSAC of the scan before it
# in flight, and so is the hint the moved cloud leaves for the scan behind it.  B and C are the clouds the loops END on:
# their last step is checked against the oracle.
A, B, C_MOVED = (300_000, 1), (260_000, 2), (170_000, 3, 3.0)


def _assert_oracle(t, cloud):
    assert_same_leaves(_leaves(t), _oracle_leaves(*cloud), ordered=False)


def _scan_loop(steps):
    keys = [A, B, C_MOVED]
    clouds = [_cloud(*k) for k in keys]

    def script(s):
        fh = s.forest()
        dev = [s.dev(c) for c in clouds]
        ahead, m = 0, None
        for i in range(steps):
            a, m = s.step(fh, dev[i % 3], len(clouds[i % 3]), read_mask=(i == steps - 1))
            ahead += a
        return ahead, m, s.tables(fh)

    (ahead, m_a, t_a), (serial, m_s, t_s) = _both(script)
    # Nothing is read back between the steps, so every build but the first has its front on the ahead stream - a
    # build whose hint is then rejected too (its second attempt is the serial one): exactly steps - 1
    assert (ahead, serial) == (steps - 1, 0)
    _assert_equal(t_a, t_s)
    assert np.array_equal(m_a, m_s)
    last = keys[(steps - 1) % 3]
    if last != A:
        _assert_oracle(t_a, last)


# ---- 1. the scan loop ----------------------------------------------------------------------------------------------
def test_scan_loop_runs_ahead_and_changes_no_result():
    # 12 steps; rejected hints: the moved cloud's (steps 2, 5, 8, 11) and those of the scan behind it (3, 6, 9)
    _scan_loop(12)


@pytest.mark.parametrize("steps", [2, 3, 4, 5, 6, 7])
def test_scan_loop_step_by_step(steps):
    """Every step of the loop's first two rounds, each as the LAST step of a loop of its own: reading a step's tables
    back in the middle of a loop is work the library cannot vouch for and would make the next build serial."""
    _scan_loop(steps)


# ---- 2. what makes the next build serial ---------------------------------------------------------------------------
# g: a second forest of the context that holds two host poses and is built BEFORE the loop starts, so that each case
# enqueues the one thing it names and nothing else; g2: a third, empty forest
def _leaf_stats(s, fh, g, g2, aux):
    ids = np.arange(64, dtype=np.int32)
    count, mean, cov = np.empty(64, np.int64), np.empty((64, 3)), np.empty((64, 6))
    s.ctx.check(s.lib.octl_forest_leaf_stats(g, s.nat.ptr(ids), 64, s.nat.ptr(count), s.nat.ptr(mean), s.nat.ptr(cov),
                                             None, None))


def _two_pose_ransac(s, fh, g, g2, aux):
    s.ransac(g, n_poses=2)      # (two poses: the listing order comes from order.hip's kernels, then ransac_launch)


def _add_pose_host(s, fh, g, g2, aux):
    pts = _cloud(20_000, 5)
    s.ctx.check(s.lib.octl_forest_add_pose(g2, s.nat.ptr(pts), len(pts), C.byref(C.c_int32(0))))


def _transform_poses(s, fh, g, g2, aux):
    T = np.ascontiguousarray(np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(1, 12), (2, 1)))
    s.ctx.check(s.lib.octl_forest_transform_poses(g, None, 0, s.nat.ptr(T)))


def _nearest(s, fh, g, g2, aux):
    q = _cloud(20_000, 5)[:256].copy()
    slot, index = np.empty(256, np.int32), np.empty(256, np.int64)
    d2, count = np.empty(256), np.empty(256, np.int32)
    s.ctx.check(s.lib.octl_forest_nearest(g, s.nat.ptr(q), 256, 1, 0.5, None, 0, s.nat.ptr(slot), s.nat.ptr(index),
                                          s.nat.ptr(d2), s.nat.ptr(count)))


def _second_forest_build(s, fh, g, g2, aux):
    s.insert(g, aux, B[0])
    s.build(g)


def _profiling(s, fh, g, g2, aux):
    s.ctx.set_profiling(True)


DISTURBANCES = {"leaf_stats": _leaf_stats, "two-pose ransac_all": _two_pose_ransac, "add_pose from host": _add_pose_host,
                "transform_poses": _transform_poses, "nearest": _nearest, "second forest's build": _second_forest_build,
                "profiling": _profiling}


@pytest.mark.parametrize("what", list(DISTURBANCES))
def test_next_build_is_serial_after(what):
    a, b = _cloud(*A), _cloud(*B)

    def script(s):
        fh, g, g2 = s.forest(), s.forest(), s.forest()
        da, db, aux = s.dev(a), s.dev(b), s.dev(b)
        for pts in (_cloud(20_000, 5), _cloud(15_000, 6)):
            s.ctx.check(s.lib.octl_forest_add_pose(g, s.nat.ptr(pts), len(pts), C.byref(C.c_int32(0))))
        s.build(g)
        s.step(fh, da, len(a))
        warm, _ = s.step(fh, db, len(b))          # (the loop is one that runs ahead)
        DISTURBANCES[what](s, fh, g, g2, aux)
        after, _ = s.step(fh, da, len(a))
        labels = None
        if what == "profiling":
            labels = sorted(s.ctx.timings())
            s.ctx.set_profiling(False)
        again, _ = s.step(fh, db, len(b))         # (and the loop recovers)
        return warm, after, again, labels, s.tables(fh)

    (warm, after, again, labels, t_a), (_, _, _, labels_serial, t_s) = _both(script)
    assert warm == 1, "the undisturbed loop did not run ahead: the case proves nothing"
    assert after == 0, f"the build behind {what} ran ahead"
    assert again == 1
    assert labels == labels_serial      # (profiling: the timing labels of the one-stream build)
    if what == "profiling":
        assert {"part_hist", "part_scatter", "bucket_build", "bucket_nodes", "ransac", "apply_mask"} <= set(labels)
    _assert_equal(t_a, t_s)
    _assert_oracle(t_a, B)


# ---- 3. two forests, two contexts ----------------------------------------------------------------------------------
def test_two_forests_alternating_on_one_context():
    a, b, c = _cloud(*A), _cloud(*B), _cloud(*C_MOVED)

    def script(s):
        f, g = s.forest(), s.forest()
        da, db, dc = s.dev(a), s.dev(b), s.dev(c)
        for i in range(4):
            s.step(f, (da, db)[i % 2], (len(a), len(b))[i % 2])
            s.step(g, (db, dc)[i % 2], (len(b), len(c))[i % 2])
        return s.tables(f), s.tables(g)

    (fa, ga), (fs, gs) = _both(script)
    _assert_equal(fa, fs)
    _assert_equal(ga, gs)
    _assert_oracle(fa, B)
    _assert_oracle(ga, C_MOVED)


def test_two_contexts_in_one_process():
    a, b, c = _cloud(*A), _cloud(*B), _cloud(*C_MOVED)

    def run(ahead):
        s, t = _Session(ahead), _Session(ahead)
        try:
            fs, ft = s.forest(), t.forest()
            ds, dt = [s.dev(a), s.dev(b)], [t.dev(b), t.dev(c)]
            for i in range(4):
                s.step(fs, ds[i % 2], (len(a), len(b))[i % 2])
                t.step(ft, dt[i % 2], (len(b), len(c))[i % 2])
            out = s.tables(fs), t.tables(ft)
            s.ctx.sync()
            t.ctx.sync()
            return out
        finally:
            s.close()
            t.close()

    (sa, ta), (ss, ts) = run(True), run(False)
    _assert_equal(sa, ss)
    _assert_equal(ta, ts)
    _assert_oracle(sa, B)
    _assert_oracle(ta, C_MOVED)


# ---- 4. the host feed of bench.py's run_pipelined ------------------------------------------------------------------
def test_pipelined_host_feed():
    """Six different scans through TWO device buffers, each scan from a pinned buffer of its own: the host never waits
    for a copy, so the upload into the cloud a build reads can still be in flight when its front is opened (the ahead
    stream must inherit the upload's event), and the next upload overwrites the buffer the previous scan was built
    from while this one is built (its gate must cover that scan's front)."""
    keys = [(260_000, 10 + i) for i in range(5)] + [B]
    scans = [_cloud(*k) for k in keys]
    nbytes = max(c.nbytes for c in scans)

    def script(s):
        fh = s.forest()
        pin, dbuf = [s.pinned(nbytes) for _ in scans], [s.dev(nbytes=nbytes), s.dev(nbytes=nbytes)]
        for h, c in zip(pin, scans):
            C.memmove(h, s.nat.ptr(c), c.nbytes)

        def upload(i):
            s.ctx.check(s.lib.octl_dev_upload_async(s.ctx.handle, dbuf[i & 1], pin[i], scans[i].nbytes))

        upload(0)
        ahead = 0
        for i in range(len(scans)):
            s.insert(fh, dbuf[i & 1], len(scans[i]))
            if i + 1 < len(scans):
                upload(i + 1)
            a = _builds_ahead()
            s.build(fh)
            ahead += _builds_ahead() - a
            s.ransac(fh)
            s.ctx.check(s.lib.octl_forest_apply_mask_async(fh))
        out = s.tables(fh)
        s.ctx.check(s.lib.octl_ctx_sync_uploads(s.ctx.handle))
        s.ctx.check(s.lib.octl_forest_clear(fh))
        return ahead, out

    (ahead, t_a), (serial, t_s) = _both(script)
    assert (ahead, serial) == (len(scans) - 1, 0)      # every build but the first
    _assert_equal(t_a, t_s)
    _assert_oracle(t_a, B)


# ---- 5. an error behind the front -----------------------------------------------------------------------------------
def test_domain_error_behind_a_front_that_ran_ahead():
    a, b = _cloud(*A), _cloud(*B)
    bad = b.copy()
    bad[12345, 1] = 3.0e12      # a top-level voxel index outside the domain: the histogram pass finds it

    def script(s):
        fh = s.forest()
        da, db, dbad = s.dev(a), s.dev(b), s.dev(bad)
        s.step(fh, da, len(a))
        s.step(fh, db, len(b))
        before = _builds_ahead()
        s.insert(fh, dbad, len(bad))
        with pytest.raises(s.nat.DomainError):
            s.build(fh)
        front_ahead = _builds_ahead() - before
        s.step(fh, db, len(b))
        out = s.tables(fh)
        s.ctx.sync()
        return front_ahead, out

    (front_ahead, t_a), (_, t_s) = _both(script)
    assert front_ahead == 1, "the failing build's front did not run ahead: the case proves nothing"
    _assert_equal(t_a, t_s)
    _assert_oracle(t_a, B)


# ---- 6. a front buffer has to grow ----------------------------------------------------------------------------------
def test_a_larger_cloud_than_any_before():
    small, big = _cloud(*B), _cloud(390_000, 4)     # (both ask for 256 buckets: the hint is usable)

    def script(s):
        fh = s.forest()
        ds, db = s.dev(small), s.dev(big)
        s.step(fh, ds, len(small))
        s.step(fh, ds, len(small))
        grew, _ = s.step(fh, db, len(big))       # the records of the partition do not fit the buffer any more
        s.step(fh, ds, len(small))
        return grew, s.tables(fh)

    (grew, t_a), (_, t_s) = _both(script)
    print(f"\nthe build whose records outgrew their buffer ran ahead: {bool(grew)}")   # (either is right)
    _assert_equal(t_a, t_s)
    _assert_oracle(t_a, B)


# ---- 7. the ahead stream cannot be had --------------------------------------------------------------------------------
def test_builds_stay_serial_while_the_ahead_stream_cannot_be_had():
    """The stream, its events and its status words are made by the first RANSAC behind a build that may be run ahead
    of.  When that fails - here: the allocation of the status words, through octl_debug_fail_alloc - nothing is
    reported, the next build is serial, and the RANSAC behind it tries again."""
    b = _cloud(*B)

    def script(s):
        fh = s.forest()
        db = s.dev(b)
        s.ctx.set_option("NO_BUILD_AHEAD", 1)
        for _ in range(2):                        # (every buffer of a step has its size; no ahead stream yet)
            s.step(fh, db, len(b))
        s.ctx.set_option("NO_BUILD_AHEAD", 0 if s.ahead else 1)
        s.insert(fh, db, len(b))
        s.build(fh)
        seen = C.c_int64(0)
        s.ctx.check(s.lib.octl_debug_fail_alloc(1, None))
        try:
            s.ransac(fh)                          # its one growth: the status words
        finally:
            s.ctx.check(s.lib.octl_debug_fail_alloc(0, C.byref(seen)))
        s.ctx.check(s.lib.octl_forest_apply_mask_async(fh))
        denied, _ = s.step(fh, db, len(b))
        granted, _ = s.step(fh, db, len(b))
        return seen.value, denied, granted, s.tables(fh)

    (seen, denied, granted, t_a), (seen_s, _, _, t_s) = _both(script)
    assert (seen, denied, granted) == (1, 0, 1) and seen_s == 0
    _assert_equal(t_a, t_s)
    _assert_oracle(t_a, B)
