"""apply_device_mask (csrc/mask.hip) against the NumPy model of tests/_maskmodel.py, at the shapes where a stream
compaction goes wrong: tails of n, both sides of the 256-point block split, empty tiles and empty block workgroups,
the size rule between the fused kernel (k_mask_scan) and the separate kernels at its limit, the in-place fill of
alive flags that were never written, and the alive flags as the next build reads them.

Every comparison is exact (integer tables with np.array_equal, coordinates by their bytes).  Every case runs under
the default switches and under NO_FUSED_TABLES=1.  The block tables are shaped with Forest.set_contents: a scheme
with one leaf per wanted block (two poses, K = 1: every point its own leaf), sizes chosen freely, rows drawn inside
their leaf's cube.  The property a case is about is asserted on the host arrays before the call."""

import ctypes as C

import numpy as np
import pytest

from tests._maskmodel import INT64_MAX, apply_mask_model, check_tables, filter_count_model
from tests._util import set_option

pytestmark = pytest.mark.gpu

GRID = (4.0, 4.0, 4.0)


def _launches():
    from octreelib_amd import _native as nat

    c = C.c_uint64(0)
    nat.get_context().check(nat.load().octl_debug_launches(C.byref(c)))
    return c.value


def _base_forest(n_pairs, seed=1):
    """Two poses of uniform points, subdivided until every point has a leaf of its own: n_pairs (leaf, pose) blocks."""
    from octreelib_amd._engine import Forest

    rng = np.random.default_rng([seed, n_pairs])
    a = (n_pairs + 1) // 2
    f = Forest(0, np.zeros(3), 1.0)
    f.add_pose(rng.random((a, 3)) * GRID)
    if n_pairs > a:
        f.add_pose(rng.random((n_pairs - a, 3)) * GRID)
    f.subdivide(1)
    assert len(f.blocks["node"]) == n_pairs
    return f


class _Table:
    """A block table with the given sizes on the (leaf, pose) pairs of _base_forest(len(sizes)), in table order."""

    def __init__(self, sizes, seed=1):
        self.sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        assert (self.sizes > 0).all()
        self.seed = seed
        self.node = self.slot = self.rows = None

    @property
    def n(self):
        return int(self.sizes.sum(dtype=np.int64))

    @property
    def starts(self):
        return np.cumsum(self.sizes, dtype=np.int64) - self.sizes

    def forest(self):
        f = _base_forest(len(self.sizes), self.seed)
        blk = f.blocks
        if self.rows is None:
            nd = f.nodes
            self.node, self.slot = blk["node"].copy(), blk["slot"].copy()
            per = np.repeat(self.node, self.sizes)
            u = np.random.default_rng([self.seed, 77]).random((len(per), 3)) * 0.96875 + 0.015625
            self.rows = nd["corner"][per] + u * nd["edge"][per][:, None]
        assert np.array_equal(blk["node"], self.node) and np.array_equal(blk["slot"], self.slot)
        f.set_contents(self.node, self.slot, self.sizes, self.rows)
        return f

    def check(self, t):
        """The tables the forest holds after set_contents are the ones that were asked for."""
        blocks, perm, xyz = t
        assert np.array_equal(blocks["node"], self.node) and np.array_equal(blocks["slot"], self.slot)
        assert np.array_equal(blocks["size"], self.sizes) and np.array_equal(blocks["start"], self.starts)
        assert xyz.tobytes() == self.rows.tobytes()
        assert np.array_equal(np.sort(perm), np.arange(self.n))
        # (leaf-major tables over a pose-major store: the identity only where the poses happen to lie in sequence)
        assert np.array_equal(perm, np.arange(self.n)) == bool((np.diff(self.slot) >= 0).all())


def _snapshot(f, table=None):
    blocks = {k: v.copy() for k, v in f.blocks.items()}
    perm = f.perm.copy()
    # (the two 2 M-point tables: set_contents stores the rows it was given verbatim - what the small tables check)
    xyz = table.rows if table is not None and table.n > 300_000 else f.xyz.copy()
    t = (blocks, perm, xyz)
    check_tables(*t)
    if table is not None:
        table.check(t)
    return t


def _assert_is_model(f, want):
    blocks, perm, xyz, n, nb = want
    assert f.n_ord == n
    got = f.blocks
    assert len(got["node"]) == nb
    for k in ("node", "slot", "start", "size"):
        assert np.array_equal(got[k], blocks[k]), k
    assert np.array_equal(f.perm, perm)
    assert f.xyz.tobytes() == xyz.tobytes()
    return blocks, perm, xyz


def _run_case(make, steps, table=None, after=None):
    """make() -> a forest; steps: callables (blocks, perm, xyz) -> mask, applied one after the other with the model
    chained; after(f, tables, closing list).  Both routes.  Returns the launches of every apply_host_mask per route."""
    launches = {}
    for no_fused in (0, 1):
        set_option("NO_FUSED_TABLES", no_fused)
        f = make()
        closing = []
        try:
            t = _snapshot(f, table)
            launches[no_fused] = []
            for step in steps:
                mask = np.ascontiguousarray(step(t), dtype=np.uint8)
                want = apply_mask_model(*t, mask)
                l0 = _launches()
                f.apply_host_mask(mask)
                launches[no_fused].append(_launches() - l0)
                t = _assert_is_model(f, want)
            if after is not None:
                after(f, t, closing)
        finally:
            f.close()
            for fn in closing:
                fn()
    set_option("NO_FUSED_TABLES", 0)
    return launches


def _bernoulli(p, seed=3):
    return lambda t: (np.random.default_rng([seed, len(t[1])]).random(len(t[1])) < p).astype(np.uint8)


def _kept_per_block(blocks, mask):
    cs = np.concatenate(([0], np.cumsum(mask != 0, dtype=np.int64)))
    return cs[blocks["start"] + blocks["size"]] - cs[blocks["start"]]


def _small_sizes(n, hi, rng):
    """Sizes in [1, hi] that sum to n."""
    out = []
    left = n
    while left > 0:
        s = int(min(left, rng.integers(1, hi + 1)))
        out.append(s)
        left -= s
    return out


# ---- tails and alignment -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["one_block", "small_blocks"])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2048, 2049, 4101])
def test_tails_and_alignment(n, layout):
    sizes = [n] if layout == "one_block" else _small_sizes(n, 5, np.random.default_rng(n))
    table = _Table(sizes, seed=2)
    assert table.n == n and (layout == "one_block" or n == 1 or len(sizes) >= max(2, n // 5))

    def only(i):
        def step(t):
            m = np.zeros(len(t[1]), dtype=np.uint8)
            m[i] = 1
            return m
        return step

    for step in (_bernoulli(0.5), lambda t: np.ones(len(t[1]), dtype=np.uint8),
                 lambda t: np.zeros(len(t[1]), dtype=np.uint8), only(0), only(-1)):
        _run_case(table.forest, [step], table)


# ---- both sides of the 256-point block split -----------------------------------------------------------------------
def _split_table(shape):
    rng = np.random.default_rng(17)
    if shape == "mixed":
        sizes = [1, 63, 64, 255, 256, 257, 320, 2048, 2049, 5000] + [200] * 12 + [1, 256, 257, 3]
    elif shape == "lanes":
        sizes = rng.integers(1, 41, 192)
        for i, s in ((0, 257), (63, 300), (64 + 3, 1000), (64 + 4, 2049), (64 + 60, 513)):
            sizes[i] = s
    elif shape == "last_workgroup":
        sizes = rng.integers(1, 9, 261)
        sizes[259] = 777
    else:
        nb = int(shape)
        sizes = rng.integers(1, 7, nb)
        sizes[0], sizes[nb // 2], sizes[nb - 1] = 300, 257, 256
    return _Table(sizes, seed=3)


@pytest.mark.parametrize("shape", ["mixed", "lanes", "last_workgroup", "255", "256", "257", "513"])
def test_both_sides_of_the_256_point_block_split(shape):
    table = _split_table(shape)
    sizes, starts = table.sizes, table.starts
    big = sizes > 256
    straddles = starts // 2048 != (starts + sizes - 1) // 2048
    if shape == "mixed":
        assert set([1, 63, 64, 255, 256, 257, 320, 2048, 2049, 5000]) <= set(sizes.tolist())
        assert (straddles & big).any() and (straddles & ~big).any()      # blocks across tile boundaries, both paths
    elif shape == "lanes":
        assert big[0] and big[63] and big[:64].sum() == 2                # lanes 0 and 63 of the first wave
        assert big[64:128].sum() == 3 and big[128:].sum() == 0           # three in one wave, none in the next
        assert len(sizes) <= 256 and table.n > 2048
    elif shape == "last_workgroup":
        nb = len(sizes)
        assert nb % 256 != 0 and big.sum() == 1 and np.flatnonzero(big)[0] >= 256 * (nb // 256)
    else:
        assert len(sizes) == int(shape) and big.any() and (sizes == 256).any()
    # two masks in a row: the second one meets the halved blocks, on the other side of the split
    _run_case(table.forest, [_bernoulli(0.5), _bernoulli(0.5, seed=4)], table)


# ---- mask content --------------------------------------------------------------------------------------------------
def _content_table():
    rng = np.random.default_rng(23)
    sizes = rng.integers(1, 41, 700)
    sizes[100] = 600
    if sizes.sum() % 2 == 0:
        sizes[5] += 1
    return _Table(sizes, seed=4)


def _mask_bytes(t):
    values = np.array([0, 1, 2, 0x7F, 0x80, 0xFF], dtype=np.uint8)
    m = np.random.default_rng(29).choice(values, len(t[1]))
    assert set(m.tolist()) == set(values.tolist())
    return m


def _mask_empty_tiles(t):
    n = len(t[1])
    m = _bernoulli(0.5)(t)
    m[2048:4 * 2048] = 0
    per_tile = np.add.reduceat(m.astype(np.int64), np.arange(0, n, 2048))
    assert len(per_tile) >= 6 and (per_tile[1:4] == 0).all() and per_tile[0] > 0 and (per_tile[4:] > 0).all()
    return m


def _mask_empty_blocks(t):
    blocks = t[0]
    m = _bernoulli(0.5)(t)
    lo, hi = int(blocks["start"][200]), int(blocks["start"][560])
    m[lo:hi] = 0
    kept = _kept_per_block(blocks, m)
    assert (kept[200:560] == 0).all() and (kept[256:512] == 0).all()    # blocks 256..511: a whole block workgroup
    assert kept[:200].sum() > 0 and kept[560:].sum() > 0 and len(kept) >= 700
    return m


@pytest.mark.parametrize("content", ["bytes", "p002", "p050", "p098", "empty_tiles", "empty_blocks", "two_in_a_row"])
def test_mask_content(content):
    table = _content_table()
    assert table.n > 6 * 2048 and table.n % 8 != 0 and len(table.sizes) == 700
    steps = {
        "bytes": [_mask_bytes],
        "p002": [_bernoulli(0.02)],
        "p050": [_bernoulli(0.5)],
        "p098": [_bernoulli(0.98)],
        "empty_tiles": [_mask_empty_tiles],
        "empty_blocks": [_mask_empty_blocks],
        "two_in_a_row": [_bernoulli(0.7), _bernoulli(0.3, seed=5), _bernoulli(0.5, seed=6)],
    }[content]
    _run_case(table.forest, steps, table)


def test_a_mask_of_zeros_leaves_an_empty_forest_that_still_works():
    table = _content_table()

    def after(f, t, closing):
        assert f.n_ord == 0 and len(f.blocks["node"]) == 0 and len(f.perm) == 0 and f.xyz.shape == (0, 3)
        f.apply_host_mask(np.zeros(0, dtype=np.uint8))
        assert f.n_ord == 0 and len(f.blocks["node"]) == 0
        f.subdivide(4)
        assert f.n_ord == 0 and len(f.blocks["node"]) == 0 and len(f.perm) == 0
        assert int(f.info.n_points) == 0 and int(f.info.n_blocks) == 0

    _run_case(table.forest, [lambda t: np.zeros(len(t[1]), dtype=np.uint8)], table, after)


# ---- the route rule at its limit -----------------------------------------------------------------------------------
def _workgroups(n, nb):
    return -(-n // 2048) + 2 * -(-nb // 256)


class _Plain:
    """The base forest itself as the table: nb == n, every block one point."""

    def __init__(self, n):
        self.n, self.sizes = n, np.ones(n, dtype=np.int32)

    def forest(self):
        return _base_forest(self.n, seed=5)


def _route_pair(pair):
    if pair == "long_tile_chain":
        # 3000 blocks of about 680 points: nearly every block takes the wave path; nt = 1000 / 1001, nbw = 12
        sizes = np.random.default_rng(31).integers(300, 1066, 3000)
        d = 2_048_000 - int(sizes.sum())
        sizes += d // 3000
        sizes[: d % 3000] += 1
        more = sizes.copy()
        more[-1] += 1
        assert (sizes > 256).mean() > 0.95
        return _Table(sizes, seed=5), _Table(more, seed=5)
    # 123 000 blocks, 2000 of them of two points: nt = 62, nbw = 481; then nb = n = 123 137: nt = 61, nbw = 482
    sizes = np.ones(123_000, dtype=np.int32)
    sizes[np.random.default_rng(37).choice(123_000, 2000, replace=False)] = 2
    return _Table(sizes, seed=5), _Plain(123_137)


@pytest.mark.parametrize("pair", ["long_tile_chain", "long_block_chains"])
def test_the_route_rule_at_its_limit(pair):
    """ceil(n / 2048) + 2 ceil(nb / 256) = 1024 takes the fused kernel, 1025 the separate ones; the two routes are
    told apart by their launches, which are read off a small table first."""
    from octreelib_amd import _native as nat

    # (the look-back status words of both routes at their largest: no fill of a grown array inside a count)
    ctx = nat.get_context()
    warm = np.ones(1024 * 2048, dtype=np.uint32)
    out, total = np.empty_like(warm), C.c_uint32(0)
    ctx.check(ctx.lib.octl_debug_exclusive_scan(ctx.handle, nat.ptr(warm), len(warm), nat.ptr(out), C.byref(total)))
    assert total.value == len(warm)
    small = _Table([3, 5, 300, 2, 7], seed=6)
    got = _run_case(small.forest, [_bernoulli(0.5)], small)
    fused, unfused = got[0][0], got[1][0]
    assert fused != unfused, (fused, unfused)
    print(f"launches of apply_host_mask: fused {fused}, unfused {unfused}")
    limit, past = _route_pair(pair)
    assert _workgroups(limit.n, len(limit.sizes)) == 1024 and _workgroups(past.n, len(past.sizes)) == 1025
    if pair == "long_tile_chain":
        assert (limit.n, past.n, len(limit.sizes)) == (2_048_000, 2_048_001, 3000)
    else:
        assert (limit.n, len(limit.sizes), past.n, len(past.sizes)) == (125_000, 123_000, 123_137, 123_137)
    for shape, default_route in ((limit, fused), (past, unfused)):
        got = _run_case(shape.forest, [_bernoulli(0.5)], shape if isinstance(shape, _Table) else None)
        assert got[1][0] == unfused, (got, fused, unfused)
        assert got[0][0] == default_route, (got, fused, unfused)


# ---- the alive flags, observed through the next build --------------------------------------------------------------
def _canon_build(f, with_history):
    """The tables of a build independent of the node numbering: nodes keyed by (voxel, child path), blocks in storage
    order, the reference's listing order.  with_history: epochs and the listing order, which depend on the sequence
    of subdivisions a forest has seen, not only on its points."""
    from octreelib_amd._engine import _node_paths

    nd, blk = f.nodes, f.blocks
    paths = _node_paths(nd)
    keys = [(int(v), p) for v, p in zip(nd["voxel"].tolist(), paths)]
    nodes = {k: (int(nd["depth"][i]), nd["corner"][i].tobytes(), nd["edge"][i].tobytes(),
                 bool(nd["first_child"][i] >= 0), int(nd["epoch"][i]) if with_history else None)
             for i, k in enumerate(keys)}
    assert len(nodes) == len(keys)
    blocks = [(keys[b], int(s), int(st), int(sz)) for b, s, st, sz in
              zip(blk["node"].tolist(), blk["slot"].tolist(), blk["start"].tolist(), blk["size"].tolist())]
    order = [blocks[b][:2] for b in f.order.tolist()] if with_history else None
    return nodes, blocks, order, f.voxels.copy(), f.xyz.copy(), f.perm.copy()


def _assert_rebuild_equals_a_fresh_forest(f, store, slot_sizes, K2, replay=None):
    """f has been masked: subdivide(K2) must give the tables of a fresh forest that holds only the survivors (per
    pose, in store order).  perm keeps naming the points by their index in the store, dead ones included
    (octl_forest_get_perm), so the fresh forest's perm maps through the survivors' store indices.  replay: the K of
    the subdivision f saw before the mask when that one split nothing - the fresh forest is taken through the same
    sequence, and then epochs and listing order are compared as well.  Voxels whose points all died stay in a
    forest as empty roots (a Grid keeps its managers), so every voxel must keep a survivor for the comparison."""
    from octreelib_amd._engine import Forest

    surv = np.sort(f.perm)
    assert len(np.unique(np.floor(store[surv]), axis=0)) == len(f.voxels)
    off = np.concatenate(([0], np.cumsum(slot_sizes)))
    f.subdivide(K2)
    got = _canon_build(f, replay is not None)
    g = Forest(0, np.zeros(3), 1.0)
    try:
        for s in range(len(slot_sizes)):
            ids = surv[(surv >= off[s]) & (surv < off[s + 1])]
            assert len(ids) > 0
            g.add_pose(store[ids])
        if replay is not None:
            g.subdivide(replay)
            assert (g.nodes["first_child"] < 0).all()
        g.subdivide(K2)
        want = _canon_build(g, replay is not None)
    finally:
        g.close()
    assert (np.array([v[3] for v in want[0].values()])).any()          # K2 splits: a real placement
    assert got[0] == want[0]
    assert got[1] == want[1]
    assert got[2] == want[2]
    assert np.array_equal(got[3], want[3])
    assert got[4].tobytes() == want[4].tobytes()
    assert np.array_equal(got[5], surv[want[5]])
    assert got[4].tobytes() == store[got[5]].tobytes()


@pytest.mark.parametrize("p", [0.02, 0.98])
@pytest.mark.parametrize("route", ["bucket_build", "level_loop"])
def test_alive_flags_as_the_next_build_reads_them(route, p):
    from octreelib_amd._engine import Forest

    K1, K2 = 1_000_000, 6
    for n_store in (6000, 6001):
        for last_alive in (False, True):
            if route == "level_loop":
                set_option("NO_BUCKET_BUILD", 1)
            rng = np.random.default_rng([n_store, int(last_alive)])
            sizes = [n_store // 2 + 7, n_store - n_store // 2 - 7]
            store = rng.random((n_store, 3)) * (2.0, 2.0, 2.0)

            def make():
                f = Forest(0, np.zeros(3), 1.0)
                f.add_pose(store[: sizes[0]])
                f.add_pose(store[sizes[0]:])
                f.subdivide(K1)
                assert (f.nodes["first_child"] < 0).all() and len(f.voxels) == 8
                return f

            def step(t):
                perm = t[1]
                m = (np.random.default_rng(41).random(len(perm)) < p).astype(np.uint8)
                m[perm == n_store - 1] = 1 if last_alive else 0
                assert len(perm) == n_store and n_store % 2 == n_store - 6000
                assert bool(m[np.flatnonzero(perm == n_store - 1)[0]]) == last_alive
                assert abs(m.mean() - p) < 0.01
                return m

            def after(f, t, closing):
                assert store[t[1]].tobytes() == t[2].tobytes()
                _assert_rebuild_equals_a_fresh_forest(f, store, sizes, K2, replay=K1)

            _run_case(make, [step], None, after)


# ---- the in-place fill of alive flags that were never written ----------------------------------------------------------
@pytest.mark.parametrize("K1", [40, 1_000_000])
@pytest.mark.parametrize("n_store", [4099, 6149])
def test_in_place_alive_fill_of_an_adopted_cloud(n_store, K1):
    """A cloud adopted on the device has no alive flags until something needs them: the first apply_mask writes them
    inside its own kernels (by position in k_blk_kept, by store index in k_mask_scan).  The next build reads them."""
    from octreelib_amd import _native as nat
    from octreelib_amd._engine import Forest

    ctx = nat.get_context()
    assert n_store % 2 == 1 and n_store % 8 != 0 and n_store > 2 * 2048
    store = np.ascontiguousarray(np.random.default_rng(n_store).random((n_store, 3)) * (2.0, 2.0, 2.0))

    def make_and_free():
        d = C.c_void_p()
        ctx.check(ctx.lib.octl_dev_alloc(ctx.handle, store.nbytes, C.byref(d)))
        ctx.check(ctx.lib.octl_dev_upload(ctx.handle, d, nat.ptr(store), store.nbytes))
        f = Forest(0, np.zeros(3), 1.0)
        f.add_pose_device(d, n_store, adopt=True)
        f.subdivide(K1)
        assert bool((f.nodes["first_child"] >= 0).any()) == (K1 < n_store)
        return f, lambda: ctx.check(ctx.lib.octl_dev_free(ctx.handle, d))

    for no_bucket in (0, 1):
        frees = []

        def make():
            set_option("NO_BUCKET_BUILD", no_bucket)
            # (a forest of the same size whose points all die, closed: an allocation of the size of the alive flags
            #  that holds zeros is what the allocator has at hand - a flag the fill misses then reads "dead" and not
            #  whatever an earlier test left there; best effort, the flags themselves cannot be read from the host)
            f, free = make_and_free()
            f.apply_host_mask(np.zeros(n_store, dtype=np.uint8))
            assert f.n_ord == 0
            f.close()
            free()
            f, free = make_and_free()
            frees.append(free)
            return f

        def after(f, t, closing):
            closing.append(frees.pop())
            assert store[t[1]].tobytes() == t[2].tobytes()
            _assert_rebuild_equals_a_fresh_forest(f, store, [n_store], 15, replay=K1 if K1 > n_store else None)

        _run_case(make, [_bernoulli(0.5, seed=n_store)], None, after)
        assert not frees
    set_option("NO_BUCKET_BUILD", 0)


# ---- the device-mask entry -----------------------------------------------------------------------------------------
def _ransac_scene():
    from octreelib_amd import synthetic
    from octreelib_amd._engine import Forest

    f = Forest(0, np.zeros(3), 1.0)
    f.add_pose(synthetic.planar_cloud(9001, (3, 3, 2), seed=2, stream=1))
    f.add_pose(synthetic.planar_cloud(7003, (3, 3, 2), seed=2, stream=2))
    f.subdivide(40)
    return f


def _ransac_on_every_other_block(f, t):
    """RANSAC on half of the blocks; the mask it leaves, after asserting what the other half reads."""
    blocks = t[0]
    sub = np.ascontiguousarray(f.order[::2])
    np.random.seed(0)
    f.ransac_blocks(sub, np.random.random((256, 6)), 0.01)
    m = f.device_mask()
    evaluated = np.zeros(len(blocks["node"]), dtype=bool)
    evaluated[sub] = True
    per_pos = np.repeat(evaluated, blocks["size"])
    assert len(m) == len(per_pos) and (m[~per_pos] == 1).all()        # blocks that were not evaluated read 1
    assert (m[per_pos] == 0).any() and (m[per_pos] != 0).any() and (~per_pos).any()
    return m


@pytest.mark.parametrize("entry", ["apply_mask", "apply_mask_async"])
def test_the_device_mask_entry(entry):
    for no_fused in (0, 1):
        set_option("NO_FUSED_TABLES", no_fused)
        f = _ransac_scene()
        try:
            t = _snapshot(f)
            assert len(np.unique(t[0]["slot"])) == 2 and len(t[1]) == 16004
            m = _ransac_on_every_other_block(f, t)
            want = apply_mask_model(*t, m)
            if entry == "apply_mask":
                n = C.c_int64(-1)
                f.ctx.check(f.lib.octl_forest_apply_mask(f.handle, C.byref(n)))
                assert n.value == want[3]
                f.n_ord = n.value
                f._invalidate()
            else:
                f.apply_device_mask()
                assert f.n_ord == want[3]
            _assert_is_model(f, want)
        finally:
            f.close()
    set_option("NO_FUSED_TABLES", 0)


# ---- filter_count ----------------------------------------------------------------------------------------------------
def _filter_table():
    rng = np.random.default_rng(43)
    sizes = rng.integers(1, 80, 90)
    for i, s in ((0, 1), (7, 64), (8, 65), (30, 257), (31, 5000), (60, 64), (61, 65), (88, 257), (89, 1)):
        sizes[i] = s
    sizes[40:48] = 300
    return _Table(sizes, seed=7)


def _intervals():
    out = [(0, INT64_MAX), (5, 4), (INT64_MAX, 0)]
    for c in (64, 65, 66, 256, 257, 258):
        out += [(c, INT64_MAX), (0, c - 1)]
    return out


@pytest.mark.parametrize("selection", ["none", "one", "all"])
def test_filter_count(selection):
    table = _filter_table()
    assert {1, 64, 65, 257, 5000} <= set(table.sizes.tolist())
    slots = {"none": (), "one": (1,), "all": (0, 1)}[selection]
    sel = np.zeros(2, dtype=np.uint8)
    sel[list(slots)] = 1
    for lo, hi in _intervals():
        for no_fused in (0, 1):
            set_option("NO_FUSED_TABLES", no_fused)
            f = table.forest()
            try:
                t = _snapshot(f, table)
                want = filter_count_model(*t, sel, lo, hi)
                if (lo, hi) == (0, INT64_MAX) or not slots:
                    assert want[3] == table.n and want[4] == len(table.sizes)          # nothing changes
                elif lo > hi:
                    assert want[3] == int(table.sizes[np.isin(table.slot, slots, invert=True)].sum())
                else:
                    # the bound bites in both poses: a pose that is not selected keeps what the other loses
                    everywhere = filter_count_model(*t, np.ones(2, dtype=np.uint8), lo, hi)[3]
                    assert 0 < everywhere < want[3] < table.n if selection == "one" else 0 < want[3] < table.n
                f.filter_count(slots, lo, hi)
                _assert_is_model(f, want)
            finally:
                f.close()
    set_option("NO_FUSED_TABLES", 0)


def test_filter_count_on_top_of_an_unapplied_ransac_mask():
    """octl_forest_filter_count with a RANSAC mask pending: the filter clears the emptied leaves' bytes in that
    mask and one compaction applies both (include/octreelib_hip.h)."""
    for no_fused in (0, 1):
        set_option("NO_FUSED_TABLES", no_fused)
        f = _ransac_scene()
        try:
            t = _snapshot(f)
            m = _ransac_on_every_other_block(f, t)
            c = int(np.median(t[0]["size"][t[0]["slot"] == 1]))
            sel = np.array([0, 1], dtype=np.uint8)
            want = filter_count_model(*t, sel, c, INT64_MAX, mask=m)
            only_filter = filter_count_model(*t, sel, c, INT64_MAX)
            only_mask = apply_mask_model(*t, m)
            assert want[3] < min(only_filter[3], only_mask[3])               # both took points away
            f.filter_count((1,), c, INT64_MAX)
            _assert_is_model(f, want)
        finally:
            f.close()
    set_option("NO_FUSED_TABLES", 0)
