"""The derived map tables of a forest - pooled leaf planes, adjustment moments, neighbour index, plane segments - are
stamped with the state of the forest they were made from (forest.h: content_stamp), and everything that changes the
block table, the ordered points, the node table or the pose offsets moves that stamp on.

Each table is kept for ONE pose selection (the last it was asked for), and a call with another selection makes it again
whatever its stamp says.  So the stamp decides only in the first call after a change that asks for the selection the
table holds.  For every mutator and for both selections, a forest A that holds all four tables for that selection is
changed and asked for the same selection first: the library's timers must show that all four tables were made again,
every array must equal, byte for byte, what a forest B that never made a table answers, and point_to_plane at the ABI,
which never recomputes, must refuse the old planes as stale.

raycast and registration_system keep no table of their own: the cube cast answers from the neighbour index (made in the
timed region nn_group), the plane cast and registration_system from the pooled planes (pool_group) - so MADE covers them.
A transform_poses that is refused (DomainError) is the opposite case: nothing may be made again, every answer stays."""

import numpy as np
import pytest

from octreelib_amd import _native as nat
from octreelib_amd._engine import Forest
from octreelib_amd.registration import se3_exp
from tests._util import set_option
from tests.test_cpu_segments import floor_and_wall

pytestmark = pytest.mark.gpu

K = 64
ORIGIN = np.array([2.0, 2.0, 1.5])
MOVE = [se3_exp([0.01, -0.02, 0.015, 0.05, -0.03, 0.02], ORIGIN), se3_exp([-0.015, 0.01, 0.02, -0.02, 0.04, 0.01], ORIGIN),
        se3_exp([0.02, 0.015, -0.01, 0.03, 0.02, -0.04], ORIGIN)]


def _rays(Q):
    """A fixed fan of rays from the queries: three directions per origin, one of them along an axis."""
    O = np.repeat(Q[:150], 3, axis=0)
    D = np.random.default_rng(3).normal(size=(len(O), 3))
    D[::3] = np.eye(3)[np.arange(len(O[::3])) % 3]
    return np.ascontiguousarray(O), np.ascontiguousarray(D)


def _scene():
    """(three poses of 2000 points, a late pose, points for extend_pose, queries) of the floor-and-wall cloud."""
    P = floor_and_wall()
    pick = np.random.default_rng(11).permutation(len(P))
    poses = [np.ascontiguousarray(P[pick[2000 * p: 2000 * (p + 1)]]) for p in range(3)]
    late = np.ascontiguousarray(P[pick[6000:7500]])
    extra = np.ascontiguousarray(P[pick[7500:8300]])
    Q = np.ascontiguousarray(P[pick[9000:9600]] + 0.003)
    return poses, late, extra, Q


def _make(poses, k=K):
    f = Forest(0, np.zeros(3), 1.0)
    for P in poses:
        f.add_pose(P)
    f.subdivide(k)
    return f


# the timed regions that only the making of a table opens: pooled planes, neighbour index, adjustment tables, segments
MADE = ("pool_group", "nn_group", "adj_group", "seg_init")


def _consume(f, Q, selections, made=None):
    """Every array the four consumers return, for the selections in the order given: {name: array}.  made: the timers
    of the first selection's calls must show exactly these of the regions MADE."""
    out = {}
    for i, slots in enumerate(selections):
        tag = "all" if slots is None else "0,2"
        if i == 0 and made is not None:
            f.ctx.set_profiling(True)
        try:
            pl = f.leaf_planes(slots)
            pp = f.point_to_plane(Q, slots)
            nn = f.nearest(Q, 4, 0.2, slots)
            ad = f.adjustment_system(slots=slots, origin=ORIGIN)
            sg = f.plane_segments(slots)
            rc = f.raycast(*_rays(Q), 3.0, 0.0, slots, "cube")
            rp = f.raycast(*_rays(Q), 3.0, 0.0, slots, "plane")
            rg = f.registration_system(Q, slots=slots, origin=ORIGIN, per_point=True)
            if i == 0 and made is not None:
                timers = f.ctx.timings()
                assert tuple(k for k in MADE if k in timers) == tuple(made), (tag, sorted(timers))
        finally:
            if i == 0 and made is not None:
                f.ctx.set_profiling(False)
        t = sg.segments
        for name, a in (("planes.node", pl.node), ("planes.count", pl.count), ("planes.mean", pl.mean),
                        ("planes.covariance", pl.covariance), ("planes.eigenvalues", pl.eigenvalues),
                        ("planes.eigenvectors", pl.eigenvectors), ("p2p.node", pp.node), ("p2p.row", pp.row),
                        ("p2p.distance", pp.distance), ("nn.slot", nn[0]), ("nn.index", nn[1]), ("nn.d2", nn[2]),
                        ("nn.count", nn[3]), ("adj.H", ad.H), ("adj.g", ad.g), ("adj.cost", ad.cost),
                        ("adj.n_points", ad.n_points), ("adj.n_blocks", ad.n_blocks),
                        ("adj.n_leaves", np.asarray(ad.n_leaves, dtype=np.int64)), ("seg.neighbour", sg.neighbour),
                        ("seg.label", sg.label), ("seg.root", t.root), ("seg.n_leaves", t.n_leaves),
                        ("seg.count", t.count), ("seg.mean", t.mean), ("seg.covariance", t.covariance),
                        ("seg.eigenvalues", t.eigenvalues), ("seg.eigenvectors", t.eigenvectors),
                        ("ray.cube.node", rc.node), ("ray.cube.t", rc.t), ("ray.cube.row", rc.row),
                        ("ray.plane.node", rp.node), ("ray.plane.t", rp.t), ("ray.plane.row", rp.row),
                        ("reg.H", rg.H), ("reg.g", rg.g), ("reg.cost", np.float64(rg.cost)),
                        ("reg.counts", np.array([rg.n_used, rg.n_located], dtype=np.int64)), ("reg.node", rg.node),
                        ("reg.row", rg.row), ("reg.residual", rg.residual)):
            out[f"{name}[{tag}]"] = np.ascontiguousarray(a)
    return out


def _point_to_plane_abi(f, Q):
    """octl_forest_point_to_plane as it is: against the pooled planes the device holds, never recomputed."""
    n = len(Q)
    node, row, dist = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n)
    rc = f.lib.octl_forest_point_to_plane(f.handle, nat.ptr(Q), n, 8, -1.0, nat.ptr(node), nat.ptr(row), nat.ptr(dist))
    return rc, bytes(f.lib.octl_last_error(f.ctx.handle))


# ---- the mutators: each takes the forest and the scene, and leaves the forest built -----------------------------------
def _late_pose(incremental):
    def run(f, poses, late, extra):
        set_option("NO_INCREMENTAL", 0 if incremental else 1)
        f.ctx.set_profiling(True)
        try:
            f.add_pose(late)
            f.ensure_built()
            timers = f.ctx.timings()
        finally:
            f.ctx.set_profiling(False)
        assert ("inc_place" in timers) == incremental, sorted(timers)     # (the path the case is about was taken)
    return run


def _extend_pose(f, poses, late, extra):
    f.extend_pose(1, extra)
    f.ensure_built()


def _rebuild_other_k(f, poses, late, extra):
    f.subdivide(24)


def _planar_build(f, poses, late, extra):
    f.subdivide_planar((-1, 1e-4, 16, 0))


def _adopt_scheme(f, poses, late, extra):
    other = _make(poses, 24)
    try:
        f.adopt_scheme(other)
    finally:
        other.close()


def _set_contents(f, poses, late, extra):
    """map_leaf_points with a function that keeps the first half of every leaf's points (they stay in their leaves)."""
    blk = {k: v.copy() for k, v in f.blocks.items()}
    xyz = f.xyz
    size = (blk["size"] + 1) // 2
    rows = np.concatenate([np.arange(a, a + n) for a, n in zip(blk["start"].tolist(), size.tolist())])
    f.set_contents(blk["node"], blk["slot"], size, xyz[rows])


def _ransac_device_mask(f, poses, late, extra):
    table = np.random.default_rng(5).random((128, 6))
    f.ransac_all(10, table, 0.01)
    f.apply_device_mask()


def _host_mask(f, poses, late, extra):
    keep = np.ones(f.n_ord, dtype=np.uint8)
    keep[::3] = 0
    f.apply_host_mask(keep)


def _filter_count(f, poses, late, extra):
    f.filter_count([0, 1, 2], 6, 1 << 30)


def _clear_and_again(f, poses, late, extra):
    """octl_forest_clear on the SAME device forest (its buffers and stale tables are the point), the wrapper's
    bookkeeping set back to that of an empty forest by hand (the wrapper has no clear of its own)."""
    f.ctx.check(f.lib.octl_forest_clear(f.handle))
    f.n_slots, f.slot_sizes, f.slot_epoch, f.slot_voxel_keys = 0, [], [], []
    f.epoch, f.has_scheme, f._dirty, f.info, f.n_ord = 0, False, True, None, 0
    f._creation_codes, f._code_origin = np.empty(0, dtype=np.int64), None
    f._member_next, f._member_pending, f._device_clouds, f._in_place = 0, [], [], None
    f._invalidate()
    for P in poses:
        f.add_pose(P)
    f.subdivide(K)


def _transform_poses(slots):
    """Move the poses of `slots` (None: all), then subdivide again: transform_poses leaves no scheme."""
    def run(f, poses, late, extra):
        f.transform_poses(MOVE if slots is None else [MOVE[s] for s in slots], slots)
        assert not f.has_scheme and f.info is None
        f.subdivide(K)
    return run


MUTATORS = [("late pose, incremental", _late_pose(True)), ("late pose, re-placed", _late_pose(False)),
            ("extend_pose", _extend_pose), ("rebuild with another K", _rebuild_other_k),
            ("planar build", _planar_build), ("adopt_scheme", _adopt_scheme), ("set_contents", _set_contents),
            ("RANSAC and apply_device_mask", _ransac_device_mask), ("apply_host_mask", _host_mask),
            ("filter_count", _filter_count), ("clear and the same poses again", _clear_and_again),
            ("transform_poses then subdivide", _transform_poses(None)),
            ("transform_poses of 0 2 then subdivide", _transform_poses([0, 2]))]


@pytest.mark.parametrize("held", [None, [0, 2]], ids=["holds_all", "holds_0_2"])
@pytest.mark.parametrize("what,mutate", MUTATORS, ids=[m[0].replace(" ", "_").replace(",", "") for m in MUTATORS])
def test_no_table_survives(what, mutate, held):
    poses, late, extra, Q = _scene()
    other = [0, 2] if held is None else None
    a, b = _make(poses), _make(poses)
    try:
        # A makes every table for both selections, `held` last: that is what its four tables hold; B makes none
        before = _consume(a, Q, (other, held), made=MADE)
        blocks = a.info.n_blocks
        leaves = len(before["planes.node[all]"])
        print(f"{what}: {leaves} leaves, {blocks} blocks, {a.info.n_nodes} nodes")
        assert leaves >= 100 and blocks >= 2 * leaves and a.info.n_nodes > a.info.n_voxels
        assert 0 < before["planes.count[0,2]"].sum() < before["planes.count[all]"].sum()    # (unselected blocks exist)
        # (the check that follows can tell: on the unchanged forest the held selection makes nothing again)
        a._pooled = None
        _consume(a, Q, (held,), made=())
        assert _point_to_plane_abi(a, Q)[0] == 0
        mutate(a, poses, late, extra)
        rc, err = _point_to_plane_abi(a, Q)
        assert rc == nat.OCTL_E_STATE and b"stale" in err, (what, rc, err)
        mutate(b, poses, late, extra)
        # the held selection first: nothing but the stamps can tell A that its tables are stale
        got = _consume(a, Q, (held, other), made=MADE)
        want = _consume(b, Q, (held, other), made=MADE)
        assert list(got) == list(want)
        for name in got:
            x, y = got[name], want[name]
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, name)
        # (... and the change was one that a table kept from before would have shown)
        changed = [n for n in got if got[n].shape != before[n].shape or got[n].tobytes() != before[n].tobytes()]
        if mutate is not _clear_and_again:
            assert any(n.startswith("planes.") for n in changed) and any(n.startswith("adj.") for n in changed), changed
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("held", [None, [0, 2]], ids=["holds_all", "holds_0_2"])
def test_refused_transform_poses_keeps_every_table(held):
    """The row of the matrix that is no mutator: a transform_poses the library refuses (a moved point leaves the voxel
    domain) changes nothing, so nothing may be made again and every answer is the one from before."""
    poses, late, extra, Q = _scene()
    other = [0, 2] if held is None else None
    a = _make(poses)
    try:
        before = _consume(a, Q, (other, held), made=MADE)
        far = np.eye(4)
        far[0, 3] = 2.0 ** 31      # 2^31 voxel edges
        mirror = (a.epoch, a.has_scheme, a._dirty, list(a.slot_epoch), a.n_ord)
        with pytest.raises(nat.DomainError):
            a.transform_poses([MOVE[0], far] if held is not None else [MOVE[0], MOVE[1], far], held)
        assert (a.epoch, a.has_scheme, a._dirty, list(a.slot_epoch), a.n_ord) == mirror and a.info is not None
        assert _point_to_plane_abi(a, Q)[0] == nat.OCTL_OK
        a._pooled = None
        got = _consume(a, Q, (held,), made=())
        assert got and set(got) <= set(before)
        for name in got:
            x, y = got[name], before[name]
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name
    finally:
        a.close()


@pytest.mark.parametrize("what,mutate", MUTATORS, ids=[m[0].replace(" ", "_").replace(",", "") for m in MUTATORS])
def test_raycast_on_two_tables_held_for_two_selections(what, mutate):
    """raycast is the consumer with two tables behind it, each with its own (stamp, selection) pair: the pooled planes
    for the plane cast, the neighbour index for the cube cast.  Forest A holds the planes for ALL poses and the
    neighbour index for [0, 2]; after the change both casts, for both selections, must equal what a forest B that held
    nothing answers, byte for byte - one stale table is enough for a wrong answer."""
    poses, late, extra, Q = _scene()
    a, b = _make(poses), _make(poses)
    try:
        a.leaf_planes(None)
        a.nearest(Q, 4, 0.2, [0, 2])
        mutate(a, poses, late, extra)
        mutate(b, poses, late, extra)
        O, D = _rays(Q)
        hit = 0
        # (each table is asked first for the selection it holds: nothing but its stamp can tell A that it is stale)
        for slots, surface in ((None, "plane"), ([0, 2], "cube"), ([0, 2], "plane"), (None, "cube")):
            x, y = a.raycast(O, D, 3.0, 0.0, slots, surface), b.raycast(O, D, 3.0, 0.0, slots, surface)
            for name in ("node", "t", "row"):
                assert getattr(x, name).tobytes() == getattr(y, name).tobytes(), (what, slots, surface, name)
            hit += int((x.node >= 0).sum())
        assert hit > len(O)      # (the fan sees the map)
    finally:
        a.close()
        b.close()
