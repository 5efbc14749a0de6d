"""The operation-sequence generator and its oracle model, alone (tests/_opseq.py; the device side is
tests/test_gpu_opseq.py): the caps the seed set must meet, the replay that forks a model, the model-side sanity of the
scenes, and the NumPy specifications of the queries on the model's own tables."""

import collections
import hashlib

import numpy as np
import pytest

from octreelib_amd.leaf_stats import leaf_statistics_np
from octreelib_amd.query import HostMap
from tests import _opseq as S


@pytest.mark.parametrize("seed", S.SEEDS)
def test_sequence_caps_replay_and_scene(seed):
    q = S.generate(seed)
    assert 8 <= len(q.log) <= 20, q.printed()
    assert len(q.log) == len(q.obs) == len(q.meta)
    assert q.rejected <= 0.25 * q.draws, (q.rejected, q.draws)
    # replaying the log on a fresh model reproduces every recorded observation: the fork mechanism
    m = S.Model(q.container)
    for i, op in enumerate(q.log):
        m.apply(op)
        assert m.observe() == q.obs[i], f"step {i}\n{q.printed(i)}"
        assert m.pooled == q.meta[i]["pooled"]
    # the scenes
    assert q.flags == {"depth2": True, "emptied": True, "late100": True}, q.printed()
    assert q.closest > 1e-9
    for p, (table, counters) in q.obs[-1].items():
        assert counters[1] == len(table) and counters[2] == sum(d[0] for _, d in table)


def test_seed_set_covers_kinds_containers_and_transitions():
    kinds, trans, containers, f32 = collections.Counter(), collections.Counter(), collections.Counter(), 0
    worst = 0.0
    for seed in S.SEEDS:
        q = S.generate(seed)
        kinds.update(op["op"] for op in q.log)
        trans.update(S.transitions(q.log))
        containers[q.container["kind"] + (str(q.container["edge"]) if q.container["kind"] == "grid" else "")] += 1
        f32 += any(op.get("cloud", {}).get("form") == "f32" for op in q.log)
        worst = max(worst, q.rejected / q.draws)
    # most mutating operations (the inserts into an empty container aside) have a read-only one directly before and
    # one directly after them
    n_mut = before = after = 0
    for seed in S.SEEDS:
        log = S.generate(seed).log
        ro = lambda i: 0 <= i < len(log) and log[i]["op"] in S.READ_ONLY
        first = next(i for i, op in enumerate(log) if op["op"] != "insert")
        for i in range(first, len(log)):
            if log[i]["op"] in S.MUTATING:
                n_mut, before, after = n_mut + 1, before + ro(i - 1), after + ro(i + 1)
    print("mutating:", n_mut, "read-only directly before:", before, "directly after:", after)
    assert 2 * before > n_mut and 2 * after > n_mut
    print("kinds:", dict(kinds))
    print("transitions:", dict(trans))
    print("containers:", dict(containers), "f32 seeds:", f32, "worst rejection share:", worst)
    for k in S.MUTATING + S.READ_ONLY:
        assert kinds[k] >= 5, (k, kinds[k])
    for t in S.TRANSITIONS:
        assert trans[t] >= 2, (t, trans[t])
    for c in ("manager", "octree"):
        assert containers[c] >= 4, containers
    assert sum(v for k, v in containers.items() if k.startswith("grid")) >= 4
    assert {"grid1", "grid2", "grid5"} <= set(containers)
    assert 3 * f32 >= len(S.SEEDS)
    assert sum(any(op.get("cloud", {}).get("utm") for op in S.generate(s).log) for s in S.SEEDS) >= 2
    forms = {op["cloud"]["form"] for s in S.SEEDS for op in S.generate(s).log if "cloud" in op}
    assert forms == {"f64", "f32", "fortran", "strided"}


# sha256(repr((repr(q.log), q.obs, q.meta)))[:16] of generate(seed), computed in a worktree of the commit before the
# second generation was added to tests/_opseq.py: the logs, observations and bookkeeping of the old seeds have not moved
OLD_SEED_DIGESTS = {
    0: "95a2e04756336fe4", 1: "a47d2a41cdd7313f", 2: "4785a4e202a0f090", 3: "692243ba79e4e1c6", 4: "1740aa98184586af",
    5: "8fc1ed819b922469", 6: "8e1940261ed01b41", 7: "93c8547dfeb7a130", 8: "c54241329f2602e6", 9: "e781eea442ff06c9",
    10: "8544a8e2e0447059", 11: "2c085854707350f1", 12: "6218001093344c3d", 13: "a5bfab1d125c972a",
    14: "9f6dbed3ae3e5502", 15: "29200b693b0239a3", 16: "d3a26c6200974371", 17: "a16e3c9fca33e683",
    18: "b7eea9eddb465ae1", 19: "8d3661ac86cc7b6c", 20: "cb2d2af59969bbe3", 21: "5c50425115225781",
    22: "cf2ece52637c0c4d", 23: "3bf9f27738f50aaa"}


@pytest.mark.parametrize("seed", S.SEEDS)
def test_old_seeds_are_what_they_were(seed):
    q = S.generate(seed)
    assert hashlib.sha256(repr((repr(q.log), q.obs, q.meta)).encode()).hexdigest()[:16] == OLD_SEED_DIGESTS[seed]
    assert not any(op["op"] in S.NEW_MUTATING + S.NEW_READ_ONLY for op in q.log)


# the same digests for the second generation, computed in a worktree of the commit before the third generation was added
SEED2_DIGESTS = {
    100: "9999249236589868", 101: "b448246429d07c7f", 102: "1960e49fa2919f33", 103: "e569af0fc2857c06",
    104: "78bfdb6c318ba29b", 105: "5c43b819ab821420", 106: "4f21db003e77fea9", 107: "cf4808228d14a502",
    108: "89a0b2fee823447f", 109: "db7718fa4bcf9c78", 110: "750aa59c01398276", 111: "2cf2be0812efdad4",
    112: "7c984036ca2bd2f2", 113: "4377fb9c58bfb736", 114: "6791968be05ae953", 115: "4786ff537ec8267a",
    116: "ffc9f88d92653370", 117: "89cebb7a596d30ec", 118: "d334053cf974c461", 119: "2008b49f111b2812",
    120: "38e5ba635ad0e00b", 121: "3ae51f562b32bba8", 122: "c8991ecceb078562", 123: "60b269aa23bc0cd6"}


@pytest.mark.parametrize("seed", S.SEEDS2)
def test_second_generation_seeds_are_what_they_were(seed):
    q = S.generate(seed)
    assert hashlib.sha256(repr((repr(q.log), q.obs, q.meta)).encode()).hexdigest()[:16] == SEED2_DIGESTS[seed]
    assert not any(op["op"] in S.GEN3_MUTATING + S.GEN3_READ_ONLY for op in q.log)


# ---- the second generation: the map queries and transform_poses ------------------------------------------------------------
def _total(obs):
    return sum(counters[2] for _, counters in obs.values())


@pytest.mark.parametrize("seed", S.SEEDS2)
def test_second_generation_caps_replay_and_scene(seed):
    q = S.generate(seed)
    assert 8 <= len(q.log) <= 24, q.printed()
    assert len(q.log) == len(q.obs) == len(q.meta) == len(q.ident)
    assert q.rejected <= 0.25 * q.draws, (q.rejected, q.draws)
    m = S.Model(q.container)
    for i, op in enumerate(q.log):
        before = (m.observe(), m.pooled) if op["op"] == "transform_poses_refused" else None
        m.apply(op)
        assert m.observe() == q.obs[i], f"step {i}\n{q.printed(i)}"
        assert m.pooled == q.meta[i]["pooled"]
        if before is not None:      # a refused call changes nothing and invalidates nothing
            assert (q.obs[i], q.meta[i]["pooled"]) == before and q.meta[i]["pooled"] == q.meta[i - 1]["pooled"]
        ident = m.identity()
        assert (ident is None) == (q.ident[i] is None)
        for p in ident or ():
            assert np.array_equal(ident[p][0], q.ident[i][p][0]) and np.array_equal(ident[p][1], q.ident[i][p][1])
            # the identity: strictly ascending row numbers of the cloud as first inserted, one per surviving row
            assert len(ident[p][0]) == q.obs[i][p][1][2] and np.all(np.diff(ident[p][0]) > 0)
            assert len(ident[p][0]) == 0 or 0 <= ident[p][0][0] and ident[p][0][-1] < m.n_inserted[p]
        if op["op"] == "transform_poses":      # no scheme remains, and a subdivide is the next mutating operation
            assert not m.internal_nodes() and all(c[0] == len(t) for t, c in q.obs[i].values() if q.container["kind"] != "grid")
            nxt = next(o["op"] for o in q.log[i + 1:] if o["op"] in S.ALL_MUTATING)
            assert nxt in S.SUBDIVIDES, q.printed()
    assert q.flags["depth2"] and q.flags["emptied"], q.printed()
    assert q.closest > 1e-9
    for p, (table, counters) in q.obs[-1].items():
        assert counters[1] == len(table) and counters[2] == sum(d[0] for _, d in table)
    shifted = [i for i, op in enumerate(q.log) if op.get("fn") == "shift_z"]
    if shifted:      # only as the last mutating operation
        assert not any(op["op"] in S.ALL_MUTATING for op in q.log[shifted[0] + 1:])


def test_second_generation_covers_kinds_containers_and_transitions():
    kinds, trans, containers = collections.Counter(), collections.Counter(), collections.Counter()
    tp = collections.Counter()
    utm = after_removal = async_mask = 0
    worst = 0.0
    for seed in S.SEEDS2:
        q = S.generate(seed)
        kinds.update(op["op"] for op in q.log)
        kinds.update("raycast_" + op["surface"] for op in q.log if op["op"] == "raycast")
        trans.update(S.transitions2(q.log))
        containers[q.container["kind"]] += 1
        worst = max(worst, q.rejected / q.draws)
        moves = [i for i, op in enumerate(q.log) if op["op"] == "transform_poses"]
        for i in moves:
            tp[q.container["kind"]] += 1
            tp["subset" if q.log[i]["poses"] is not None else "all"] += 1
        utm += bool(moves) and q.container["utm"]
        removers = S.FILTERS + ("apply_mask", "ransac", "map_select")
        after_removal += any(q.log[k]["op"] in removers and _total(q.obs[k]) < _total(q.obs[k - 1])
                             for i in moves for k in range(1, i))
        async_mask += any(a["op"] == "ransac" and b["op"] == "raycast" for a, b in zip(q.log, q.log[1:]))
    print("kinds:", dict(kinds))
    print("transitions:", dict(trans))
    print("containers:", dict(containers), "transform_poses:", dict(tp), "on UTM clouds:", utm,
          "after rows were removed:", after_removal, "worst rejection share:", worst)
    for k in S.NEW_MUTATING + S.NEW_READ_ONLY + ("raycast_cube", "raycast_plane"):
        assert kinds[k] >= 5, (k, kinds[k])
    for t in S.TRANSITIONS2:
        assert trans[t] >= 2, (t, trans[t])
    for c in ("grid", "manager", "octree"):
        assert containers[c] >= 4, containers
    for k in ("grid", "manager", "subset", "all"):
        assert tp[k] >= 2, tp
    assert utm >= 2 and after_removal >= 3 and async_mask >= 2


# ---- the third generation: moved inserts, carve, remove_poses -------------------------------------------------------------
@pytest.mark.parametrize("seed", S.SEEDS3)
def test_third_generation_caps_replay_and_scene(seed):
    q = S.generate(seed)
    assert 8 <= len(q.log) <= 28, q.printed()
    assert len(q.log) == len(q.obs) == len(q.meta) == len(q.ident)
    assert q.rejected <= 0.25 * q.draws, (q.rejected, q.draws)
    m = S.Model(q.container)
    for i, op in enumerate(q.log):
        before = (m.observe(), m.pooled, list(m.poses)) if op["op"] in S.REFUSED else None
        held, had = {p: m.counters(p)[2] for p in m.poses}, dict(m.n_inserted)
        m.apply(op)
        assert m.observe() == q.obs[i], f"step {i}\n{q.printed(i)}"
        assert m.pooled == q.meta[i]["pooled"] and m.returned == q.meta[i].get("returns")
        assert list(q.obs[i]) == m.poses
        if before is not None:      # a refused call changes nothing and invalidates nothing
            assert (q.obs[i], q.meta[i]["pooled"], m.poses) == before and q.meta[i]["pooled"] == q.meta[i - 1]["pooled"]
        ident = m.identity()
        assert (ident is None) == (q.ident[i] is None)
        for p in ident or ():
            assert np.array_equal(ident[p][0], q.ident[i][p][0]) and np.array_equal(ident[p][1], q.ident[i][p][1])
            assert len(ident[p][0]) == q.obs[i][p][1][2] and np.all(np.diff(ident[p][0]) > 0)
            assert len(ident[p][0]) == 0 or 0 <= ident[p][0][0] and ident[p][0][-1] < m.n_inserted[p]
        if op["op"] in S.MOVED:      # the rows are numbered as in the cloud as given, all of them
            given = len(S.make_cloud(op["cloud"]))
            assert m.n_inserted[op["pose"]] - had.get(op["pose"], 0) == given
            if ident is not None and op["op"] == "insert_moved":
                assert np.array_equal(ident[op["pose"]][0], np.arange(given))
        if op["op"] in ("carve", "remove_poses"):      # the booked return value is the rows that left; the scheme stays
            now = {p: m.counters(p)[2] for p in m.poses}
            assert m.returned == sum(held.values()) - sum(now.values()) >= 0
            if op["op"] == "remove_poses":
                assert all(now[p] == held[p] for p in now) and set(held) - set(now) == set(op["poses"]) and now
            else:
                assert all(now[p] == held[p] for p in now if op["poses"] is not None and p not in op["poses"])
        if op["op"] == "store_size":
            assert m.returned == (sum(m.n_inserted[p] for p in m.poses), sum(c[2] for _, c in q.obs[i].values()), len(m.poses))
        if op["op"] == "transform_poses":
            nxt = next(o["op"] for o in q.log[i + 1:] if o["op"] in S.ALL_MUTATING)
            assert nxt in S.SUBDIVIDES, q.printed()
        if op["op"] == "ransac":      # pose numbers 0 .. n-1, whatever their slots
            assert sorted(m.poses) == list(range(len(m.poses)))
    assert q.flags["depth2"] and q.flags["emptied"], q.printed()
    assert q.closest > 1e-9
    for p, (table, counters) in q.obs[-1].items():
        assert counters[1] == len(table) and counters[2] == sum(d[0] for _, d in table)
    assert not any(op.get("fn") == "shift_z" for op in q.log)      # (carve and remove_poses are not drawable after it)


def test_third_generation_covers_kinds_containers_and_transitions():
    kinds, trans, containers, c = collections.Counter(), collections.Counter(), collections.Counter(), collections.Counter()
    worst = 0.0
    for seed in S.SEEDS3:
        q = S.generate(seed)
        kinds.update(op["op"] for op in q.log)
        trans.update(S.transitions3(q.log))
        containers[q.container["kind"]] += 1
        worst = max(worst, q.rejected / q.draws)
        slots = []      # the pose numbers in slot order, before every operation
        for i, op in enumerate(q.log):
            k = op["op"]
            if k == "carve":
                c["carve fused" if op["fused"] else "carve unfused"] += 1
                c["carve of a pose subset"] += op["poses"] is not None
                c["carve that removes rows"] += q.meta[i]["returns"] > 0
                c["carve that removes nothing"] += q.meta[i]["returns"] == 0
                c["carve with earlier evidence"] += op.get("evidence_from") is not None
            if k == "remove_poses":
                removers = S.FILTERS + ("apply_mask", "ransac", "map_select", "carve")
                c["removal after rows left"] += any(q.log[j]["op"] in removers and _total(q.obs[j]) < _total(q.obs[j - 1])
                                                    for j in range(1, i))
                c["removal on a UTM grid"] += bool(q.container["utm"])
                c["removal of the first slot"] += slots[0] in op["poses"]
                c["removal of a middle slot"] += any(p in op["poses"] for p in slots[1:-1])
                c["removal of the last slot"] += slots[-1] in op["poses"]
                c["removal of a pose named twice"] += len(set(op["poses"])) < len(op["poses"])
                c["removal on a " + q.container["kind"]] += 1
            if k in S.MOVED:
                c["moved " + op["cloud"]["form"]] += 1
                c["moved " + op["matrix"]] += 1
                c["moved into an empty map"] += i == 0
                if "motions" in op:
                    c[f"piecewise M={len(op['motions'])}"] += 1
                    c["segment " + op["segment_dtype"]] += 1
                else:
                    c["one motion"] += 1
            if k == "insert" and i and any(op["pose"] in o["poses"] for o in q.log[:i] if o["op"] == "remove_poses"):
                c["insert of a freed number"] += 1
            slots = list(q.obs[i])
    print("kinds:", dict(kinds))
    print("transitions:", dict(trans))
    print("containers:", dict(containers), "worst rejection share:", worst)
    print("cases:", dict(c))
    for k in S.GEN3_MUTATING + S.GEN3_READ_ONLY:
        assert kinds[k] >= 5, (k, kinds[k])
    for t in S.TRANSITIONS3:
        assert trans[t] >= 2, (t, trans[t])
    for k in ("grid", "manager", "octree"):
        assert containers[k] >= 4, containers
    assert c["carve fused"] >= 3 and c["carve unfused"] >= 3 and c["carve of a pose subset"] >= 2
    assert c["carve that removes rows"] >= 6
    assert c["removal after rows left"] >= 3 and c["removal on a UTM grid"] >= 2
    assert c["removal of the first slot"] >= 2 and c["removal of a middle slot"] >= 2
    assert c["piecewise M=1024"] >= 2
    for k in ("segment int32", "segment uint16", "segment int64", "moved device32", "moved device64"):
        assert c[k] >= 2, (k, c)


# the same digests for the third generation, computed in a worktree of the commit before the fourth generation was added
SEED3_DIGESTS = {
    200: "26b052883fef3114", 201: "dab8d33b4ba1f1b2", 202: "08d7aa7cffd10a8d", 203: "d19ac878e207a6a7",
    204: "820be7f91144571b", 205: "53463f2498a0eaa9", 206: "f5c16ace3357ed44", 207: "07624a56439b2873",
    208: "a934d4c87710d077", 209: "edebd86e56ad4c7b", 210: "25179ca4dcc2ea33", 211: "657cd45c17dfbe62",
    212: "d6823cbf68bf40a3", 213: "16c38240a762b22b", 214: "c9d777fef1dc1cae", 215: "112a4be5c83ae916",
    216: "87b6b9052019ff58", 217: "b7aee4c3226a5b1a", 218: "12e79ad4736192cd", 219: "3c76649e443f915b",
    220: "6555fdfb9ec8a5b6", 221: "cd27386ab5d4c21e", 222: "7e645563a83595b9", 223: "518a5446f3e06d98"}


@pytest.mark.parametrize("seed", S.SEEDS3)
def test_third_generation_seeds_are_what_they_were(seed):
    q = S.generate(seed)
    assert hashlib.sha256(repr((repr(q.log), q.obs, q.meta)).encode()).hexdigest()[:16] == SEED3_DIGESTS[seed]
    assert not any(op["op"] in S.GEN4_MUTATING + S.GEN4_READ_ONLY for op in q.log)


# ---- the fourth generation: prune, remove_sparse, radius_count, the nearest-point registrations --------------------------
def _same(a, b):
    """Equality of two booked return values (a radius_count books an array)."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return a is not None and b is not None and np.array_equal(a, b)
    return a == b


@pytest.mark.parametrize("seed", S.SEEDS4)
def test_fourth_generation_caps_replay_and_scene(seed):
    q = S.generate(seed)
    assert 8 <= len(q.log) <= 28, q.printed()
    assert len(q.log) == len(q.obs) == len(q.meta) == len(q.ident)
    assert q.rejected <= 0.25 * q.draws, (q.rejected, q.draws)
    m = S.Model(q.container)
    for i, op in enumerate(q.log):
        k = op["op"]
        before = (m.observe(), m.pooled, list(m.poses)) if k in S.REFUSED + S.GEN4_READ_ONLY else None
        held = {p: m.counters(p) for p in m.poses}
        rows = {p: sorted(map(bytes, m.pose_rows(p))) for p in m.poses} if k in ("prune", "remove_sparse") else None
        m.apply(op)
        assert m.observe() == q.obs[i], f"step {i}\n{q.printed(i)}"
        assert m.pooled == q.meta[i]["pooled"] and _same(m.returned, q.meta[i].get("returns"))
        assert list(q.obs[i]) == m.poses
        if before is not None and k in S.REFUSED:      # a refused call changes nothing and invalidates nothing
            assert (q.obs[i], q.meta[i]["pooled"], m.poses) == before and q.meta[i]["pooled"] == q.meta[i - 1]["pooled"]
        if before is not None and k in S.GEN4_READ_ONLY:      # the new reads change nothing; only the plane form makes a table
            assert (q.obs[i], m.poses) == (before[0], before[2])
            assert q.meta[i]["pooled"] == (before[1] or k == "nearest_plane_registration_system")
        ident = m.identity()
        assert (ident is None) == (q.ident[i] is None)
        for p in ident or ():
            assert np.array_equal(ident[p][0], q.ident[i][p][0]) and np.array_equal(ident[p][1], q.ident[i][p][1])
            assert len(ident[p][0]) == q.obs[i][p][1][2] and np.all(np.diff(ident[p][0]) > 0)
            assert len(ident[p][0]) == 0 or 0 <= ident[p][0][0] and ident[p][0][-1] < m.n_inserted[p]
        now = {p: m.counters(p) for p in m.poses}
        if k == "prune":
            # every pose reads back the same rows and the same non-empty leaves; the five numbers add up; a prune that
            # finds nothing leaves the pooled table standing, any other one invalidates it
            n_nodes, n_voxels, nodes_dropped, voxels_dropped, collapsed = m.returned
            assert {p: sorted(map(bytes, m.pose_rows(p))) for p in m.poses} == rows
            assert all(now[p][1:] == held[p][1:] and now[p][0] <= held[p][0] for p in now)
            assert [t for t, _ in q.obs[i].values()] == [t for t, _ in q.obs[i - 1].values()]
            assert n_nodes == sum(t.root.n_nodes() for t in m.scheme_trees()) and n_voxels == len(m.scheme_trees())
            assert (nodes_dropped > 0) == (voxels_dropped + collapsed > 0) and nodes_dropped >= voxels_dropped + 8 * collapsed
            assert q.meta[i]["pooled"] == (q.meta[i - 1]["pooled"] and nodes_dropped == 0)
            assert nodes_dropped == 0 or q.meta[i]["stats"] == "nan"
            assert nodes_dropped > 0 or q.meta[i]["stats"] == q.meta[i - 1]["stats"]
            assert m._prune(None, dry=True) == {"voxels": 0, "collapsed": 0, "outer": False, "bare": False}
        if k == "remove_sparse":      # the booked return value is the rows that left, all of them from the tested poses
            assert m.returned == sum(c[2] for c in held.values()) - sum(c[2] for c in now.values()) >= 0
            assert all(now[p][2] == held[p][2] for p in now if op["poses"] is not None and p not in op["poses"])
            assert all(set(sorted(map(bytes, m.pose_rows(p)))) <= set(rows[p]) for p in m.poses)
            assert not q.meta[i]["pooled"]
        if k == "radius_count":
            cnt = m.returned
            assert cnt.dtype == np.int32 and len(cnt) == op["n"] + 6 and not cnt[-6:-1].any() and cnt.min() >= 0
            assert op["max_count"] is None or cnt.max() <= op["max_count"]
        if k == "transform_poses":
            assert not m.collapsed and not m.dropped      # (the map is rebuilt: the collapsed-node guard is lifted)
            nxt = next(o["op"] for o in q.log[i + 1:] if o["op"] in S.ALL_MUTATING)
            assert nxt in S.SUBDIVIDES, q.printed()
        if k == "ransac":
            assert sorted(m.poses) == list(range(len(m.poses)))
    assert q.flags["depth2"] and q.flags["emptied"], q.printed()
    assert q.closest > 1e-9
    for p, (table, counters) in q.obs[-1].items():
        assert counters[1] == len(table) and counters[2] == sum(d[0] for _, d in table)
    assert not any(op.get("fn") == "shift_z" for op in q.log)


def test_fourth_generation_covers_kinds_containers_and_transitions():
    kinds, trans, containers, c = collections.Counter(), collections.Counter(), collections.Counter(), collections.Counter()
    worst, f32, utm = 0.0, 0, 0
    for seed in S.SEEDS4:
        q = S.generate(seed)
        kinds.update(op["op"] for op in q.log)
        trans.update(S.transitions4(q.log, q.meta))
        kind = q.container["kind"]
        containers[kind] += 1
        worst = max(worst, q.rejected / q.draws)
        f32 += any(op.get("cloud", {}).get("form") in ("f32", "device32") for op in q.log)
        utm += bool(q.container["utm"])
        for i, op in enumerate(q.log):
            k, facts = op["op"], q.meta[i].get("facts")
            if k == "prune":
                c["prune that drops a voxel"] += facts["voxels"] > 0
                c["prune that collapses a node"] += facts["collapsed"] > 0
                c["prune that finds nothing"] += facts["voxels"] + facts["collapsed"] == 0
                c["prune that drops an outermost voxel"] += facts["outer"]
                c["prune on a " + kind] += 1
                c["manager emptied to its bare root"] += kind == "manager" and facts["bare"]
            if k in ("insert", "insert_moved") and facts is not None:
                c["insert that re-creates a dropped voxel"] += facts["recreated"] > 0
            if k == "remove_sparse":
                c["remove_sparse that removes rows"] += facts["removed"] > 0
                c["remove_sparse that removes nothing"] += facts["removed"] == 0
                c["remove_sparse of a pose subset"] += op["poses"] is not None
                c["remove_sparse among a pose subset"] += op["among"] is not None
            if k == "radius_count":
                c[f"radius_count capped at {op['max_count']}"] += 1
                c["radius_count with a saturated query"] += facts["saturated"] > 0
            if k in ("point_registration_system", "nearest_plane_registration_system"):
                name = "point" if k == "point_registration_system" else "plane"
                c[name + " registration with Huber weights"] += op["huber_delta"] is not None
                c[name + " registration with a given origin"] += op["origin"] is not None
                c[name + " registration that uses no point"] += facts["n_used"] == 0
                c[name + " registration that uses some points"] += 0 < facts["n_used"] < facts["n"]
                if name == "plane":
                    c["plane registration with a match in a leaf without a plane"] += facts["no_plane"] > 0
            if k == "carve" and op.get("remapped"):
                c["carve with evidence carried over a prune"] += 1
    print("kinds:", dict(kinds))
    print("transitions:", dict(trans))
    print("containers:", dict(containers), "f32 / device32 seeds:", f32, "UTM seeds:", utm, "worst rejection share:", worst)
    print("cases:", dict(c))
    for k in S.GEN4_MUTATING + S.GEN4_READ_ONLY:
        assert kinds[k] >= 5, (k, kinds[k])
    for t in S.TRANSITIONS4:
        assert trans[t] >= 2, (t, trans[t])
    for k in ("grid", "manager", "octree"):
        assert containers[k] >= 4, containers
    assert f32 >= 3 and utm >= 2
    assert c["prune that drops a voxel"] >= 3 and c["prune that collapses a node"] >= 4 and c["prune that finds nothing"] >= 2
    assert c["prune on a manager"] >= 2 and c["prune on a octree"] >= 2 and c["manager emptied to its bare root"] >= 1
    assert c["remove_sparse that removes rows"] >= 6 and c["remove_sparse that removes nothing"] >= 1
    assert c["remove_sparse of a pose subset"] >= 2 and c["remove_sparse among a pose subset"] >= 2
    for cap in (None, 1, 3, 7):
        assert c[f"radius_count capped at {cap}"] >= 2, (cap, c)
    assert c["radius_count with a saturated query"] >= 3
    for name in ("point", "plane"):
        assert c[name + " registration with Huber weights"] >= 2 and c[name + " registration with a given origin"] >= 2, c
        assert c[name + " registration that uses no point"] >= 1 and c[name + " registration that uses some points"] >= 3, c
    assert c["plane registration with a match in a leaf without a plane"] >= 2


def test_collapsed_node_guard_rejects_a_refilled_node():
    """No seed draws an insert once a prune has collapsed a node, so the guard is held here: after seed 303's log (a
    manager whose prunes collapsed nodes) a cloud that fills the cube is Rejected; a cloud confined to a leaf that was
    never collapsed is taken; and a transform_poses lifts the guard."""
    q = S.generate(303)
    m = S.Model.replay(q.container, q.log)
    assert m.kind == "manager" and m.collapsed and any(q.meta[i]["facts"]["collapsed"] for i, op in enumerate(q.log)
                                                        if op["op"] == "prune")
    pose = next(p for p in S.MANAGER_POSES if p not in m.poses)
    cloud = {"seed": 999001, "n": 4000, "edge": S.cloud_edge(q.container), "utm": False, "form": "f64", "cube": True}
    with pytest.raises(S.Rejected, match="collapsed"):
        m.apply({"op": "insert", "pose": pose, "cloud": cloud})
    # the rejected draw leaves the model unusable, as in the generator: a fresh replay
    m = S.Model.replay(q.container, q.log)
    full = next(v for t in m.trees_of(m.poses[0]) for v in t.leaves(True))
    key = (None, (np.asarray(full.corner, dtype=np.float64) + 0.0).tobytes(), float(full.edge))
    assert key not in m.collapsed
    inside = {**cloud, "n": 2000}
    rows = S.model_cloud(inside)
    lo, hi = rows.min(axis=0), rows.max(axis=0)
    shrunk = np.asarray(full.corner, dtype=np.float64) + (rows - lo) / (hi - lo) * float(full.edge) * 0.999
    tree = m.trees_of(m.poses[0])[0]
    start = len(tree.points)
    m.o.insert_points(m.poses[0], shrunk)      # (an extend by hand: every row into the one occupied leaf)
    assert len(tree.points) == start + len(shrunk)
    m._guard_collapsed()
    identity = {"xi": [0.0] * 6, "origin": [0.0, 0.0, 0.0]}
    m = S.Model.replay(q.container, q.log)
    m.apply({"op": "transform_poses", "poses": None, "motions": [identity] * len(m.poses)})
    assert not m.collapsed and not m.dropped


_Leaf = S._Leaf


@pytest.mark.parametrize("seed", [0, 7, 106, 115, 203, 214, 303, 302])
def test_numpy_specifications_answer_the_models_tables(seed):
    """locate_np, pooled_leaf_statistics_np, point_to_plane_np (through HostMap, which rebuilds the node table from
    the leaves) and leaf_statistics_np on the model at the end of a sequence; at the end of two sequences of the second
    generation (115 contains a transform_poses) nearest_np, raycast_np, plane_segments_np, registration_system_np and
    adjustment_system_np too; at the end of two of the third (203: a manager after carve and remove_poses, 214: a UTM
    grid after two removals) ray_evidence_np as well; at the end of two of the fourth (303: a manager after
    remove_sparse and prune, 302: a UTM grid after a prune that dropped voxels) radius_count_np, sparse_keep_np and
    the two nearest-point registration systems."""
    q = S.generate(seed)
    m = S.Model.replay(q.container, q.log)
    leaves = {p: [_Leaf(c, e, r) for c, e, r in m.leaf_rows(p, non_empty=False)] for p in m.poses}
    if m.kind == "grid":
        keys = sorted(k for k, mg in m.o.managers.items() if mg.octrees)      # (not the voxels only removed poses were in)
        hm = HostMap(0, float(m.c["edge"]), [(np.array(k, dtype=np.float64), float(m.c["edge"])) for k in keys], leaves)
    else:
        hm = HostMap(1, float(m.c["edge"]), [(np.array(m.c["corner"]), float(m.c["edge"]))], leaves)
    stored = np.vstack([m.pose_rows(p) for p in m.poses])
    assert len(stored) > 100
    node = hm.locate(stored)
    if not m.displaced:
        assert np.all(node >= 0) and np.all(hm.nodes["first_child"][node] < 0)
    Q = np.concatenate([stored[::5] + 0.003, [[np.nan, 0.0, 0.0], [1e300, 0.0, 0.0]]])
    res = hm.point_to_plane(Q, None, 8, None)
    assert np.all(res.row[-2:] == -1) and (res.row >= 0).any()
    assert int(res.planes.count.sum()) == len(stored)
    assert np.all(np.isfinite(res.distance[res.row >= 0])) and np.all(np.isnan(res.distance[res.row < 0]))
    for p in m.poses:
        rows = [r for _, _, r in m.leaf_rows(p)]
        st = leaf_statistics_np(rows)
        assert st.count.tolist() == [len(r) for r in rows] and np.all(np.isfinite(st.covariance))
    if seed < S.SEEDS2[0]:
        return
    assert seed >= S.SEEDS3[0] or (seed == 115) == any(op["op"] == "transform_poses" for op in q.log)
    e = S.cloud_edge(m.c)
    nn = hm.nearest(stored[::20] + 0.003 * e, 3, max_distance=0.5 * e)
    assert (nn.count > 0).all() and np.all(nn.distance2[:, 0] <= 3 * (0.003 * e) ** 2 * (1 + 1e-12))
    with np.errstate(invalid="ignore"):      # (inf - inf between two pads)
        assert np.all(np.diff(nn.distance2, axis=1)[np.isfinite(nn.distance2[:, 1:])] >= 0)
    own = hm.nearest(stored[::20], 1, max_distance=0.05 * e)
    sizes = {p: len(m.pose_rows(p)) for p in m.poses}
    assert np.all(own.distance2[:, 0] == 0.0) and all(0 <= i < sizes[p] for p, i in zip(own.pose[:, 0], own.index[:, 0]))
    # rays from outside towards stored points hit an occupied leaf no later than the leaf of the point they aim at
    aim = stored[::20]
    O = aim + np.array([0.0, 0.0, 6.0 * e])
    for surface in ("cube", "plane"):
        hits = hm.raycast(O, aim - O, 8.0 * e, surface=surface)
        assert hits.node.shape == (len(O),) and np.all(hits.t[hits.hit] <= 8.0 * e) and np.all(np.isinf(hits.t[~hits.hit]))
        assert np.all(hm.nodes["first_child"][hits.node[hits.hit]] < 0) and np.all((hits.row >= 0) == (hits.hit & (surface == "plane")))
    cube = hm.raycast(O, aim - O, 8.0 * e)
    assert cube.hit.all() and np.all(cube.t <= 6.0 * e)
    assert hm.raycast(O, np.zeros_like(O), 8.0 * e).hit.sum() == 0
    seg = hm.plane_segments(None, 8, 1e-3 * e ** 2)
    assert len(seg.label) == len(seg.planes) and seg.neighbour.shape == (len(seg.planes), 6)
    assert seg.segments.n_leaves.sum() == (seg.label >= 0).sum() and seg.label.max() + 1 == len(seg.segments.count)
    p0 = m.poses[0]
    scan = m.pose_rows(p0)[:800]
    rs = hm.registration_system(scan, None, None, per_point=True)
    assert rs.n_located == len(scan) and 0 < rs.n_used <= rs.n_located and np.array_equal(rs.H, rs.H.T)
    assert np.array_equal(rs.node, hm.locate(scan)) and np.all(np.isfinite(rs.residual[rs.row >= 0]))
    if m.kind != "octree":
        ad = hm.adjustment_system(None, None, leaves=True)
        assert ad.H.shape == (len(m.poses), 6, 6) and np.all(np.isfinite(ad.H)) and ad.n_leaves[0] == len(ad.leaves)
        assert int(ad.blocks.count.sum()) == len(stored)
    if seed < S.SEEDS3[0]:
        return
    if seed < S.SEEDS4[0]:
        assert sum(op["op"] == "remove_poses" for op in q.log) >= (2 if seed == 214 else 1)
    # rays from outside that measure exactly the distance to the stored point they aim at: every one of them ends in the
    # leaf of its point, none ends in an inner node, and the hits are at least the live rays that reach the map
    r = np.sqrt(((aim - O) ** 2).sum(axis=1))
    ev = hm.ray_evidence(O, aim - O, r, 0.05 * e)
    leaf = hm.locate(aim)
    assert len(ev) == len(hm.nodes["edge"]) and ev.hits.dtype == ev.through.dtype == np.uint32
    assert np.all(ev.hits >= np.bincount(leaf, minlength=len(ev))) and int(ev.hits.sum()) >= len(aim)
    inner = hm.nodes["first_child"] >= 0
    assert not ev.hits[inner].any() and not ev.through[inner].any()
    silent = hm.ray_evidence(O, aim - O, r, 0.05 * e, returned=np.zeros(len(aim), dtype=bool))
    assert not silent.hits.any() and np.all(silent.through >= ev.through)
    assert not np.any(ev.free(1, 0) & (np.bincount(leaf, minlength=len(ev)) > 0))      # carve would keep what was hit
    if seed < S.SEEDS4[0]:
        return
    prunes = [q.meta[i]["facts"] for i, op in enumerate(q.log) if op["op"] == "prune"]
    assert prunes and any(op["op"] == "remove_sparse" for op in q.log)
    assert seed != 302 or (q.container["utm"] and any(f["voxels"] > 0 for f in prunes))
    # every stored point counts itself at a tiny radius; a cap only cuts the count
    some = stored[::20]
    assert np.all(hm.radius_count(some, 1e-6 * e, max_count=1) == 1)
    free, capped = hm.radius_count(some, 0.2 * e), hm.radius_count(some, 0.2 * e, max_count=3)
    assert free.dtype == np.int32 and np.all(free >= capped) and np.array_equal(capped, np.minimum(free, 3))
    # the decisions of remove_sparse: one per stored row - and the model's tiled evaluation is the rule itself
    decided = hm.remove_sparse(0.1 * e, 2)
    assert [p for p, _ in decided] == m.poses and all(len(k) == len(m.pose_rows(p)) for p, k in decided)
    tiled = S.sparse_keep_tiled({p: m.pose_rows(p) for p in m.poses}, m.poses, m.poses, 0.1 * e, 2)
    assert all(np.array_equal(k, tiled[p]) for p, k in decided) and any((~k).any() for _, k in decided)
    part = m.poses[:1]
    other = [(p, k) for p, k in hm.remove_sparse(0.1 * e, 2, pose_numbers=m.poses[-1:], among=part)]
    tiled = S.sparse_keep_tiled({p: m.pose_rows(p) for p in m.poses}, m.poses[-1:], part, 0.1 * e, 2)
    assert [p for p, _ in other] == m.poses[-1:] and np.array_equal(other[0][1], tiled[m.poses[-1]])
    # stored rows as a scan at the identity: every point is its own nearest point
    scan = stored[::15][:600]
    ps = hm.point_registration_system(scan, None, max_distance=0.05 * e)
    assert ps.cost == 0 and ps.n_used == ps.n_located == len(scan)
    ns = hm.nearest_plane_registration_system(scan, None, max_distance=0.05 * e, per_point=True)
    assert ns.n_used <= ns.n_located == len(scan) and np.array_equal(ns.node, hm.locate(scan))
