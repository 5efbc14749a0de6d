"""The operation-sequence generator and its oracle model, alone (tests/_opseq.py; the device side is
tests/test_gpu_opseq.py): the caps the seed set must meet, the replay that forks a model, the model-side sanity of the
scenes, and the NumPy specifications of the queries on the model's own tables."""

import collections

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


class _Leaf:
    def __init__(self, corner, edge, rows):
        self.corner_min, self.edge_length, self._rows = corner, edge, rows

    def get_points(self):
        return self._rows


@pytest.mark.parametrize("seed", [0, 7])
def test_numpy_specifications_answer_the_models_tables(seed):
    """locate_np, pooled_leaf_statistics_np, point_to_plane_np (through HostMap, which rebuilds the node table from
    the leaves) and leaf_statistics_np on the model at the end of a sequence."""
    q = S.generate(seed)
    m = S.Model.replay(q.container, q.log)
    leaves = {p: [_Leaf(c, e, r) for c, e, r in m.leaf_rows(p, non_empty=False)] for p in m.poses}
    if m.kind == "grid":
        keys = sorted(m.o.managers)
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
