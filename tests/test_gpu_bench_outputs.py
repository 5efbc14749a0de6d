"""A plain `bench.py` run - no --full - with --dump-outputs: it times exactly --steps steps, prints the contract's
line and nothing measured beside the headline, and writes what its last timed step computed.  Two runs with the same
arguments write the same arrays, and those arrays are the oracle's leaf table for the same cloud.

bench.py runs in a child of the GPU-free fork server (tests/conftest.py): a process that has touched the GPU never
forks or execs."""

import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = ("leaf_index", "leaf_corner", "leaf_edge", "leaf_points", "point_index", "point_leaf")


def _run_bench(cmd, out_path, err_path, conn):
    """Runs in a child of the GPU-free fork server: a process that has not touched the GPU may exec."""
    import subprocess

    with open(out_path, "w") as out, open(err_path, "w") as err:
        rc = subprocess.call(cmd, stdout=out, stderr=err, cwd=ROOT)
    conn.send(rc)


def _bench(mp, args, tmp_path, tag):
    line, err = str(tmp_path / f"{tag}.json"), str(tmp_path / f"{tag}.err")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--detail", str(tmp_path / f"{tag}_detail.json")]
    parent, child = mp.Pipe()
    p = mp.Process(target=_run_bench, args=(cmd, line, err, child), daemon=True)
    p.start()
    try:
        assert parent.poll(300), "bench.py did not finish"
        rc = parent.recv()
    finally:
        p.join(timeout=30)
        if p.is_alive():
            p.kill()
    assert rc == 0, open(err).read()[-3000:]
    lines = [ln for ln in open(line).read().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_times_its_steps_and_dumps_the_last_step(tmp_path):
    from tests import conftest

    mp = conftest.rank_spawner()
    if mp is None:
        pytest.skip("no fork server (it must be started before the GPU is touched: run through pytest's conftest)")
    n, steps, dims = 300_000, 5, (8, 8, 8)
    args = ["--steps", str(steps), "--warmup", "1", "--points", str(n), "--scene"] + [str(d) for d in dims]
    dumps = [tmp_path / "a", tmp_path / "b"]
    lines = [_bench(mp, args + ["--dump-outputs", str(d)], tmp_path, d.name) for d in dumps]

    for d in lines:
        assert d["metric"] == "Mpoints/s insert+subdivide+RANSAC" and d["unit"] == "Mpoints/s"
        assert d["higher_is_better"] is True and d["dtype"] == "f64"
        assert d["steps"] == steps and d["warmup"] == 1 and d["ms_per_step"] > 0
        assert abs(d["value"] / (n / d["ms_per_step"] / 1e3) - 1) < 1e-4
        for k in ("roofline", "roofline_valu", "roofline_build", "cpu_baseline", "launches_per_step"):
            assert k not in d, k
    detail = json.load(open(tmp_path / "a_detail.json"))
    assert "secondary" not in detail and "kernels" not in detail

    got = []
    for d in dumps:
        arrays = {name: np.load(d / f"{name}.npy") for name in DUMPED}
        assert sorted(os.listdir(d)) == sorted(f"{name}.npy" for name in DUMPED)
        assert all(a.dtype == np.float64 for a in arrays.values())
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
        got.append(arrays)
    for name in DUMPED:   # same arguments, same outputs
        assert np.array_equal(got[0][name], got[1][name]), name

    # the oracle on the cloud of the last timed step (bench.Workload.make_cloud: the timed loop rotates over three
    # clouds from cloud 0; cloud 2 is a third draw moved by one voxel along x)
    from octreelib_amd import synthetic
    from oracle import octree_np as onp
    from oracle import ransac_np as rnp

    cloud = (steps - 1) % 3
    pts = synthetic.planar_cloud(n, dims, seed=1, stream=1_000_000 * cloud)
    if cloud == 2:
        pts[:, 0] += 1.0
    og = onp.OGrid(1)
    og.insert_points(0, pts)
    og.subdivide(64)
    rows = og.leaf_table(0)
    np.random.seed(0)
    table = np.random.random((1024, 6))
    mask = rnp.evaluate(np.vstack([pts[i] for _, _, i in rows]), np.array([len(i) for _, _, i in rows], np.int32),
                        table, 0.01)
    og.apply_mask(0, mask)
    rows = og.leaf_table(0)
    point_leaf = np.full(n, -1.0)
    for j, (_, _, idx) in enumerate(rows):
        point_leaf[idx] = j

    a = got[0]
    assert np.array_equal(a["leaf_index"], np.arange(len(rows)))
    assert np.array_equal(a["leaf_corner"], np.array([np.asarray(c, np.float64) for c, _, _ in rows]))
    assert np.array_equal(a["leaf_edge"], np.array([e for _, e, _ in rows], np.float64))
    assert np.array_equal(a["leaf_points"], np.array([len(i) for _, _, i in rows], np.float64))
    assert np.array_equal(a["point_index"], np.arange(n))
    assert np.array_equal(a["point_leaf"], point_leaf)
