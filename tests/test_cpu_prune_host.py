"""The index arithmetic of octl_forest_prune (octreelib_amd/csrc/prune_map.h: the mark climb, the keep rule, the node
row and the containing map, the level-range rewrite - the code the kernels of prune.hip run) compiled for the CPU
alone, with AddressSanitizer and UBSan, as the stand-alone program tests/host/prune_host.cpp, and compared with
query.prune_np.  No GPU and nothing loaded into Python: the program gets heap arrays of exactly their size from a
file.  This test is about that program: it compiles it once (a few seconds) and starts it once per case and tile
size."""

import os
import subprocess

import numpy as np
import pytest

from octreelib_amd.query import prune_np
from tests._prune_cases import CASES, random_forest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("prune_host")
    exe = os.path.join(str(d), "prune_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "octreelib_amd", "csrc"), os.path.join(ROOT, "tests", "host", "prune_host.cpp"),
           "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe, d


def run(program, forest, tile, label):
    exe, d = program
    nodes, blocks, segs, mode = forest
    N, B, S = len(nodes["parent"]), len(blocks["node"]), len(segs)
    V = int(np.count_nonzero(nodes["parent"] < 0))
    src, dst = os.path.join(str(d), "in.bin"), os.path.join(str(d), "out.bin")
    with open(src, "wb") as f:
        parts = [np.array([N, V, B, mode, S], dtype=np.int64), np.array([b for _, b, _ in segs], dtype=np.int64),
                 np.array([dep for _, _, dep in segs], dtype=np.int64)]
        parts += [nodes[k].astype(np.int32) for k in ("voxel", "depth", "parent", "first_child", "epoch")]
        parts += [nodes["corner"].astype(np.float64), nodes["edge"].astype(np.float64), blocks["node"].astype(np.int32)]
        for a in parts:
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.run([exe, src, dst, str(tile)], capture_output=True, text=True)
    assert out.returncode == 0, (label, out.returncode, out.stderr[-4000:])
    raw = open(dst, "rb").read()
    at = [0]

    def take(dtype, count):
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=at[0])
        at[0] += a.nbytes
        return a

    n2, v2, internal, collapsed, deepest, s2 = take(np.int64, 6).tolist()
    seg_a, seg_b = take(np.int64, S), take(np.int64, S)
    got = {k: take(np.int32, n2) for k in ("voxel", "depth", "parent", "first_child", "epoch", "old_id")}
    got["corner"], got["edge"] = take(np.float64, 3 * n2).reshape(n2, 3), take(np.float64, n2)
    node_map, blk_node, vcode = take(np.int32, N), take(np.int32, B), take(np.uint64, v2)
    assert at[0] == len(raw) and s2 == S, label

    want = prune_np(nodes, blocks, mode)
    assert n2 == len(want.old_node) and v2 == int(np.count_nonzero(want.voxel_keep)), label
    for k in ("voxel", "depth", "parent", "first_child", "epoch"):
        assert np.array_equal(got[k], want.nodes[k]), (label, k)
    assert got["corner"].tobytes() == want.nodes["corner"].tobytes(), label
    assert got["edge"].tobytes() == want.nodes["edge"].tobytes(), label
    assert np.array_equal(got["old_id"], want.old_node), label
    assert np.array_equal(node_map, want.node_map), label
    assert np.array_equal(blk_node, want.blocks["node"]), label
    assert np.array_equal(vcode, 1000 + np.nonzero(want.voxel_keep)[0]), label
    assert collapsed == want.collapsed and internal == int(np.count_nonzero(want.nodes["first_child"] >= 0)), label
    # the level ranges: still ranges of one depth that tile the new table in the same order
    assert seg_a[0] == 0 and seg_b[0] == v2 and seg_b[-1] == n2 and np.array_equal(seg_a[1:], seg_b[:-1]), label
    for (_, _, dep), a, b in zip(segs, seg_a.tolist(), seg_b.tolist()):
        assert np.all(want.nodes["depth"][a:b] == dep), label
    assert deepest == (int(want.nodes["depth"].max()) if n2 else 0), label
    return seg_a, seg_b


@pytest.mark.parametrize("tile", [1, 7, 256])
def test_host_program_equals_prune_np(program, tile):
    for name, forest in CASES.items():
        run(program, forest, tile, f"{name}, tile {tile}")


def test_level_ranges_of_a_scheme_with_two_ranges_per_depth(program):
    seg_a, seg_b = run(program, CASES["two_segments_per_depth"], 7, "two_segments_per_depth")
    # (0,5) (5,21) (21,29) | (29,45) (45,61)  ->  the last range empties: test_cpu_prune.py has the node ids
    assert list(zip(seg_a.tolist(), seg_b.tolist())) == [(0, 3), (3, 19), (19, 27), (27, 35), (35, 35)]


def test_random_small_forests(program):
    rng = np.random.default_rng(5)
    for i in range(12):
        run(program, random_forest(rng), int(rng.integers(1, 40)), f"random forest {i}")
