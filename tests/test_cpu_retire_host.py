"""The row map of octl_forest_remove_poses (octreelib_amd/csrc/store_retire.h: the old end offsets and one shift per
pose - the code k_retire_poses runs) compiled for the CPU alone, with AddressSanitizer and UBSan, as the stand-alone
program tests/host/retire_host.cpp, and compared with np.concatenate of the poses that stay.  No GPU and nothing loaded
into Python: the program gets heap arrays of exactly their size from a file.  This test is about that program: it
compiles it once (a few seconds) and starts it once per case and tile size."""

import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("retire_host")
    exe = os.path.join(str(d), "retire_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "octreelib_amd", "csrc"), os.path.join(ROOT, "tests", "host", "retire_host.cpp"),
           "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe, d


def model(sizes, removed, xyz, alive):
    """The squeezed store, its flags and the new row of every old row: the definition."""
    off = np.concatenate(([0], np.cumsum(sizes)))
    keep = [p for p in range(len(sizes)) if p not in removed]
    rows = [np.arange(off[p], off[p + 1]) for p in keep]
    rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    fwd = np.full(off[-1], -1, dtype=np.int64)
    fwd[rows] = np.arange(len(rows))
    return xyz[rows], alive[rows], fwd


def run(program, sizes, removed, tile, seed=0):
    exe, d = program
    sizes = np.asarray(sizes, dtype=np.int64)
    rng = np.random.default_rng(seed)
    n = int(sizes.sum())
    xyz = rng.normal(size=(n, 3))
    alive = (rng.random(n) < 0.8).astype(np.uint8)
    end = np.cumsum(sizes)
    gone = np.array([sizes[p] if p in removed else 0 for p in range(len(sizes))], dtype=np.int64)
    shift = np.concatenate(([0], np.cumsum(gone)))
    src, dst = os.path.join(str(d), "in.bin"), os.path.join(str(d), "out.bin")
    with open(src, "wb") as f:
        for a in (np.array([len(sizes), n], dtype=np.int64), end, shift, xyz, alive):
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.run([exe, src, dst, str(tile)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-4000:])
    raw = open(dst, "rb").read()
    n_new = int(np.frombuffer(raw, dtype=np.int64, count=1)[0])
    got_xyz = np.frombuffer(raw, dtype=np.float64, count=3 * n_new, offset=8).reshape(n_new, 3)
    got_alive = np.frombuffer(raw, dtype=np.uint8, count=n_new, offset=8 + 24 * n_new)
    got_fwd = np.frombuffer(raw, dtype=np.int64, count=n, offset=8 + 25 * n_new)
    want_xyz, want_alive, want_fwd = model(sizes, set(removed), xyz, alive)
    label = f"sizes {sizes.tolist()}, removed {sorted(removed)}, tile {tile}"
    assert n_new == len(want_xyz), label
    assert got_xyz.tobytes() == want_xyz.tobytes(), label
    assert np.array_equal(got_alive, want_alive), label
    assert np.array_equal(got_fwd, want_fwd), label


CASES = [
    # (sizes, removed)
    ([5, 4, 6], {0}),                      # first, odd shift
    ([4, 5, 6], {0}),                      # first, even shift
    ([5, 4, 6], {1}),                      # middle
    ([5, 4, 7], {2}),                      # last
    ([5, 4, 7, 3], {0, 2}),                # two non-adjacent: odd then even total shift
    ([5, 4, 7, 3], {0, 1, 2, 3}),          # all
    ([5, 4, 7], set()),                    # none
    ([0, 0, 5, 0, 4, 0, 0, 7, 0], {2}),    # empty poses in front, between and behind; remove a full one
    ([0, 0, 5, 0, 4, 0, 0, 7, 0], {4}),
    ([0, 0, 5, 0, 4, 0, 0, 7, 0], {0, 3, 8}),     # remove only empty ones: nothing moves
    ([0, 0, 5, 0, 4, 0, 0, 7, 0], {1, 2, 5, 7}),
    ([1], {0}),                            # one row, gone
    ([1], set()),                          # one row, kept
    ([1, 1, 1], {1}),
    ([3, 1, 0, 2], {1}),                   # the one-row pose leaves: everything behind moves by one row
    ([1001, 778, 1535, 2048, 1, 0], {0}),  # the scene of the GPU tests: later poses move by an odd shift
    ([1001, 778, 1535, 2048, 1, 0], {1, 3}),
    ([1001, 778, 1535, 2048, 1, 0], {4}),
    ([1001, 778, 1535, 2048, 1, 0], {5}),
]


@pytest.mark.parametrize("tile", [1, 7, 2048])
def test_row_map_equals_the_concatenation_of_the_kept_poses(program, tile):
    for i, (sizes, removed) in enumerate(CASES):
        run(program, sizes, removed, tile, seed=i)


def test_random_partitions(program):
    rng = np.random.default_rng(11)
    for i in range(12):
        P = int(rng.integers(1, 12))
        sizes = rng.integers(0, 40, P) * (rng.random(P) < 0.7)
        removed = set(np.nonzero(rng.random(P) < 0.4)[0].tolist())
        run(program, sizes, removed, int(rng.integers(1, 33)), seed=100 + i)
