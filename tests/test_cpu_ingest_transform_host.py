"""The per-thread body of k_ingest_xf (octreelib_amd/csrc/ingest_xf.h: ingest_xf_thread - row-group index arithmetic,
tails, index clamping, matrix pick) compiled for the CPU alone, with AddressSanitizer and UBSan and without contraction,
as the stand-alone program tests/host/ingest_xf_host.cpp, and compared byte for byte with transform_rows_np.  No GPU and
nothing loaded into Python: the program gets the cloud, the indices and the table from a file, puts each into a heap
block that ends exactly behind its last element and loops over the threads of a launch.  This test is about that
program: it compiles it once (a few seconds) and starts it once per case."""

import os
import subprocess

import numpy as np
import pytest

from octreelib_amd.registration import se3_exp, transform_rows_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 2, 3, 4, 5, 7, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 20_006]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("ingest_xf_host")
    exe = os.path.join(str(d), "ingest_xf_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "octreelib_amd", "csrc"), os.path.join(ROOT, "tests", "host", "ingest_xf_host.cpp"),
           "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe, d


def _run(program, cloud, table, segment=None, dst_odd=False, src_off=False, in_place=False):
    """The rows the host build stores for `cloud` under table (M, 12) / segment (raw uint16, not validated)."""
    exe, d = program
    n, f32 = len(cloud), cloud.dtype == np.float32
    head = np.array([n, f32, segment is not None, len(table), dst_odd, src_off, in_place], dtype=np.int64)
    src, dst = os.path.join(str(d), "rows.in"), os.path.join(str(d), "rows.out")
    with open(src, "wb") as f:
        f.write(head.tobytes())
        f.write(np.ascontiguousarray(table, dtype=np.float64).tobytes())
        if segment is not None:
            f.write(np.ascontiguousarray(segment, dtype=np.uint16).tobytes())
        f.write(np.ascontiguousarray(cloud).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-4000:])
    raw = open(dst, "rb").read()
    assert len(raw) == 24 * n + 8
    assert int(np.frombuffer(raw[24 * n:], dtype=np.int64)[0]) == n      # every row folded once
    return np.frombuffer(raw[:24 * n], dtype=np.float64).reshape(n, 3)


def _cloud(n, seed, dtype):
    rng = np.random.default_rng(seed)
    p = (rng.random((n, 3)) * 40.0 - 20.0).astype(dtype)
    if n > 2:
        p[1] = [-0.0, 0.0, -0.0]
        p[n // 2, 1] = np.nan
    return p


def _transforms(m, seed):
    rng = np.random.default_rng(seed)
    return np.stack([se3_exp(np.concatenate([rng.normal(size=3), rng.normal(size=3) * 10.0])) for _ in range(m)])


def _table(T):
    return np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(-1, 4, 4)[:, :3, :].reshape(-1, 12))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rigid_every_size_and_both_destination_parities(program, dtype):
    T = _transforms(1, 3)[0]
    for n in SIZES:
        cloud = _cloud(n, n + 1, dtype)
        want = transform_rows_np(T, cloud)
        for dst_odd in (False, True):
            got = _run(program, cloud, _table(T), dst_odd=dst_odd, src_off=(n % 2 == 1))
            assert got.tobytes() == want.tobytes(), (n, dst_odd)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_piecewise_every_size_and_both_destination_parities(program, dtype):
    Ts = _transforms(3, 5)
    for n in SIZES:
        cloud = _cloud(n, n + 2, dtype)
        rng = np.random.default_rng(n)
        seg = np.sort(rng.integers(0, 3, n)) if n % 2 else rng.integers(0, 3, n)    # runs / shuffled
        want = transform_rows_np(Ts, cloud, seg)
        for dst_odd in (False, True):
            got = _run(program, cloud, _table(Ts), seg, dst_odd=dst_odd, src_off=(n % 3 == 1))
            assert got.tobytes() == want.tobytes(), (n, dst_odd)


def test_f64_cloud_moved_in_place(program):
    """The host f64 form: the cloud lies in the store and is moved there - a thread reads all its rows first."""
    Ts = _transforms(4, 7)
    for n in (1, 2, 3, 5, 1023, 1025, 4097):
        cloud = _cloud(n, n, np.float64)
        seg = np.random.default_rng(n).integers(0, 4, n)
        for dst_odd in (False, True):
            got = _run(program, cloud, _table(Ts[0]), dst_odd=dst_odd, in_place=True)
            assert got.tobytes() == transform_rows_np(Ts[0], cloud).tobytes()
            got = _run(program, cloud, _table(Ts), seg, dst_odd=dst_odd, in_place=True)
            assert got.tobytes() == transform_rows_np(Ts, cloud, seg).tobytes()


@pytest.mark.parametrize("m", [1, 2, 64, 1024])
def test_table_sizes_and_clamped_indices(program, m):
    """Every table row is reachable, and an index at or beyond M reads row M - 1: no read leaves the table (the table
    is a heap block of exactly M matrices)."""
    Ts = _transforms(m, m)
    n = 2500
    for dtype in (np.float64, np.float32):
        cloud = _cloud(n, 11, dtype)
        rng = np.random.default_rng(m)
        seg = rng.integers(0, m, n)
        seg[:m] = np.arange(m)[:n]
        got = _run(program, cloud, _table(Ts), seg)
        assert got.tobytes() == transform_rows_np(Ts, cloud, seg).tobytes()
        raw = seg.copy()
        raw[::7] = m + rng.integers(0, 65535 - m, len(raw[::7]))
        raw[-1] = 65535
        got = _run(program, cloud, _table(Ts), raw, dst_odd=True)
        assert got.tobytes() == transform_rows_np(Ts, cloud, np.minimum(raw, m - 1)).tobytes()
        only_last = np.full(n, m - 1)
        got = _run(program, cloud, _table(Ts), only_last)
        assert got.tobytes() == transform_rows_np(Ts, cloud, only_last).tobytes()
