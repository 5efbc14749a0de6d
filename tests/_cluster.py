"""What the cluster tests share: the plain O(n^2) definition (adjacency matrix plus breadth-first search), the scenes - a
chain of points spaced exactly `radius` apart with one gap an ulp wider - and, for the CPU tests, the
stand-alone host build of the kernels' linking sink (tests/host/cluster_host.cpp) over the tables of a HostMap
(tests/_cell.py: host_tables)."""

import os
import subprocess

import numpy as np

from octreelib_amd.query import HostMap
from tests._cell import host_tables
from tests._raycast import ROOT


def adjacency(P, radius):
    """(n, n) bool: d2 <= r2 in radius_count_np's own expression."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        dx = P[:, None, 0] - P[None, :, 0]
        dy = P[:, None, 1] - P[None, :, 1]
        dz = P[:, None, 2] - P[None, :, 2]
        return (dx * dx + dy * dy) + dz * dz <= np.float64(radius) * np.float64(radius)


def brute_roots(P, radius):
    """Smallest member of the connected component of every row: adjacency matrix and breadth-first search."""
    adj = adjacency(P, radius)
    assert np.array_equal(adj, adj.T)                      # the expression is symmetric bit for bit
    n = len(adj)
    root = np.full(n, -1, dtype=np.int64)
    for s in range(n):
        if root[s] >= 0:
            continue
        root[s] = s
        queue = [s]
        while queue:
            u = queue.pop()
            for v in np.nonzero(adj[u] & (root < 0))[0]:
                root[v] = s
                queue.append(int(v))
    return root


def brute_labels(clouds, radius, lo=1, hi=None):
    """cluster_labels_np's answer from brute_roots: (labels per cloud, sizes, first)."""
    parts = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for _, c in clouds]
    P = np.concatenate(parts) if parts else np.empty((0, 3))
    root = brute_roots(P, radius)
    size = np.bincount(root, minlength=len(P))[root]
    inside = (size >= lo) & ((size <= hi) if hi is not None else True)
    keys = np.unique(root[inside])
    label = np.where(inside, np.searchsorted(keys, root), -1).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    where = np.searchsorted(off, keys, side="right") - 1
    first = np.stack([where, keys - off[where]], axis=1).reshape(-1, 2)
    return np.split(label, off[1:-1]), np.bincount(root, minlength=len(P))[keys].astype(np.int64), first


CHAIN_RADIUS = 13.0 * 2.0 ** -7          # 0.1015625
CHAIN_START = (-1.25, -0.75, -2.5)


def diagonal_chain(n=60, gap_at=41, start=CHAIN_START):
    """n points along the diagonal (3, 4, 12) / 13, consecutive ones EXACTLY CHAIN_RADIUS apart in the kernel's
    arithmetic: the step is (3, 4, 12) 2^-7, every coordinate is a multiple of 2^-7 below 4 and 3^2 + 4^2 + 12^2 = 13^2,
    so every difference, product and sum is exact and d2 == r2 bit for bit (inclusive: joined).  From point gap_at on
    every x is 2^-51 larger - one ulp of a coordinate in [2, 4), still exact - so the one step across the gap has
    d2 > r2 while every other step keeps d2 == r2: the chain is two clusters, [0, gap_at) and [gap_at, n).  From the
    default start it crosses integer voxel walls (negative voxels included) and, its coordinates being multiples of
    2^-7, lies on leaf walls again and again.  Returns (n, 3) float64."""
    step = np.array([3.0, 4.0, 12.0]) * 2.0 ** -7
    P = np.asarray(start, dtype=np.float64) + np.arange(n, dtype=np.float64)[:, None] * step
    P[gap_at:, 0] += 2.0 ** -51
    assert np.abs(P).max() < 4.0
    d = P[1:] - P[:-1]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    r2 = np.float64(CHAIN_RADIUS) * np.float64(CHAIN_RADIUS)
    assert np.all(np.delete(d2, gap_at - 1) == r2) and d2[gap_at - 1] > r2
    return P


# ---- the kernels' sink on the host -------------------------------------------------------------------------------------
def build_host_program(directory):
    """tests/host/cluster_host.cpp compiled for the CPU alone with AddressSanitizer and UBSan (the compile line of
    tests/_cell.py: build_host_program); returns the program."""
    exe = os.path.join(str(directory), "cluster_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "octreelib_amd", "csrc"), os.path.join(ROOT, "tests", "host", "cluster_host.cpp"),
           "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def run_host_program(exe, directory, hm: HostMap, radius, pose_numbers=None, reversed_order=False):
    """(root, size, first) per position of the ordered arrays from the host build over the tables of `hm`, and the
    tables themselves."""
    t = host_tables(hm, pose_numbers)
    nodes = hm.nodes
    n = len(t["ord_idx"])
    head = np.array([hm.mode, len(t["vcode"]), len(t["fc"]), len(t["rec"]), n, int(reversed_order), 0, *t["org"]],
                    dtype=np.int64)
    src, dst = os.path.join(str(directory), "cluster.in"), os.path.join(str(directory), "cluster.out")
    with open(src, "wb") as f:
        for a, dt in ((head, np.int64), ([hm.edge, radius], np.float64), (t["vcode"], np.uint64), (t["fc"], np.int32),
                      (t["parent"], np.int32), (nodes["corner"], np.float64), (nodes["edge"], np.float64),
                      (t["first"], np.int32), (t["cnt"], np.int32), (t["rec"], np.uint32), (t["xyz_ord"], np.float64),
                      (t["ord_idx"], np.uint32)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-4000:])
    raw = open(dst, "rb").read()
    assert len(raw) == 16 * n
    root = np.frombuffer(raw, np.int32, n).copy()
    size = np.frombuffer(raw, np.uint32, n, offset=4 * n).copy()
    first = np.frombuffer(raw, np.uint64, n, offset=8 * n).copy()
    return root, size, first, t
