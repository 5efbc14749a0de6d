"""What the cell tests share: the 0.1 lattice whose coordinates fall either side of their cell walls, an independent
dict-of-tuples model of the two rules with exact rational arithmetic, and - for the CPU tests - the stand-alone host
build of the kernels' walk (tests/host/cell_host.cpp) over the tables of a HostMap."""

import os
import subprocess
from fractions import Fraction

import numpy as np

from octreelib_amd.query import HostMap
from tests._raycast import ROOT

CELL = 0.1
CAPS = (None, 1, 3, 7)


# ---- an independent model ----------------------------------------------------------------------------------------------
def exact_cell(row, cell):
    """The cell of one point as a tuple of Python ints: the floor of the exact rational quotient (None: not finite)."""
    if not all(np.isfinite(v) for v in row):
        return None
    c = Fraction(float(cell))
    return tuple((Fraction(float(v)) / c).__floor__() for v in row)


def model_count(Q, clouds, cell, cap=None):
    held = {}
    for _, P in clouds:
        for row in np.asarray(P, dtype=np.float64).reshape(-1, 3).tolist():
            key = exact_cell(row, cell)
            if key is not None:
                held[key] = held.get(key, 0) + 1
    out = [held.get(exact_cell(row, cell), 0) for row in np.asarray(Q, dtype=np.float64).reshape(-1, 3).tolist()]
    return np.array([c if cap is None else min(c, cap) for c in out], dtype=np.int32).reshape(-1)


def model_keep(clouds, counted, tested, cell, m):
    """keep per cloud of `clouds` ([(pose, points)] in slot order; None for a cloud that is not tested): a point stays
    iff fewer than m points of the counted poses with a smaller (cloud position, row) share its cell."""
    ids = {}
    for s, (p, P) in enumerate(clouds):
        if p in counted:
            for r, row in enumerate(np.asarray(P).tolist()):
                ids.setdefault(exact_cell(row, cell), []).append((s, r))
    out = []
    for s, (p, P) in enumerate(clouds):
        if p not in tested:
            out.append(None)
            continue
        keep = np.ones(len(P), dtype=bool)
        for r, row in enumerate(np.asarray(P).tolist()):
            key = exact_cell(row, cell)
            keep[r] = key is None or sum(1 for i in ids.get(key, ()) if i < (s, r)) < m
        out.append(keep)
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------
def lattice01(lo=-8, hi=8):
    """fl(k * 0.1) for k in [lo, hi) per axis: coordinates that the rounding of k * 0.1 puts on either side of the wall
    of cell k.  Returns (points (n^3, 3), the k of every coordinate (n^3, 3))."""
    k = np.arange(lo, hi)
    t = k * CELL
    P = np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(-1, 3)
    K = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(P), K


def ulp_neighbours(P):
    """P with every coordinate moved one ulp up, and one ulp down."""
    return np.nextafter(P, np.inf), np.nextafter(P, -np.inf)


# ---- the kernels' walk on the host -------------------------------------------------------------------------------------
def build_host_program(directory):
    """tests/host/cell_host.cpp compiled for the CPU alone with AddressSanitizer and UBSan (the flags of
    tests/_raycast.py: build_host_program); returns the program."""
    exe = os.path.join(str(directory), "cell_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "octreelib_amd", "csrc"), os.path.join(ROOT, "tests", "host", "cell_host.cpp"),
           "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def host_tables(hm: HostMap, pose_numbers=None):
    """The tables of `hm` laid out as the device lays them out (tests/_raycast.py: run_host_program has the same voxel
    keys and node table): the store is every pose's cloud in insertion order (HostMap.clouds), the ordered arrays are
    the (leaf, pose) blocks of the selected poses in (node, slot) order."""
    nodes = hm.nodes
    fc = np.asarray(nodes["first_child"], dtype=np.int32)
    N = len(fc)
    parent = np.full(N, -1, dtype=np.int32)
    for i in np.nonzero(fc >= 0)[0]:
        parent[fc[i]:fc[i] + 8] = i
    if hm.mode == 0:
        vox = np.floor_divide(hm.voxels, int(hm.edge)).astype(np.int64)
    else:
        vox = np.zeros((1, 3), dtype=np.int64)
    org = vox.min(axis=0) if hm.mode == 0 else np.zeros(3, dtype=np.int64)
    rel = (vox - org + (1 << 20)).astype(np.uint64)
    vcode = (rel[:, 0] << np.uint64(42)) | (rel[:, 1] << np.uint64(21)) | rel[:, 2]
    assert np.all(np.diff(vcode.astype(np.int64)) > 0)
    blocks, off = [], 0
    for slot, (p, leaves) in enumerate(hm._leaves.items()):
        for v in leaves:
            pts = np.asarray(v.get_points(), dtype=np.float64).reshape(-1, 3)
            if len(pts) and (pose_numbers is None or p in pose_numbers):
                blocks.append((hm._id(v), slot, pts, off + np.arange(len(pts))))
            off += len(pts)
    blocks.sort(key=lambda b: (b[0], b[1]))
    rec = np.zeros((len(blocks), 4), dtype=np.uint32)
    first, cnt = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    start = 0
    for i, (node, slot, pts, _) in enumerate(blocks):
        rec[i] = (start, len(pts), slot, 0)
        if cnt[node] == 0:
            first[node] = i
        cnt[node] += 1
        start += len(pts)
    xyz_ord = np.concatenate([b[2] for b in blocks]) if blocks else np.empty((0, 3))
    ord_idx = np.concatenate([b[3] for b in blocks]).astype(np.uint32) if blocks else np.empty(0, dtype=np.uint32)
    return dict(vcode=vcode, org=org, fc=fc, parent=parent, first=first, cnt=cnt, rec=rec, xyz_ord=xyz_ord,
                ord_idx=ord_idx)


def run_host_program(exe, directory, hm: HostMap, Q, cell, cap=None, pose_numbers=None, below=None, tables=None):
    """The counts of the host build for the queries Q over the tables of `hm`.  below (n,) uint32: only stored points
    with a smaller store index count (the rank of thin); None: every one."""
    t = host_tables(hm, pose_numbers) if tables is None else tables
    Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, 3)
    n = len(Q)
    below = np.full(n, 0xffffffff, dtype=np.uint32) if below is None else np.asarray(below, dtype=np.uint32)
    nodes = hm.nodes
    head = np.array([hm.mode, len(t["vcode"]), len(t["fc"]), len(t["rec"]), len(t["ord_idx"]), n,
                     2 ** 31 - 1 if cap is None else cap, *t["org"]], dtype=np.int64)
    src, dst = os.path.join(str(directory), "cell.in"), os.path.join(str(directory), "cell.out")
    with open(src, "wb") as f:
        for a, dt in ((head, np.int64), ([hm.edge, cell], np.float64), (t["vcode"], np.uint64), (t["fc"], np.int32),
                      (t["parent"], np.int32), (nodes["corner"], np.float64), (nodes["edge"], np.float64),
                      (t["first"], np.int32), (t["cnt"], np.int32), (t["rec"], np.uint32), (t["xyz_ord"], np.float64),
                      (t["ord_idx"], np.uint32), (Q, np.float64), (below, np.uint32)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-4000:])
    raw = open(dst, "rb").read()
    assert len(raw) == 4 * n
    return np.frombuffer(raw, np.int32, n).copy()
