"""What the raycast tests share: scenes and rays with the situations the query has to get right (ties in t, grazing
contacts, walls and an ulp either side of them), the leaf set of a map as raycast_np takes it, and - for the CPU tests -
the stand-alone host build of the kernel's traversal (tests/host/raycast_host.cpp) over the tables of a HostMap."""

import itertools
import os
import subprocess

import numpy as np

from octreelib_amd import RayHits, normalize_directions, raycast_np
from octreelib_amd.query import HostMap, check_raycast_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("node", "t", "row")
DIRECTIONS = np.array([d for d in itertools.product((-1.0, 0.0, 1.0), repeat=3) if any(d)])   # axes and all diagonals


def assert_hits_equal(got: RayHits, ref: RayHits, what):
    """All three fields equal, bit for bit up to the sign of zero (np.array_equal): the order (t, node) is total."""
    for name in FIELDS:
        a, b = getattr(got, name), getattr(ref, name)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, a.shape, b.dtype, b.shape)
        if not np.array_equal(a, b):
            bad = np.nonzero(a != b)[0]
            i = int(bad[0])
            raise AssertionError(f"{what}: {name} differs in {len(bad)} of {len(a)} rays, first {i}: got "
                                 f"{[getattr(got, f)[i].tolist() for f in FIELDS]}, expected "
                                 f"{[getattr(ref, f)[i].tolist() for f in FIELDS]}")


# ---- scenes and rays ---------------------------------------------------------------------------------------------------
def lattice_points():
    """{0, 1/8, .., 15/8}^3: with K = 8 and 1 m voxels every leaf is a cube of edge 1/4 that holds 8 points; every
    coordinate, wall and t along an axis is exact in f64."""
    t = np.arange(16) / 8.0
    return np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(-1, 3)


def lattice_rays(seed=0, n_origins=70):
    """Rays along the axes and the face and space diagonals, both signs, exact zero components included, from origins
    whose coordinates lie on lattice planes, on leaf and voxel walls, one ulp either side of them, and outside."""
    rng = np.random.default_rng(seed)
    vals = np.array([0.0, 0.125, 0.25, 0.5, 0.75, 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 1.25, 1.875, 2.0,
                     np.nextafter(2.0, 3.0), np.nextafter(0.0, -1.0), -0.5, 2.5, 0.3, 1.7])
    O = vals[rng.integers(0, len(vals), (n_origins, 3))]
    origins = np.repeat(O, len(DIRECTIONS), axis=0)
    directions = np.tile(DIRECTIONS, (n_origins, 1))
    return np.ascontiguousarray(origins), np.ascontiguousarray(directions)


def box_rays(rng, lo, hi, n, margin):
    """n random rays: origins uniform in the box [lo - margin, hi + margin], aimed at uniform points of [lo, hi] or, for
    a third of them, anywhere."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    O = rng.uniform(lo - margin, hi + margin, (n, 3))
    target = rng.uniform(lo, hi, (n, 3))
    D = target - O
    k = n // 3
    D[:k] = rng.normal(size=(k, 3))
    return O, D


def tie_mask(origins, unit_directions, t_max, leaf, **kw):
    """Rays whose two best candidates have the same t: the answer over the leaves numbered backwards (the largest id
    wins a tie) names another leaf at the same t."""
    node, corner, edge = leaf
    a = raycast_np(origins, unit_directions, t_max, node, corner, edge, **kw)
    b = raycast_np(origins, unit_directions, t_max, -np.asarray(node, dtype=np.int64), corner, edge, **kw)
    assert np.array_equal(a.t, b.t)
    return a.hit & (a.node != -b.node)


# ---- a map as raycast_np takes it -------------------------------------------------------------------------------------
def leaves_of(nodes, count_per_node=None):
    """((ids, corner, edge), count) of the scheme leaves of a node table."""
    leaf = np.nonzero(np.asarray(nodes["first_child"]) < 0)[0]
    cube = (leaf, np.asarray(nodes["corner"])[leaf], np.asarray(nodes["edge"])[leaf])
    return cube, None if count_per_node is None else np.asarray(count_per_node)[leaf]


def host_counts(hm: HostMap, pose_numbers=None):
    """Points of the chosen poses in every node of a HostMap."""
    per_node = np.zeros(len(hm.nodes["edge"]), dtype=np.int64)
    for p, leaves in hm._leaves.items():
        if pose_numbers is None or p in pose_numbers:
            for v in leaves:
                per_node[hm._id(v)] += len(v.get_points())
    return per_node


# ---- the kernel's traversal on the host --------------------------------------------------------------------------------
def build_host_program(directory):
    """tests/host/raycast_host.cpp compiled for the CPU alone with AddressSanitizer and UBSan; returns the program."""
    exe = os.path.join(str(directory), "raycast_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "octreelib_amd", "csrc"), os.path.join(ROOT, "tests", "host", "raycast_host.cpp"),
           "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def run_host_program(exe, directory, hm: HostMap, origins, unit_directions, t_min, t_max, surface="cube",
                     min_points=None, max_variance=None, pose_numbers=None) -> RayHits:
    """The answers of the host build over the tables of `hm`, laid out as the device lays them out: packed voxel keys
    relative to the smallest voxel, the node table with parents, one block record per occupied leaf, 64-byte plane
    rows."""
    code, min_points, mv = check_raycast_args(surface, min_points, max_variance)
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
    count = host_counts(hm, pose_numbers)
    held = np.nonzero(count > 0)[0]
    rec = np.zeros((len(held), 4), dtype=np.uint32)
    rec[:, 1] = count[held]
    first = np.zeros(N, dtype=np.int32)
    cnt = np.zeros(N, dtype=np.int32)
    first[held] = np.arange(len(held))
    cnt[held] = 1
    node_row = np.full(N, -1, dtype=np.int32)
    rows = np.zeros((0, 8))
    if code == 1:
        planes = hm.leaf_planes(pose_numbers)
        node_row[planes.node] = np.arange(len(planes))
        rows = np.concatenate([planes.normal, planes.mean, planes.eigenvalues[:, :1],
                               planes.count[:, None].astype(np.float64)], axis=1)
    n = len(origins)
    tmin = np.broadcast_to(np.asarray(t_min, dtype=np.float64), (n,))
    tmax = np.broadcast_to(np.asarray(t_max, dtype=np.float64), (n,))
    head = np.array([hm.mode, len(vcode), N, len(rec), len(rows), n, code, min_points, *org], dtype=np.int64)
    src, dst = os.path.join(str(directory), "rays.in"), os.path.join(str(directory), "rays.out")
    with open(src, "wb") as f:
        for a, dt in ((head, np.int64), ([hm.edge, mv], np.float64), (vcode, np.uint64), (fc, np.int32),
                      (parent, np.int32), (nodes["corner"], np.float64), (nodes["edge"], np.float64), (first, np.int32),
                      (cnt, np.int32), (rec, np.uint32), (node_row, np.int32), (rows, np.float64),
                      (origins, np.float64), (unit_directions, np.float64), (tmin, np.float64), (tmax, np.float64)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-4000:])
    raw = open(dst, "rb").read()
    assert len(raw) == 16 * n
    return RayHits(np.frombuffer(raw, np.int32, n, 0).copy(), np.frombuffer(raw, np.float64, n, 8 * n).copy(),
                   np.frombuffer(raw, np.int32, n, 4 * n).copy())
