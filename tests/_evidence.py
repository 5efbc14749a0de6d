"""What the ray-evidence tests share: the definition over a node table, the comparison, rays with measured ranges for
the raycast scenes (tests/_raycast.py), and - for the CPU tests - the stand-alone host build of the kernel's walk
(tests/host/evidence_host.cpp) over the tables of a HostMap."""

import os
import subprocess

import numpy as np

from octreelib_amd import RayEvidence, ray_evidence_np
from octreelib_amd.query import HostMap, evidence_inputs
from tests._raycast import ROOT, leaves_of


def evidence_of_nodes(nodes, o, d, t_min, t_free, t_end) -> RayEvidence:
    """ray_evidence_np over the leaves of a node table (HostMap.nodes or the engine's)."""
    (leaf, corner, edge), _ = leaves_of(nodes)
    return ray_evidence_np(o, d, t_min, t_free, t_end, leaf, corner, edge, len(np.asarray(nodes["edge"])))


def assert_evidence_equal(got: RayEvidence, ref: RayEvidence, what):
    for name in ("through", "hits"):
        a, b = getattr(got, name), getattr(ref, name)
        assert a.dtype == b.dtype == np.uint32 and a.shape == b.shape, (what, name, a.dtype, a.shape, b.dtype, b.shape)
        if not np.array_equal(a, b):
            bad = np.nonzero(a != b)[0]
            i = int(bad[0])
            raise AssertionError(f"{what}: {name} differs in {len(bad)} of {len(a)} nodes, first {i}: got {a[i]}, "
                                 f"expected {b[i]}")


def measured(rng, n, lo, hi, no_echo=0.1):
    """(ranges (n,), returned (n,)): ranges uniform in [lo, hi], some of them exact multiples of 1/8 (ends on lattice
    planes), a share without an echo."""
    r = rng.uniform(lo, hi, n)
    k = n // 4
    r[:k] = np.round(r[:k] * 8.0) / 8.0
    return r, rng.random(n) >= no_echo


# ---- the kernel's walk on the host -------------------------------------------------------------------------------------
def build_host_program(directory):
    """tests/host/evidence_host.cpp compiled for the CPU alone with AddressSanitizer and UBSan; returns the program."""
    exe = os.path.join(str(directory), "evidence_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "octreelib_amd", "csrc"), os.path.join(ROOT, "tests", "host", "evidence_host.cpp"),
           "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def run_host_program(exe, directory, hm: HostMap, o, d, t_min, t_free, t_end) -> RayEvidence:
    """The counters of the host build over the tables of `hm`, laid out as the device lays them out (packed voxel keys
    relative to the smallest voxel, the node table with parents)."""
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
    n = len(o)
    ts = [np.broadcast_to(np.asarray(t, dtype=np.float64), (n,)) for t in (t_min, t_free, t_end)]
    head = np.array([hm.mode, len(vcode), N, n, *org], dtype=np.int64)
    src, dst = os.path.join(str(directory), "rays.in"), os.path.join(str(directory), "rays.out")
    with open(src, "wb") as f:
        for a, dt in ((head, np.int64), ([hm.edge], np.float64), (vcode, np.uint64), (fc, np.int32), (parent, np.int32),
                      (nodes["corner"], np.float64), (nodes["edge"], np.float64), (o, np.float64), (d, np.float64),
                      (ts[0], np.float64), (ts[1], np.float64), (ts[2], np.float64)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-4000:])
    raw = open(dst, "rb").read()
    assert len(raw) == 8 * N
    return RayEvidence(np.frombuffer(raw, np.uint32, N, 0).copy(), np.frombuffer(raw, np.uint32, N, 4 * N).copy())


def compare_host(program, hm: HostMap, O, D, ranges, margin, what, min_range=0.0, returned=None):
    """Host program against the definition on the inputs evidence_inputs makes; returns (reference, inputs)."""
    exe, d = program
    inp = evidence_inputs(O, D, ranges, margin, min_range, returned)
    got = run_host_program(exe, d, hm, *inp)
    ref = evidence_of_nodes(hm.nodes, *inp)
    assert_evidence_equal(got, ref, what)
    return ref, inp
