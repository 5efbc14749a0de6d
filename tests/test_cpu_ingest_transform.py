"""Inserting under a transform, without a GPU: transform_rows_np (the definition) against a per-row loop and its
validation errors; the entries declared, bound and exported; the keyword-only arguments of the classes; the caller's own
plug types fed the host-transformed cloud."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import octreelib_amd as oa
from octreelib_amd import MaxPoints
from octreelib_amd import _native as nat
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree
from octreelib_amd.octree.octree_base import OctreeConfigBase
from octreelib_amd.octree_manager import OctreeManager
from octreelib_amd.registration import se3_exp, transform_np, transform_rows_np

from tests.test_cpu_query import HostManager, HostOctree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _transforms(m, seed):
    rng = np.random.default_rng(seed)
    return np.stack([se3_exp(np.concatenate([rng.normal(size=3), rng.normal(size=3) * 5.0])) for _ in range(m)])


# ---- the definition ------------------------------------------------------------------------------------------------
def test_exported():
    assert "transform_rows_np" in oa.__all__ and oa.transform_rows_np is transform_rows_np


@pytest.mark.parametrize("m", [1, 2, 3, 64, 1024])
def test_rows_against_a_per_row_loop(m):
    rng = np.random.default_rng(m)
    P = rng.normal(size=(700, 3)) * 30.0
    P[3] = [-0.0, 0.0, -0.0]
    Ts = _transforms(m, m + 1)
    seg = rng.integers(0, m, len(P))
    seg[:2] = [m - 1, 0]
    want = np.concatenate([transform_np(Ts[seg[i]], P[i:i + 1]) for i in range(len(P))])
    for T, s in ((Ts, seg), (Ts[:, :3, :], seg.astype(np.uint16)), (Ts, seg.astype(np.int64).tolist())):
        got = transform_rows_np(T, P, s)
        assert got.dtype == np.float64 and got.flags.c_contiguous and got.tobytes() == want.tobytes()


def test_one_transform_is_transform_np_bit_for_bit():
    rng = np.random.default_rng(2)
    P = rng.normal(size=(500, 3)) * 1e3
    T = _transforms(1, 9)[0]
    assert transform_rows_np(T, P).tobytes() == transform_np(T, P).tobytes()
    assert transform_rows_np(T[:3], P).tobytes() == transform_np(T, P).tobytes()
    # M = 1 as a stack
    assert transform_rows_np(T[None], P, np.zeros(len(P), dtype=np.int32)).tobytes() == transform_np(T, P).tobytes()
    # the identity is not the identity on bits: 1 * -0.0 + 0 * y = +0.0
    z = transform_rows_np(np.eye(4), np.array([[-0.0, -0.0, -0.0]]))
    assert not np.signbit(z).any()
    assert transform_rows_np(T, np.empty((0, 3))).shape == (0, 3)
    assert transform_rows_np(T[None], np.empty((0, 3)), np.empty(0, dtype=np.int64)).shape == (0, 3)


def test_f32_points_are_widened_first():
    rng = np.random.default_rng(3)
    P = (rng.normal(size=(300, 3)) * 50.0).astype(np.float32)
    Ts = _transforms(4, 4)
    seg = rng.integers(0, 4, len(P))
    assert transform_rows_np(Ts[0], P).tobytes() == transform_np(Ts[0], P.astype(np.float64)).tobytes()
    assert transform_rows_np(Ts, P, seg).tobytes() == transform_rows_np(Ts, P.astype(np.float64), seg).tobytes()


def test_validation_errors():
    P = np.zeros((5, 3))
    T = np.eye(4)
    seg = np.zeros(5, dtype=np.int64)
    bad_row = np.eye(4)
    bad_row[3, 0] = 1.0
    with pytest.raises(ValueError, match=r"the last row of a 4x4 transform must be \(0, 0, 0, 1\)"):
        transform_rows_np(bad_row, P)
    with pytest.raises(ValueError, match=r"the last row of a 4x4 transform must be \(0, 0, 0, 1\)"):
        transform_rows_np(np.stack([T, bad_row]), P, seg)
    with pytest.raises(ValueError, match=r"expected a 4x4 or 3x4 transform, got shape \(3, 3\)"):
        transform_rows_np(np.eye(3), P)
    with pytest.raises(ValueError, match=r"expected a 4x4 or 3x4 transform, got shape \(2, 4\)"):
        transform_rows_np(np.zeros((2, 2, 4)), P, seg)
    nf = np.eye(4)
    nf[1, 3] = np.inf
    with pytest.raises(ValueError, match="the transform is not finite"):
        transform_rows_np(nf, P)
    with pytest.raises(ValueError, match="the transform is not finite"):
        transform_rows_np(np.stack([T, T, nf]), P, seg)
    with pytest.raises(ValueError, match="0 transforms: between 1 and 1024"):
        transform_rows_np(np.zeros((0, 4, 4)), P, seg)
    with pytest.raises(ValueError, match="1025 transforms: between 1 and 1024"):
        transform_rows_np(np.tile(T, (1025, 1, 1)), P, seg)
    with pytest.raises(ValueError, match="needs segment"):
        transform_rows_np(T[None], P)
    with pytest.raises(ValueError, match="segment is given with a single transform"):
        transform_rows_np(T, P, seg)
    with pytest.raises(ValueError, match="integer dtype"):
        transform_rows_np(T[None], P, np.zeros(5))
    with pytest.raises(ValueError, match=r"segment must have shape \(5,\)"):
        transform_rows_np(T[None], P, np.zeros(4, dtype=np.int64))
    with pytest.raises(ValueError, match=r"segment must have shape \(5,\)"):
        transform_rows_np(T[None], P, np.zeros((5, 1), dtype=np.int64))
    with pytest.raises(ValueError, match=r"segment entries must lie in \[0, 2\)"):
        transform_rows_np(np.stack([T, T]), P, np.array([0, 1, 2, 0, 0]))
    with pytest.raises(ValueError, match=r"segment entries must lie in \[0, 2\)"):
        transform_rows_np(np.stack([T, T]), P, np.array([0, 1, -1, 0, 0]))
    with pytest.raises(ValueError, match="stack of them"):
        transform_rows_np(np.zeros((1, 1, 4, 4)), P, seg)


# ---- the entries and the classes -----------------------------------------------------------------------------------
DECLS = {
    "octl_forest_add_pose_xf": "int octl_forest_add_pose_xf(octl_forest* f, const void* xyz, int64_t n, uint32_t flags, "
                               "const double* transforms, int32_t n_transforms, const uint16_t* segment, int32_t* slot);",
    "octl_forest_extend_pose_xf": "int octl_forest_extend_pose_xf(octl_forest* f, int32_t slot, const void* xyz, "
                                  "int64_t n, uint32_t flags, const double* transforms, int32_t n_transforms, "
                                  "const uint16_t* segment);",
}


def test_entries_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "octreelib_hip.h")).read()
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "#define OCTL_XF_MAX_SEGMENTS 1024" in header
    assert "enum { OCTL_XF_F32 = 1, OCTL_XF_DEVICE = 2 };" in header
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = nat.load()     # (loading does not touch the GPU)
    for name, decl in DECLS.items():
        assert decl in header
        res, args = nat.SIGNATURES[name]
        assert res is C.c_int and len(args) == decl.count(",") + 1
        assert hasattr(lib, name) and name in integration
    from octreelib_amd.registration import XF_MAX_SEGMENTS

    assert XF_MAX_SEGMENTS == 1024


def test_new_arguments_are_keyword_only():
    for cls, positional in ((Grid, ["self", "pose_number", "points"]), (OctreeManager, ["self", "pose_number", "points"]),
                            (Octree, ["self", "points"])):
        sig = inspect.signature(cls.insert_points)
        assert list(sig.parameters) == positional + ["transform", "segment"]
        for name in ("transform", "segment"):
            assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
            assert sig.parameters[name].default is None


# ---- the caller's own plug types -----------------------------------------------------------------------------------
def _leaves(obj, pose):
    return sorted((tuple(v.corner_min.tolist()), float(v.edge_length), v.get_points().tobytes())
                  for v in obj.get_leaf_points(pose_number=pose))


def test_plug_manager_under_a_transform_equals_the_transformed_cloud():
    rng = np.random.default_rng(5)
    A, B = rng.uniform(-1, 1, (800, 3)), rng.uniform(-1, 1, (600, 3)).astype(np.float32)
    Ts = _transforms(3, 6) * 1.0
    Ts[:, :3, 3] *= 0.1
    seg = rng.integers(0, 3, len(B))

    def run(twin):
        m = HostManager(HostOctree, OctreeConfigBase(), np.array([-4.0, -4.0, -4.0]), 8.0)
        assert m._plug is not None
        if twin:
            m.insert_points(0, transform_rows_np(Ts[0], A))
            m.insert_points(1, transform_rows_np(Ts, B, seg))
        else:
            m.insert_points(0, A, transform=Ts[0])
            m.insert_points(1, B, transform=Ts, segment=seg)
        m.subdivide([MaxPoints(25)])
        return [m.get_points(p).tobytes() for p in (0, 1)], [_leaves(m, p) for p in (0, 1)]

    assert run(False) == run(True)
    m = HostManager(HostOctree, OctreeConfigBase(), np.zeros(3), 8.0)
    with pytest.raises(ValueError, match="segment is given without transforms"):
        m.insert_points(0, A, segment=np.zeros(len(A), dtype=np.int64))
    with pytest.raises(ValueError, match=r"segment entries must lie in \[0, 3\)"):
        m.insert_points(0, B, transform=Ts, segment=seg + 1)


def test_plug_grid_is_handed_the_transformed_cloud(monkeypatch):
    """The plug path of Grid.insert_points buckets a pose on the device; here that step is replaced by NumPy (as
    tests/test_cpu_query.py does), so that what the plug's managers receive can be compared without a GPU."""
    from octreelib_amd.grid._plugged import PluggedGrid

    def host_insert(self, pose, points):
        P = nat.as_points(points)
        vox = (np.floor_divide(P, 2.0) * 2).astype(int)
        uniq, inv = np.unique(vox, axis=0, return_inverse=True)
        self._pose_voxels[pose] = []
        for j, coords in enumerate(uniq):
            key = tuple(int(c) for c in coords)
            if key not in self._managers:
                self._managers[key] = HostManager(HostOctree, OctreeConfigBase(), np.array(coords), 2)
            self._pose_voxels[pose].append(key)
            self._managers[key].insert_points(pose, P[inv.reshape(-1) == j])

    monkeypatch.setattr(PluggedGrid, "insert_points", host_insert)
    rng = np.random.default_rng(8)
    A, B = rng.uniform(0, 4, (900, 3)), rng.uniform(0, 4, (700, 3)).astype(np.float32)
    Ts = _transforms(2, 10)
    seg = np.sort(rng.integers(0, 2, len(B)))

    def run(twin):
        g = Grid(GridConfig(octree_manager_type=HostManager, octree_type=HostOctree, octree_config=OctreeConfigBase(),
                            voxel_edge_length=2))
        assert g._plug is not None
        if twin:
            g.insert_points(0, transform_rows_np(Ts[1], A))
            g.insert_points(1, transform_rows_np(Ts, B, seg))
        else:
            g.insert_points(0, A, transform=Ts[1])
            g.insert_points(1, B, transform=Ts, segment=seg)
        g.subdivide([MaxPoints(30)])
        return [g.get_points(p).tobytes() for p in (0, 1)], [
            sorted((tuple(v.corner_min.tolist()), float(v.edge_length), v.get_points().tobytes())
                   for v in g.get_leaf_points(p)) for p in (0, 1)]

    assert run(False) == run(True)
