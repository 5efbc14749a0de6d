"""transform_poses without a GPU: the entry is declared, bound with the declared arity and exported by the
cross-compiled library; Grid and OctreeManager have the method; the caller's own plug types are refused by name; the
kernel's rows per workgroup are what tests/test_gpu_transform_poses.py sizes its poses by."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from octreelib_amd import _native as nat
from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree
from octreelib_amd.octree.octree_base import OctreeConfigBase
from octreelib_amd.octree_manager import OctreeManager

from tests.test_cpu_query import HostManager, HostOctree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "octl_forest_transform_poses"
DECL = ("int octl_forest_transform_poses(octl_forest* f, const uint8_t* slot_sel, int32_t n_sel, "
        "const double* transforms);")


def test_entry_declared_and_in_signature_table():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "octreelib_hip.h")).read())
    assert DECL in header
    assert "#define OCTL_ABI_VERSION 1" in header
    res, args = nat.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == DECL.count(",") + 1
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert NAME in integration


def test_library_exports_the_entry():
    lib = nat.load()     # (loading does not touch the GPU)
    assert hasattr(lib, NAME)
    assert lib.octl_forest_transform_poses.argtypes == nat.SIGNATURES[NAME][1]
    assert lib.octl_abi_version() == 1


def test_methods_and_their_signatures():
    for cls in (Grid, OctreeManager):
        sig = inspect.signature(cls.transform_poses)
        assert list(sig.parameters) == ["self", "transforms", "pose_numbers"]
        assert sig.parameters["pose_numbers"].default is None
        assert sig.parameters["transforms"].default is inspect.Parameter.empty
    assert not hasattr(Octree, "transform_poses")
    for cls in (Grid, OctreeManager):     # the adjust docstrings point at it
        assert "transform_poses" in cls.adjust.__doc__
    import octreelib_amd.adjustment as adjustment

    assert "transform_poses" in adjustment.__doc__


def test_plug_types_are_refused():
    g = Grid(GridConfig(octree_manager_type=HostManager, octree_type=HostOctree, octree_config=OctreeConfigBase(),
                        voxel_edge_length=2))
    assert g._plug is not None
    with pytest.raises(NotImplementedError, match="plug types"):
        g.transform_poses([np.eye(4)])
    m = OctreeManager(HostOctree, OctreeConfigBase(), np.zeros(3), 4.0)
    m.insert_points(0, np.random.default_rng(1).random((50, 3)))
    with pytest.raises(NotImplementedError, match="plug types"):
        m.transform_poses([np.eye(4)], pose_numbers=[0])


def test_rows_per_workgroup_is_what_the_gpu_test_assumes():
    src = open(os.path.join(ROOT, "octreelib_amd", "csrc", "store.hip")).read()
    pairs = int(re.search(r"constexpr int XF_PAIRS = (\d+);", src).group(1))
    assert "constexpr int XF_ROWS_PER_WG = 256 * 2 * XF_PAIRS;" in src
    from tests.test_gpu_transform_poses import ROWS_PER_WG

    assert ROWS_PER_WG == 256 * 2 * pairs
