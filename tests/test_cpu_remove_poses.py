"""remove_poses without a GPU: the two entries are declared, bound with the declared arity and exported by the
cross-compiled library; Grid and OctreeManager have the method and Octree does not; the caller's own plug types and an
unknown pose are refused before anything reaches the device; the store kernel's rows per workgroup are the 2048 that
tests/test_gpu_remove_poses.py sizes its poses by (read from store.hip: no test module imports another for it)."""

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
DECLS = {
    "octl_forest_remove_poses": ("int octl_forest_remove_poses(octl_forest* f, const uint8_t* slot_sel, int32_t n_sel, "
                                 "int32_t* new_slot, int64_t* n_removed);"),
    "octl_forest_store_size": ("int octl_forest_store_size(octl_forest* f, int64_t* n_store, int64_t* n_alive, "
                               "int32_t* n_poses);"),
}


def test_entries_declared_and_in_signature_table():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "octreelib_hip.h")).read())
    assert "#define OCTL_ABI_VERSION 1" in header
    for name, decl in DECLS.items():
        assert decl in header
        res, args = nat.SIGNATURES[name]
        assert res is C.c_int and len(args) == decl.count(",") + 1


def test_library_exports_the_entries():
    lib = nat.load()     # (loading does not touch the GPU)
    for name in DECLS:
        assert hasattr(lib, name)
        assert getattr(lib, name).argtypes == nat.SIGNATURES[name][1]
    assert lib.octl_abi_version() == 1
    # a NULL forest is refused before anything looks at a device
    assert lib.octl_forest_remove_poses(None, None, 0, None, None) == nat.OCTL_E_INVALID
    assert lib.octl_forest_store_size(None, None, None, None) == nat.OCTL_E_INVALID


def test_methods_and_their_signatures():
    for cls in (Grid, OctreeManager):
        sig = inspect.signature(cls.remove_poses)
        assert list(sig.parameters) == ["self", "pose_numbers"]
        assert sig.parameters["pose_numbers"].default is inspect.Parameter.empty
    assert not hasattr(Octree, "remove_poses")


def test_plug_types_are_refused():
    g = Grid(GridConfig(octree_manager_type=HostManager, octree_type=HostOctree, octree_config=OctreeConfigBase(),
                        voxel_edge_length=2))
    assert g._plug is not None
    with pytest.raises(ValueError, match="plug types"):
        g.remove_poses([0])
    m = OctreeManager(HostOctree, OctreeConfigBase(), np.zeros(3), 4.0)
    m.insert_points(0, np.random.default_rng(1).random((50, 3)))
    with pytest.raises(ValueError, match="plug types"):
        m.remove_poses([0])


class _NoDevice:
    """Stands where the forest would: an unknown pose must be refused before the forest is asked for anything."""

    def __getattr__(self, name):
        raise AssertionError(f"the forest was asked for {name}")


@pytest.mark.parametrize("cls", [Grid, OctreeManager])
def test_unknown_pose_is_a_key_error_as_for_get_points(cls):
    obj = cls.__new__(cls)
    obj._plug, obj._slots, obj._forest = None, {3: 0, 5: 1}, _NoDevice()
    with pytest.raises(KeyError):
        obj.remove_poses([4])
    with pytest.raises(KeyError):
        obj.remove_poses([3, 4])
    assert obj._slots == {3: 0, 5: 1}


def test_rows_per_workgroup_is_what_the_gpu_test_assumes():
    src = open(os.path.join(ROOT, "octreelib_amd", "csrc", "store.hip")).read()
    units = int(re.search(r"constexpr int RT_UNITS = (\d+);", src).group(1))
    assert "constexpr int RT_ROWS_PER_WG = 256 * RT_UNITS * 2 / 3;" in src
    # tests/test_gpu_remove_poses.py reads RT_UNITS the same way and sizes its poses for 2048 rows per workgroup
    assert 256 * units * 2 // 3 == 2048
