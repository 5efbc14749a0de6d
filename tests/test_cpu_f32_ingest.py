"""CPU-only checks of the float32 input path: the four f32 entry points are declared, exported and bound, and
_native.as_points_native keeps float32 clouds in float32 (everything else goes through as_points' f64 upcast)."""

import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F32_ENTRIES = {
    "octl_forest_add_pose_f32": "int octl_forest_add_pose_f32(octl_forest* f, const float* xyz, int64_t n, int32_t* slot)",
    "octl_forest_add_pose_device_f32":
        "int octl_forest_add_pose_device_f32(octl_forest* f, const float* xyz_dev, int64_t n, int32_t* slot)",
    "octl_forest_extend_pose_f32":
        "int octl_forest_extend_pose_f32(octl_forest* f, int32_t slot, const float* xyz, int64_t n)",
    "octl_forest_extend_pose_device_f32":
        "int octl_forest_extend_pose_device_f32(octl_forest* f, int32_t slot, const float* xyz_dev, int64_t n)",
}


def _header():
    text = open(os.path.join(ROOT, "include", "octreelib_hip.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_f32_entries_are_declared_exported_and_bound():
    from octreelib_amd import _native as nat

    header = _header()
    lib = nat.load()
    for name, decl in F32_ENTRIES.items():
        assert decl + ";" in header, f"{name} is not declared as `{decl}`"
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = nat.SIGNATURES[name]
        assert res is C.c_int
        assert getattr(lib, name).argtypes == args
    p, i32, i64, pi32 = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_int32)
    assert nat.SIGNATURES["octl_forest_add_pose_f32"][1] == [p, p, i64, pi32]
    assert nat.SIGNATURES["octl_forest_add_pose_device_f32"][1] == [p, p, i64, pi32]
    assert nat.SIGNATURES["octl_forest_extend_pose_f32"][1] == [p, i32, p, i64]
    assert nat.SIGNATURES["octl_forest_extend_pose_device_f32"][1] == [p, i32, p, i64]
    assert lib.octl_abi_version() == 1   # (additive entries: the ABI version stays)


def test_as_points_native_keeps_f32():
    from octreelib_amd import _native as nat

    rng = np.random.default_rng(0)
    a = rng.normal(size=(7, 3)).astype(np.float32)
    got = nat.as_points_native(a)
    assert got.dtype == np.float32 and got.shape == (7, 3) and got.flags.c_contiguous
    assert got.tobytes() == a.tobytes()
    assert np.shares_memory(got, a)   # (already the right layout: no copy)
    # a view that starts at row 1 is C-contiguous already (only 4-byte aligned: the library copes)
    big = rng.normal(size=(9, 3)).astype(np.float32)
    got = nat.as_points_native(big[1:])
    assert got.dtype == np.float32 and np.shares_memory(got, big) and got.tobytes() == big[1:].tobytes()


@pytest.mark.parametrize("layout", ["strided", "fortran", "columns"])
def test_as_points_native_makes_f32_views_contiguous_without_changing_a_bit(layout):
    from octreelib_amd import _native as nat

    rng = np.random.default_rng(1)
    base = rng.normal(size=(11, 6)).astype(np.float32)
    base[0, 0] = np.float32(-0.0)
    base[1, 1] = np.float32(1e-42)      # subnormal
    base[2, 2] = np.nextafter(np.float32(3), np.float32(4))
    if layout == "strided":
        view = base[::2, :3]
    elif layout == "fortran":
        view = np.asfortranarray(base[:, :3])
    else:
        view = base[:, 1:6:2]
    assert not view.flags.c_contiguous
    got = nat.as_points_native(view)
    assert got.dtype == np.float32 and got.flags.c_contiguous and got.shape == view.shape
    assert got.view(np.uint32).tolist() == np.ascontiguousarray(view).view(np.uint32).tolist()


@pytest.mark.parametrize("kind", ["list", "f16", "int32", "int64", "f64", "f32_big_endian"])
def test_as_points_native_upcasts_everything_else_to_f64(kind):
    from octreelib_amd import _native as nat

    rows = [[0, 1, 2], [3, 4, 5], [-6, 7, 8]]
    src = {
        "list": rows,
        "f16": np.array(rows, dtype=np.float16),
        "int32": np.array(rows, dtype=np.int32),
        "int64": np.array(rows, dtype=np.int64),
        "f64": np.array(rows, dtype=np.float64),
        "f32_big_endian": np.array(rows, dtype=">f4"),
    }[kind]
    got = nat.as_points_native(src)
    want = nat.as_points(src)
    assert got.dtype == np.float64 and got.flags.c_contiguous
    assert got.tobytes() == want.tobytes()


def test_as_points_native_shapes():
    from octreelib_amd import _native as nat

    for bad in (np.zeros((4, 2), dtype=np.float32), np.zeros((4, 2))):
        with pytest.raises(ValueError) as e:
            nat.as_points_native(bad)
        with pytest.raises(ValueError) as want:
            nat.as_points(np.zeros((4, 2)))
        assert str(e.value) == str(want.value) == "expected an (n, 3) point cloud, got shape (4, 2)"
    with pytest.raises(ValueError, match=r"got shape \(6,\)"):
        nat.as_points_native(np.zeros(6, dtype=np.float32))
    empty = nat.as_points_native(np.zeros((0, 3), dtype=np.float32))
    assert empty.shape == (0, 3) and empty.dtype == np.float32
    assert nat.as_points_native(np.zeros(0, dtype=np.float32)).shape == (0, 3)
