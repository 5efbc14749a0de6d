"""CPU-only checks of the per-leaf statistics: the host reference leaf_statistics_np against exact arithmetic,
LeafStatistics' derived properties, and the two new C entries in the header and _native.py's signature table."""

import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from octreelib_amd.leaf_stats import (LeafStatistics, cov6_to_full, leaf_statistics_np, leaf_statistics_of_leaves,
                                      orient_eigenvectors)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
_UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))

ENTRIES = {
    "octl_forest_leaf_stats": "int octl_forest_leaf_stats(octl_forest* f, const int32_t* block_ids, int64_t nb, "
                              "int64_t* count, double* mean, double* cov, double* eigval, double* eigvec)",
    "octl_debug_sym3_eigen": "int octl_debug_sym3_eigen(octl_ctx* ctx, const double* cov6, int64_t n, double* eigval, "
                             "double* eigvec)",
}


def _exact(P):
    rows = [[Fraction(float(x)) for x in p] for p in np.asarray(P, dtype=np.float64)]
    n = len(rows)
    m = [sum(r[a] for r in rows) / n for a in range(3)]
    c = [sum((r[i] - m[i]) * (r[j] - m[j]) for r in rows) / n for i, j in _UPPER]
    return m, c


def _blocks():
    rng = np.random.default_rng(5)
    out = [rng.random((n, 3)) for n in (1, 2, 3, 17, 64)]
    out.append(np.full((9, 3), 0.1))                                               # coincident points
    out.append(rng.random((40, 3)) * [1.0, 1.0, 1e-9] + 5.0e6)                     # thin plane at UTM magnitude
    out.append(np.array([[1e-300, -1e150, 0.0], [-1e-300, 1e150, -0.0]]))            # magnitudes far apart
    out.append(rng.standard_normal((33, 3)) * [1e-8, 1.0, 1e8])
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_host_reference_against_fractions(dtype):
    blocks = _blocks()
    st = leaf_statistics_np(blocks, dtype=dtype)
    assert st.count.tolist() == [len(b) for b in blocks]
    unit = EPS if dtype is np.float64 else float(np.finfo(np.longdouble).eps)
    for i, P in enumerate(blocks):
        m, c = _exact(P)
        n = len(P)
        scale = float(np.abs(P).max())
        for a in range(3):
            assert abs(Fraction(float(st.mean[i, a])) - m[a]) <= Fraction(4 * n * unit * scale + EPS * abs(float(m[a])))
        for k, (a, b) in enumerate(_UPPER):
            err = abs(Fraction(float(st.covariance[i, a, b])) - c[k])
            assert err <= Fraction(8 * n * unit * scale * scale + EPS * abs(float(c[k]))), (i, k)


def test_host_reference_eigen_and_empty():
    blocks = _blocks()[:5] + [np.empty((0, 3))]
    st = leaf_statistics_np(blocks)
    assert st.count[-1] == 0 and np.all(st.mean[-1] == 0) and np.all(st.covariance[-1] == 0)
    w, v = st.eigenvalues, st.eigenvectors
    assert np.all(np.diff(w, axis=1) >= 0)
    for i in range(len(blocks)):
        assert np.allclose(st.covariance[i] @ v[i], v[i] * w[i], atol=1e-12)
        for col in range(3):
            x = v[i, :, col]
            assert x[np.argmax(np.abs(x))] > 0
    assert len(leaf_statistics_np([])) == 0


def test_derived_properties():
    # two leaves: a plane z = 2 (normal e_z), and a single point (all eigenvalues 0)
    mean = np.array([[1.0, 2.0, 2.0], [3.0, 3.0, 3.0]])
    cov = np.zeros((2, 3, 3))
    cov[0] = np.diag([4.0, 1.0, 0.0])
    w = np.array([[0.0, 1.0, 4.0], [0.0, 0.0, 0.0]])
    v = np.stack([np.eye(3)[:, [2, 1, 0]], np.eye(3)])
    st = LeafStatistics(np.array([10, 1]), mean, cov, w, v)
    assert np.array_equal(st.normal, [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    assert np.array_equal(st.offset, [-2.0, -3.0])   # normal . mean + offset = 0
    assert np.array_equal(st.surface_variation, [0.0, 0.0])
    st.eigenvalues = np.array([[1.0, 1.0, 1.0], [1.0, 2.0, 5.0]])
    assert np.allclose(st.surface_variation, [1 / 3, 1 / 8])
    assert len(st) == 2


def test_sign_rule_and_full_matrices():
    v = np.array([[[-1.0, 0.5, 0.0], [0.0, -0.5, -0.6], [0.0, 0.0, 0.6]]])
    orient_eigenvectors(v)
    assert np.array_equal(v[0][:, 0], [1.0, 0.0, 0.0])
    assert np.array_equal(v[0][:, 1], [0.5, -0.5, 0.0])      # tie: the lowest index is made positive
    assert np.array_equal(v[0][:, 2], [0.0, 0.6, -0.6])      # tie: index 1 was negative -> negated
    c = cov6_to_full(np.array([[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]]))
    assert np.array_equal(c[0], [[1, 2, 3], [2, 4, 5], [3, 5, 6]])


def test_host_path_of_leaves():
    class _Leaf:
        def __init__(self, p):
            self.p = p

        def get_points(self):
            return self.p

    blocks = _blocks()[:5]
    st = leaf_statistics_of_leaves([_Leaf(b) for b in blocks])
    assert st.mean.dtype == np.float64 and st.covariance.dtype == np.float64
    for i, P in enumerate(blocks):
        m, _ = _exact(P)
        for a in range(3):
            assert abs(Fraction(float(st.mean[i, a])) - m[a]) <= Fraction(EPS * abs(float(m[a])))


def _header():
    text = open(os.path.join(ROOT, "include", "octreelib_hip.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_entries_declared_and_in_signature_table():
    from octreelib_amd import _native as nat

    header = _header()
    for name, decl in ENTRIES.items():
        assert decl + ";" in header, f"{name} is not declared as `{decl}`"
        res, _ = nat.SIGNATURES[name]
        assert res is C.c_int
    p, i64 = C.c_void_p, C.c_int64
    assert nat.SIGNATURES["octl_forest_leaf_stats"][1] == [p, p, i64, p, p, p, p, p]
    assert nat.SIGNATURES["octl_debug_sym3_eigen"][1] == [p, p, i64, p, p]
    if os.path.exists(nat.lib_path()):
        lib = nat.load()
        for name in ENTRIES:
            assert getattr(lib, name).argtypes == nat.SIGNATURES[name][1]
        assert lib.octl_abi_version() == 1
