"""Helpers shared by the parity tests: canonical forms of leaf tables."""

import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name))


def canon(corners, edges, sizes, idx):
    """(corners (Lf,3) f64, edges (Lf,), sizes (Lf,), concatenated idx) ->
    ordered list of ((corner bytes, edge bytes), tuple(sorted idx))."""
    corners = np.ascontiguousarray(corners, dtype=np.float64).reshape(-1, 3)
    edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    out = []
    for i in range(len(edges)):
        # +0.0 normalises a possible -0.0 corner coordinate
        key = ((corners[i] + 0.0).tobytes(), edges[i].tobytes())
        out.append((key, tuple(sorted(int(v) for v in idx[off[i] : off[i + 1]]))))
    return out


def canon_from_list(table):
    """list of (corner, edge, idx) -> same canonical form."""
    out = []
    for corner, edge, idx in table:
        key = ((np.asarray(corner, dtype=np.float64) + 0.0).tobytes(), np.float64(edge).tobytes())
        out.append((key, tuple(sorted(int(v) for v in idx))))
    return out


def golden_canon(g, prefix):
    return canon(g[f"{prefix}_corners"], g[f"{prefix}_edges"], g[f"{prefix}_sizes"], g[f"{prefix}_idx"])


def assert_same_leaves(got, want, ordered=True):
    """Exact equality of the leaf map (corner bits, edge bits) -> index set, and of the
    list order when ordered=True."""
    assert len(got) == len(want), f"{len(got)} leaves, expected {len(want)}"
    assert dict(got) == dict(want)
    if ordered:
        assert [k for k, _ in got] == [k for k, _ in want]


def set_option(name, value=1):
    """A diagnostic switch of the process-wide context (octl_debug_set_option: the library reads its OCTL_* environment
    only when a context is created).  tests/conftest.py resets every touched switch after each test."""
    from octreelib_amd import _native as nat

    nat.get_context().set_option(name, value)


# ---- oracle scheme nodes and the NotPlanar statistic (shared by test_gpu_planarity.py and the operation-sequence tests)
EPS = 2.0 ** -53


def _descend(node, points, idx, out):
    """(corner, edge, internal, idx) of every node below `node`, with the oracle's own child arithmetic."""
    out.append((np.asarray(node.corner, dtype=np.float64), float(node.edge), node.children is not None, idx))
    if node.children is None:
        return
    d = ((points[idx] - node.corner) // (node.edge / 2)).astype(int)
    child = 4 * d[:, 0] + 2 * d[:, 1] + d[:, 2]
    for j, ch in enumerate(node.children):
        _descend(ch, points, idx[child == j], out)


def _scheme_nodes(scheme_tree, points=None):
    pts = scheme_tree.points if points is None else points
    out = []
    _descend(scheme_tree.root, pts, np.arange(len(pts)), out)
    return pts, out


def _oracle_nodes(scheme_trees, crit, K):
    """Every node of the oracle's scheme trees as key -> (edge, n, lambda, internal, rows), after asserting the
    scene's condition: nothing evaluated within 1e-9 e^2 of the threshold, and the tree is what the predicate says."""
    nodes, closest, evaluated = {}, math.inf, 0
    for t in scheme_trees:
        pts, lst = _scheme_nodes(t)
        for corner, e, internal, idx in lst:
            rows = pts[idx]
            lam = crit.smallest_eigenvalue(rows)
            if len(idx) >= crit.min_points:
                evaluated += 1
                closest = min(closest, abs(lam - crit.max_variance) / (e * e))
            assert internal == (len(idx) > K >= 0 or (len(idx) >= crit.min_points and lam > crit.max_variance))
            nodes[((corner + 0.0).tobytes(), e)] = (e, len(idx), lam, internal, rows)
    assert closest > 1e-9, f"scene unusable: a statistic lies {closest:.3g} e^2 from the threshold"
    return nodes, evaluated


def _longdouble_lambda(rows, ddof):
    p = np.asarray(rows, dtype=np.longdouble)
    d = p - p.sum(axis=0) / len(p)
    cov = np.array([[(d[:, a] * d[:, b]).sum() for b in range(3)] for a in range(3)]) / (len(p) - ddof)
    # the smallest root of the characteristic cubic, refined in longdouble from LAPACK's f64 value
    c = cov.astype(np.float64)
    s = 1.0 / max(np.abs(c).max(), 1e-300)
    lam = np.longdouble(np.linalg.eigvalsh(c * s)[0] / s)
    a, b, cc, dd, e, f = cov[0, 0], cov[0, 1], cov[0, 2], cov[1, 1], cov[1, 2], cov[2, 2]
    fro = np.sqrt((cov * cov).sum())
    for _ in range(4):   # (a Newton step is taken only where it is a refinement: not across a near-double root)
        x, y, z = a - lam, dd - lam, f - lam
        det = x * (y * z - e * e) - b * (b * z - e * cc) + cc * (b * e - y * cc)
        ddet = -((y * z - e * e) + (x * z - cc * cc) + (x * y - b * b))
        if ddet == 0 or abs(det / ddet) > 16 * EPS * fro:
            break
        lam = lam - det / ddet
    return float(lam), float(np.sqrt((cov * cov).sum()))
