"""What the neighbourhood tests share: the derived bound of DESIGN.md 4.23 checked against exact rational moments (or
against the longdouble definition where a neighbourhood is too large for them), the neighbours of a query by
radius_count_np's own arithmetic, and - for the CPU tests - the stand-alone host build of the kernels' row
(tests/host/moments_host.cpp) over the tables of a HostMap (tests/_cell.py: host_tables)."""

import os
import subprocess
from fractions import Fraction

import numpy as np

from octreelib_amd.leaf_stats import LeafStatistics, cov6_to_full
from octreelib_amd.neighbourhood import _neighbour_lists
from octreelib_amd.query import HostMap
from tests._cell import host_tables
from tests._raycast import ROOT

EPS = 2.0 ** -53


def neighbours_of(Q, clouds, radius):
    """One (n_i, 3) float64 array per query: the stored points the definition selects."""
    return _neighbour_lists(Q, clouds, radius, "neighbourhood_statistics")[1]


def gamma(n):
    return (n + 16) * EPS


def exact_moments(P):
    """(mean [3], covariance [3][3]) of the rows of P as Fractions: the exact population moments of the f64 rows."""
    rows = [[Fraction(float(v)) for v in row] for row in np.asarray(P, dtype=np.float64).tolist()]
    n = len(rows)
    mean = [sum(r[a] for r in rows) / n for a in range(3)]
    cov = [[sum((r[a] - mean[a]) * (r[b] - mean[b]) for r in rows) / n for b in range(3)] for a in range(3)]
    return mean, cov


def radius_inf(P, q):
    """R = max |p - q|_inf over the rows of P, exactly."""
    qf = [Fraction(float(v)) for v in q]
    return max(abs(Fraction(float(v)) - qf[a]) for row in np.asarray(P).tolist() for a, v in enumerate(row))


def assert_exact_bound(st: LeafStatistics, Q, lists, rows, what):
    """The rows `rows` of st against exact rational moments of their neighbours: count exact, every mean component
    within 2 g R + eps |m|, every covariance entry within 4 g R^2, g = (n + 16) eps.  Returns the largest ratio
    error / bound seen (mean, covariance) - printed by the callers, never asserted on."""
    worst_m = worst_c = 0.0
    for i in rows:
        P = lists[i]
        n = len(P)
        assert int(st.count[i]) == n, (what, i, int(st.count[i]), n)
        assert n >= 1, (what, i)
        mean, cov = exact_moments(P)
        R = radius_inf(P, Q[i])
        g = Fraction(gamma(n))
        for a in range(3):
            err = abs(Fraction(float(st.mean[i, a])) - mean[a])
            bound = 2 * g * R + Fraction(EPS) * abs(mean[a])
            assert err <= bound, (what, "mean", i, a, n, float(err), float(bound))
            if bound > 0:
                worst_m = max(worst_m, float(err / bound))
        for a in range(3):
            for b in range(3):
                err = abs(Fraction(float(st.covariance[i, a, b])) - cov[a][b])
                bound = 4 * g * R * R
                assert err <= bound, (what, "cov", i, a, b, n, float(err), float(bound))
                if bound > 0:
                    worst_c = max(worst_c, float(err / bound))
    return worst_m, worst_c


def assert_reference_bound(st: LeafStatistics, ref: LeafStatistics, Q, lists, rows, what, rounded=False):
    """The same bound against a reference of higher precision (the longdouble definition) for rows too large for
    rationals; the reference's own error, about n 2^-64 R^2, is three orders below the bound.  rounded: the reference
    was rounded to float64 afterwards (HostMap returns float64), which moves each value by half an ulp at most:
    eps |value| is added."""
    for i in rows:
        P = np.asarray(lists[i], dtype=np.longdouble)
        n = len(P)
        assert int(st.count[i]) == n == int(ref.count[i]), (what, i)
        R = np.abs(P - np.asarray(Q[i], dtype=np.longdouble)).max()
        g = np.longdouble(gamma(n))
        em = np.abs(st.mean[i].astype(np.longdouble) - ref.mean[i])
        extra = EPS if rounded else 0.0
        assert np.all(em <= 2 * g * R + (EPS + extra) * np.abs(ref.mean[i])), (what, "mean", i, n, em)
        ec = np.abs(st.covariance[i].astype(np.longdouble) - ref.covariance[i])
        assert np.all(ec <= 4 * g * R * R + extra * np.abs(ref.covariance[i])), (what, "cov", i, n, ec.max())


def pick_rows(count, limit=64, max_n=100):
    """At most `limit` rows with 1 <= count <= max_n, spread over the counts that occur (the largest ones first)."""
    idx = np.nonzero((count >= 1) & (count <= max_n))[0]
    idx = idx[np.argsort(-count[idx], kind="stable")]
    if len(idx) > limit:
        idx = idx[np.unique(np.linspace(0, len(idx) - 1, limit).astype(np.int64))]
    return [int(i) for i in idx]


# ---- the kernels' row on the host --------------------------------------------------------------------------------------
def build_host_program(directory):
    """tests/host/moments_host.cpp compiled for the CPU alone with AddressSanitizer and UBSan (the compile line of
    tests/_cell.py: build_host_program); returns the program."""
    exe = os.path.join(str(directory), "moments_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "octreelib_amd", "csrc"), os.path.join(ROOT, "tests", "host", "moments_host.cpp"),
           "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def run_host_program(exe, directory, hm: HostMap, Q, radius, eigen=True, pose_numbers=None, tables=None):
    """The rows of the host build for the queries Q over the tables of `hm`: a LeafStatistics."""
    t = host_tables(hm, pose_numbers) if tables is None else tables
    Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, 3)
    n = len(Q)
    nodes = hm.nodes
    head = np.array([hm.mode, len(t["vcode"]), len(t["fc"]), len(t["rec"]), len(t["ord_idx"]), n, int(eigen),
                     *t["org"]], dtype=np.int64)
    src, dst = os.path.join(str(directory), "moments.in"), os.path.join(str(directory), "moments.out")
    with open(src, "wb") as f:
        for a, dt in ((head, np.int64), ([hm.edge, radius], np.float64), (t["vcode"], np.uint64), (t["fc"], np.int32),
                      (t["parent"], np.int32), (nodes["corner"], np.float64), (nodes["edge"], np.float64),
                      (t["first"], np.int32), (t["cnt"], np.int32), (t["rec"], np.uint32), (t["xyz_ord"], np.float64),
                      (t["ord_idx"], np.uint32), (Q, np.float64)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-4000:])
    raw = open(dst, "rb").read()
    assert len(raw) == n * (8 + 8 * (9 + (12 if eigen else 0)))
    count = np.frombuffer(raw, np.int64, n).copy()
    body = np.frombuffer(raw, np.float64, offset=8 * n)
    mean, cov = body[:3 * n].reshape(n, 3).copy(), body[3 * n:9 * n].reshape(n, 6).copy()
    w = body[9 * n:12 * n].reshape(n, 3).copy() if eigen else None
    v = body[12 * n:21 * n].reshape(n, 3, 3).copy() if eigen else None
    return LeafStatistics(count, mean, cov6_to_full(cov), w, v)
