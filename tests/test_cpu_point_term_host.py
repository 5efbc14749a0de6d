"""The per-point term of the point-to-point registration system (octreelib_amd/csrc/reg_point_term.h - the code
k_regp_partial runs) compiled for the CPU alone, with AddressSanitizer and UBSan, as the stand-alone program
tests/host/point_term_host.cpp, and compared BIT FOR BIT with an emulation of the operation order the header documents:
every plain operation one IEEE f64 operation (Python's float arithmetic is exactly that), every fma ONE rounding of
the exact a b + c, formed in fractions.Fraction.  No GPU and nothing loaded into Python: the program reads and writes
files.  This test is about that program: it compiles it once (a few seconds) and starts it once."""

import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("point_term_host")
    exe = os.path.join(str(d), "point_term_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "octreelib_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "point_term_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe, d


def fma(a, b, c):
    """One rounding of the exact a b + c (float(Fraction) rounds to nearest even); a zero keeps IEEE's sign."""
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    return float(exact) if exact != 0 else a * b + c


def term(S, p, m, c, delta):
    """The documented order of reg_point_term, entered into the 17 sums S."""
    e = [p[i] - m[i] for i in range(3)]
    d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    delta = delta if delta > 0.0 else 0.0
    delta2 = delta * delta
    dx, dy, dz = (p[i] - c[i] for i in range(3))
    tail = delta > 0.0 and d2 > delta2
    w, rho = 1.0, 0.5 * d2
    if tail:
        s = math.sqrt(d2)
        w = delta / s
        rho = delta * (s - 0.5 * delta)
    wdx, wdy, wdz = w * dx, w * dy, w * dz
    wex, wey, wez = w * e[0], w * e[1], w * e[2]
    yy, zz = wdy * dy, wdz * dz
    S[0] += fma(wdy, dy, zz)
    S[1] += fma(wdx, dx, zz)
    S[2] += fma(wdx, dx, yy)
    S[3] = fma(-wdx, dy, S[3])
    S[4] = fma(-wdx, dz, S[4])
    S[5] = fma(-wdy, dz, S[5])
    S[6] += wdx
    S[7] += wdy
    S[8] += wdz
    S[9] += w
    S[10] += fma(wdy, e[2], -(wdz * e[1]))
    S[11] += fma(wdz, e[0], -(wdx * e[2]))
    S[12] += fma(wdx, e[1], -(wdy * e[0]))
    S[13] += wex
    S[14] += wey
    S[15] += wez
    S[16] += rho
    return tail


def expand(S):
    X, Y, Z, W = S[6], S[7], S[8], S[9]
    return [S[0], S[3], S[4], 0.0, 0.0 - Z, Y,
            S[1], S[5], Z, 0.0, 0.0 - X,
            S[2], 0.0 - Y, X, 0.0,
            W, 0.0, 0.0,
            W, 0.0,
            W,
            S[10], S[11], S[12], S[13], S[14], S[15], S[16]]


def tuples():
    """(p, m, c, delta) rows: random matches with and without Huber weights (both branches), e = 0, an origin at UTM
    scale, d2 exactly on delta^2 (an inlier: the test is d2 > delta2), and the same far from the origin."""
    rng = np.random.default_rng(11)
    n = 300
    m = rng.uniform(-3.0, 3.0, (n, 3))
    p = m + rng.normal(0.0, 0.03, (n, 3))
    c = rng.uniform(-1.0, 1.0, (n, 3))
    delta = np.where(rng.random(n) < 0.3, 0.0, rng.uniform(0.005, 0.1, n))
    p[:20] = m[:20]                                   # e = 0
    utm = np.array([5.0e6, 4.0e5, 100.0])
    m[40:120] += utm
    p[40:120] += utm
    c[40:120] = utm + rng.uniform(-1.0, 1.0, (80, 3))
    c[120:140] = 0.0                                  # (UTM points about the origin 0: d is huge)
    m[120:140] += utm
    p[120:140] = m[120:140] + rng.normal(0.0, 0.03, (20, 3))
    p[140:150] = m[140:150] + np.array([3.0, 4.0, 12.0]) / 256.0      # d2 = 169 / 65536 exactly ...
    delta[140:145] = 13.0 / 256.0                                      # ... on delta^2: an inlier
    delta[145:150] = 13.0 / 512.0                                      # ... beyond it: w = 1 / 2
    m[140:150] = np.round(m[140:150] * 64.0) / 64.0
    p[140:150] = m[140:150] + np.array([3.0, 4.0, 12.0]) / 256.0
    return np.ascontiguousarray(np.concatenate([p, m, c, delta[:, None]], axis=1))


def test_rows_equal_the_documented_order_bit_for_bit(program):
    exe, d = program
    rows = tuples()
    src, dst = os.path.join(str(d), "in.bin"), os.path.join(str(d), "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(rows)], dtype=np.int64).tobytes())
        f.write(rows.tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-4000:])
    got = np.fromfile(dst, dtype=np.float64).reshape(len(rows) + 1, 28)
    want, total, tails = [], [0.0] * 17, 0
    for r in rows.tolist():
        one = [0.0] * 17
        tails += term(one, r[0:3], r[3:6], r[6:9], r[9])
        term(total, r[0:3], r[3:6], r[6:9], r[9])
        want.append(expand(one))
    want.append(expand(total))
    want = np.array(want, dtype=np.float64)
    assert 40 < tails < len(rows) - 40                       # both Huber branches
    assert tails == int((got[:-1, 15] != 1.0).sum())          # (H_vv of a lone term is its weight)
    bad = np.nonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))[0]
    assert len(bad) == 0, (bad[:5], got[bad[0]], want[bad[0]])
    assert np.all(got[:20, 21:27] == 0.0) and np.all(got[:20, 27] == 0.0)          # e = 0: no gradient, no cost
    assert np.all(got[140:145, 15] == 1.0) and np.all(got[145:150, 15] == 0.5)      # on the threshold / beyond it
    for k in (3, 9, 14, 16, 17, 19):                                                 # structural zeros are +0.0
        assert not got[:, k].any() and not np.signbit(got[:, k]).any()
    assert np.array_equal(got[:, 15], got[:, 18]) and np.array_equal(got[:, 15], got[:, 20])
    assert np.array_equal(got[:, 4], -got[:, 8]) and np.array_equal(got[:, 10], -got[:, 13])


def test_empty_input(program):
    exe, d = program
    src, dst = os.path.join(str(d), "in0.bin"), os.path.join(str(d), "out0.bin")
    with open(src, "wb") as f:
        f.write(np.array([0], dtype=np.int64).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    got = np.fromfile(dst, dtype=np.float64)
    assert got.shape == (28,) and not got.any() and not np.signbit(got).any()
