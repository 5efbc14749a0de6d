"""NumPy model of k_ransac's certified exit (octreelib_amd/csrc/plane_cert.h and "the certified exit" in
csrc/ransac.hip): used by tools/cert_exit_sim.py and, through tests/_plane_cert.py, by the tests - which also check it
against the header itself (tests/test_cpu_plane_cert.py).  float64 throughout; the kernel's f32 roundings of the block
constants are far inside the (1 + 2^-10) factors they carry."""
import numpy as np

U32 = 2.0 ** -24
UP = 1.0 + 2.0 ** -10


# ---- the block's constants (prescreen_constants of csrc/ransac.hip) ---------------------------------------------------
def block_constants(pts, thr):
    """(eligible, thrblk, E, G): the prescreen's eligibility of the block (range certificate taken for granted), the
    threshold the certificate uses as t, the extent and the coordinate bound."""
    o = pts[0]
    E = float(np.abs((pts - o).astype(np.float32)).max())
    G = float(np.abs(o).sum()) + E
    eblk = 64.0 * U32 * E + 2.0 ** -21 * G
    elig = 2.0 ** -7 <= E <= 2.0 ** 7 and 2.0 ** -40 <= thr <= 2.0 ** 40 and eblk * 8.0 <= thr
    return elig, (thr + eblk) * UP, E, G


# ---- plane_cert.h ---------------------------------------------------------------------------------------------------
def _exceeds(S, tr_full, m, t):
    if not (2.0 ** -200 < tr_full < 2.0 ** 200 and 2.0 ** -100 <= t <= 2.0 ** 100 and m >= 1):
        return False
    tr = S[0, 0] + S[1, 1] + S[2, 2]
    if not tr > 0.0:
        return False
    xx, xy, xz, yy, yz, zz = S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]
    det = (xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz)) + xz * (xy * yz - yy * xz)
    trb = tr + 2.0 ** -32 * tr_full
    return bool(4.0 * (det - 2.0 ** -30 * tr_full ** 3) > m * t * t * UP * trb * trb)


def _margin(S, tr_full, m, t):
    """Left over right side of the header's test (above 1: it holds)."""
    tr = S[0, 0] + S[1, 1] + S[2, 2]
    xx, xy, xz, yy, yz, zz = S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]
    det = (xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz)) + xz * (xy * yz - yy * xz)
    trb = tr + 2.0 ** -32 * tr_full
    return float(4.0 * (det - 2.0 ** -30 * tr_full ** 3) / (m * t * t * UP * trb * trb))


def scatter(pts):
    """S about the centroid and the centroid relative to the first point, from the raw sums as the header forms them."""
    r = pts - pts[0]
    n = len(pts)
    s1 = r.sum(0)
    c = s1 / n
    return r.T @ r - np.outer(s1, c), c


def no_plane_holds_all(pts, t):
    n = len(pts)
    if n < 3:
        return False
    S, _ = scatter(pts)
    return _exceeds(S, np.trace(S), n, t)


def margin_all(pts, t):
    """How far no_plane_holds_all is from its line: the test's left side over its right side."""
    S, _ = scatter(pts)
    return _margin(S, np.trace(S), len(pts), t)


def no_plane_holds_others(pts, t):
    """The leave-one-out test of every point: no plane holds n - 1 of the n points."""
    n = len(pts)
    if n < 4:
        return False
    S, c = scatter(pts)
    tr = np.trace(S)
    w = n / (n - 1.0)
    for q in (pts - pts[0]) - c:
        if not _exceeds(S - w * np.outer(q, q), tr, n - 1, t):
            return False
    return True


def certified(pts, thr, L):
    """The kernel's decision for a block whose best count of hypotheses 0..63 is L: None (not tested), False, True."""
    n = len(pts)
    elig, t, _, _ = block_constants(pts, thr)
    if not elig or n - L not in (1, 2):
        return None
    return no_plane_holds_all(pts, t) if n - L == 1 else no_plane_holds_others(pts, t)


# ---- the per-hypothesis test ------------------------------------------------------------------------------------------
def cross_floor(E, G):
    return (2.0 ** -24 * E ** 4 + 2.0 ** -74 * G * G * E * E) * (1.0 + 2.0 ** -15)


def vouched(pts, idx):
    """Which hypotheses (rows of the (h, k) sample positions `idx`, all < n) the cross-product test vouches for: the
    first sample, the first one at another position, the first one at a third."""
    _, _, E, G = block_constants(pts, 1.0)
    loc = (pts - pts[0]).astype(np.float32).astype(np.float64)
    h, k = idx.shape
    p0 = idx[:, 0]
    p1 = idx[:, k - 1].copy()
    for i in range(k - 2, 0, -1):
        p1 = np.where(idx[:, i] != p0, idx[:, i], p1)
    p2 = idx[:, k - 1].copy()
    for i in range(k - 2, 1, -1):
        p2 = np.where((idx[:, i] != p0) & (idx[:, i] != p1), idx[:, i], p2)
    c = np.cross(loc[p1] - loc[p0], loc[p2] - loc[p0])
    return (c * c).sum(1) > cross_floor(E, G)


# ---- a filter in front of the certificate (forecast only: the kernel has none yet) -------------------------------------
def filter_skips(pts, plane, t, b):
    """Whether the certificate of a block with n - L = b (1 or 2) cannot succeed, judged from the residuals r of the
    points against one plane (a, b, c, d) alone - the winner of group 0: with V = sum (r - mean r)^2 / |a|^2,
    lambda_min(S) <= V, and without point i lambda_min(S_i) <= V - n / (n - 1) (r_i - mean r)^2 / |a|^2; the header's
    test asks for 4 det / tr^2 <= lambda_min above m t^2 (1 + 2^-10).  Two wave sums instead of nine."""
    n = len(pts)
    nn = float((plane[:3] ** 2).sum())
    if nn == 0.0:
        return False
    r = ((plane[0] * pts[:, 0] + plane[1] * pts[:, 1]) + plane[2] * pts[:, 2]) + plane[3]
    d = r - r.mean()
    V = float((d * d).sum()) / nn
    if b == 1:
        return V <= n * t * t * UP
    return V - n / (n - 1.0) * float((d * d).max()) / nn <= (n - 1) * t * t * UP

