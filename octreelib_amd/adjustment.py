"""
Multi-pose plane adjustment on per-block moments: refine the transforms of the poses already in the map jointly, so
that the pooled points of every leaf become as flat as possible (the eigen-factor cost sum_l N_l lambda0_l / 2 of a
sliding-window plane adjustment).

The device reduces the map ONCE to 80 bytes per (leaf, pose) block - n, s = sum d, M = sum d d^T, d = x - a about the
leaf's centre a - and every iteration after that works on those moments, never on the points
(octl_forest_adjustment_system, csrc/adjust.hip); the 6x6 solves, the pose updates and the loop are NumPy on the host.
adjustment_system_np is the same on the host: the specification, the higher-precision reference of the tests, and what
the classes built on the caller's own plug types run through query.HostMap.

The transforms are increments applied to the points as they were inserted; leaf membership stays what the last build
made it until Grid.transform_poses / OctreeManager.transform_poses write the result back into the map (the points move
on the device, the map is then subdivided and fitted again).  With T_p = (R, t) of the block's pose, every line evaluated as written (dot products left to right):
  a'  = ((R_i0 a_x + R_i1 a_y) + R_i2 a_z) + t_i in f64 (transform_np),  delta = a' - a in f64
  s'  = R s,  M' = (R M) R^T                                   in `dtype` from here on
  s'' = s' + n delta,  M'' = ((M' + delta s'^T) + s' delta^T) + (n delta) delta^T     the moved points, still about a
  leaf: N, S, M = its selected blocks added in ascending pose order; mean m = a + S / N, C = M / N - (S / N)(S / N)^T,
        eigh(C) in f64 under the library's sign rule; normal = the smallest eigenvalue's vector, lambda0 that value
  used  = N >= min_points and non-empty selected blocks >= min_poses and lambda0 finite and (no max_variance or
          lambda0 <= max_variance)
  block of a used leaf, homogeneous coordinates x~ = (d, 1) with Q = [[M'', s''], [s''^T, n]]:
        r = pi^T x~, pi = (normal, normal . (a - m));  J = A x~, A = [[K, K e], [0, normal]], K v = v x normal,
        e = a - c:  J = [(x - c) x normal, normal], the derivative of r under x <- Rot(w)(x - c) + c + v (se3_exp)
        H += A Q A^T,  g += A Q pi,  cost += pi^T Q pi / 2      per pose, its blocks in ascending node id
Blocks of unused leaves are skipped.  g is the exact gradient of the eigen-factor cost (the plane minimises the same
quadratic form); H treats the planes as fixed and is block-diagonal, so adjust is a block-Jacobi iteration.
"""

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence

import numpy as np

from octreelib_amd.leaf_stats import cov6_to_full, orient_eigenvectors
from octreelib_amd.registration import _as_origin, _matrix, as_transform, se3_exp

__all__ = ["BlockMoments", "AdjustmentLeaves", "AdjustmentSystem", "Adjustment", "block_moments_np", "root_box_centre",
           "as_transforms", "adjustment_system_np", "adjust_np", "tree_depth"]

_TRIU = np.triu_indices(6)
_UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
CHUNK_BLOCKS = 1024


def tree_depth(n_blocks: int) -> int:
    """Additions a block's term can pass through on the device for a pose of n_blocks selected blocks: 4 in the lane,
    6 of the wave butterfly, 3 across the waves, the fold thread's rows, and butterfly and waves again."""
    rows = -(-int(n_blocks) // CHUNK_BLOCKS)
    return 4 + 6 + 3 + -(-rows // 256) + 6 + 3


@dataclass
class BlockMoments:
    """The selected (leaf, pose) blocks in (node, pose) order.  pose: index into pose_numbers."""

    node: np.ndarray      # (B,) int32
    pose: np.ndarray      # (B,) int32
    count: np.ndarray     # (B,) int64
    s: np.ndarray         # (B, 3) sum of d = x - anchor
    M: np.ndarray         # (B, 6) sum of d d^T: xx xy xz yy yz zz
    anchor: np.ndarray    # (B, 3) f64 centre of the block's leaf
    pose_numbers: list = field(default_factory=list)   # the selected poses, in the order `pose` indexes
    origin: Optional[np.ndarray] = None                # centre of the box of the scheme's root cubes

    def __len__(self) -> int:
        return len(self.node)


@dataclass
class AdjustmentLeaves:
    """One row per leaf that holds a selected block, in ascending node id: the plane at the given transforms."""

    node: np.ndarray      # (L,) int32
    count: np.ndarray     # (L,) int64 pooled points
    mean: np.ndarray      # (L, 3)
    normal: np.ndarray    # (L, 3)
    lambda0: np.ndarray   # (L,)
    used: np.ndarray      # (L,) bool

    def __len__(self) -> int:
        return len(self.node)


@dataclass
class AdjustmentSystem:
    H: np.ndarray             # (S, 6, 6) symmetric, block-diagonal in the poses
    g: np.ndarray             # (S, 6)
    cost: np.ndarray          # (S,)
    n_points: np.ndarray      # (S,) int64 points of the pose in used leaves
    n_blocks: np.ndarray      # (S,) int64 blocks of the pose in used leaves
    n_leaves: tuple           # (leaves pooled, leaves used)
    origin: np.ndarray        # (3,)
    pose_numbers: list
    leaves: Optional[AdjustmentLeaves] = None
    blocks: Optional[BlockMoments] = None

    @property
    def total_cost(self):
        """The per-pose costs added in ascending pose order."""
        total = self.cost.dtype.type(0)
        for c in self.cost:
            total = total + c
        return total

    def solve(self, damping: float = 0.0, fixed=None) -> np.ndarray:
        """xi (S, 6): per free pose -(H_p + damping diag(H_p))^-1 g_p, zeros for the poses of `fixed` (pose numbers;
        None: the first selected pose, which removes the gauge).  ValueError naming the pose when a free pose has
        fewer than six used points."""
        S = len(self.pose_numbers)
        if fixed is None:
            fixed = self.pose_numbers[:1]
        elif np.isscalar(fixed):
            fixed = [fixed]
        held = set(fixed)
        xi = np.zeros((S, 6))
        for k, p in enumerate(self.pose_numbers):
            if p in held:
                continue
            if self.n_points[k] < 6:
                raise ValueError(f"adjustment system: pose {p} has {int(self.n_points[k])} used points, at least 6 "
                                 "are needed")
            H = np.asarray(self.H[k], dtype=np.float64)
            with np.errstate(invalid="ignore", over="ignore"):
                A = H + float(damping) * np.diag(np.diag(H))
                xi[k] = -np.linalg.solve(A, np.asarray(self.g[k], dtype=np.float64))
        return xi


@dataclass
class Adjustment:
    transforms: np.ndarray    # (S, 4, 4)
    iterations: int
    converged: bool
    costs: List[float] = field(default_factory=list)   # total cost of every system that was solved
    reason: str = ""
    pose_numbers: list = field(default_factory=list)


def as_transforms(transforms, n: int) -> np.ndarray:
    """(n, 3, 4) f64 of n rigid transforms given as (n, 4, 4) or (n, 3, 4) (None: identities), each validated as
    as_transform validates one; ValueError otherwise."""
    out = np.zeros((n, 3, 4))
    out[:, :, :3] = np.eye(3)
    if transforms is None:
        return out
    if len(transforms) != n:
        raise ValueError(f"expected {n} transforms, one per selected pose, got {len(transforms)}")
    for k in range(n):
        R, t = as_transform(transforms[k])
        out[k, :, :3], out[k, :, 3] = R, t
    return out


def root_box_centre(corners, edges) -> np.ndarray:
    """Centre of the axis-aligned box spanned by the cubes (corner (V, 3), edge (V,) or scalar): the default origin."""
    c = np.asarray(corners, dtype=np.float64).reshape(-1, 3)
    if len(c) == 0:
        return np.zeros(3)
    e = np.broadcast_to(np.asarray(edges, dtype=np.float64), (len(c),))
    return (c.min(axis=0) + (c + e[:, None]).max(axis=0)) / 2.0


def block_moments_np(blocks: Sequence, pose_numbers, origin=None, dtype=np.float64) -> BlockMoments:
    """BlockMoments of blocks given as (node id, pose index, anchor (3,), points (m, 3)): d = x - anchor and the sums
    in `dtype` (two exact-as-possible passes are not needed: the shift makes the sums small), rows sorted by (node,
    pose); empty blocks are dropped as the device's block table drops them."""
    rows = sorted(((int(nd), int(p), np.asarray(a, dtype=np.float64), np.asarray(x).reshape(-1, 3))
                   for nd, p, a, x in blocks if len(x)), key=lambda r: (r[0], r[1]))
    B = len(rows)
    s = np.zeros((B, 3), dtype=dtype)
    M = np.zeros((B, 6), dtype=dtype)
    for i, (_, _, a, x) in enumerate(rows):
        d = x.astype(dtype) - a.astype(dtype)
        s[i] = d.sum(axis=0)
        for k, (u, v) in enumerate(_UPPER):
            M[i, k] = (d[:, u] * d[:, v]).sum()
    return BlockMoments(np.array([r[0] for r in rows], dtype=np.int32), np.array([r[1] for r in rows], dtype=np.int32),
                        np.array([len(r[3]) for r in rows], dtype=np.int64), s, M,
                        np.array([r[2] for r in rows], dtype=np.float64).reshape(-1, 3), list(pose_numbers),
                        None if origin is None else _as_origin(origin))


def _dot3(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def _moved(blocks: BlockMoments, T: np.ndarray, dtype, magnitude: bool):
    """(n, s'', M'' full (B, 3, 3)) of every block under its pose's transform.  magnitude: every product by absolute
    values - the sizes the rounding errors are relative to."""
    fix = np.abs if magnitude else (lambda x: x)
    Tb = T[blocks.pose]                                  # (B, 3, 4) f64
    a = blocks.anchor
    with np.errstate(invalid="ignore", over="ignore"):
        ap = np.stack([((Tb[:, i, 0] * a[:, 0] + Tb[:, i, 1] * a[:, 1]) + Tb[:, i, 2] * a[:, 2]) + Tb[:, i, 3]
                       for i in range(3)], axis=1)
        delta = fix((ap - a).astype(dtype))              # (a', delta: f64 bits, whatever the dtype)
        R = fix(Tb[:, :, :3].astype(dtype))
        n = blocks.count.astype(dtype)
        s = fix(np.asarray(blocks.s).astype(dtype))
        M = fix(cov6_to_full(np.asarray(blocks.M).astype(dtype)))
        sp = np.stack([_dot3([R[:, i, 0], R[:, i, 1], R[:, i, 2]], [s[:, 0], s[:, 1], s[:, 2]]) for i in range(3)],
                      axis=1)
        W = np.empty_like(M)
        Mp = np.empty_like(M)
        for i in range(3):
            for j in range(3):
                W[:, i, j] = _dot3([R[:, i, 0], R[:, i, 1], R[:, i, 2]], [M[:, 0, j], M[:, 1, j], M[:, 2, j]])
        for i in range(3):
            for j in range(3):
                Mp[:, i, j] = _dot3([W[:, i, 0], W[:, i, 1], W[:, i, 2]], [R[:, j, 0], R[:, j, 1], R[:, j, 2]])
        s2 = sp + n[:, None] * delta
        M2 = np.empty_like(M)
        for i in range(3):
            for j in range(3):
                M2[:, i, j] = ((Mp[:, i, j] + delta[:, i] * sp[:, j]) + sp[:, i] * delta[:, j]) \
                    + (n * delta[:, i]) * delta[:, j]
    return n, s2, M2


def _leaf_planes(blocks: BlockMoments, n, s2, M2, min_points, min_poses, max_variance, dtype) -> AdjustmentLeaves:
    node = blocks.node
    B = len(node)
    if B == 0:
        z = np.zeros((0, 3), dtype=dtype)
        return AdjustmentLeaves(np.zeros(0, np.int32), np.zeros(0, np.int64), z, np.zeros((0, 3)), np.zeros(0),
                                np.zeros(0, bool))
    head = np.concatenate([[True], node[1:] != node[:-1]])
    first = np.nonzero(head)[0]
    row = np.cumsum(head) - 1
    L = len(first)
    rank = np.arange(B) - first[row]
    N = np.zeros(L, dtype=dtype)
    S = np.zeros((L, 3), dtype=dtype)
    M = np.zeros((L, 3, 3), dtype=dtype)
    for r in range(int(rank.max()) + 1):      # (ascending pose order inside every leaf)
        sel = np.nonzero(rank == r)[0]
        if r == 0:
            N[row[sel]], S[row[sel]], M[row[sel]] = n[sel], s2[sel], M2[sel]
        else:
            N[row[sel]] += n[sel]
            S[row[sel]] += s2[sel]
            M[row[sel]] += M2[sel]
    count = np.zeros(L, dtype=np.int64)
    np.add.at(count, row, blocks.count)
    n_poses = np.zeros(L, dtype=np.int64)
    np.add.at(n_poses, row, (blocks.count > 0).astype(np.int64))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mx = S / N[:, None]
        mean = blocks.anchor[first].astype(dtype) + mx
        C = M / N[:, None, None] - mx[:, :, None] * mx[:, None, :]
    C64 = np.asarray(C, dtype=np.float64)
    ok = np.all(np.isfinite(C64), axis=(1, 2))
    w = np.full((L, 3), np.nan)
    v = np.tile(np.eye(3), (L, 1, 1))
    if ok.any():
        w[ok], vv = np.linalg.eigh(C64[ok])
        v[ok] = orient_eigenvectors(np.ascontiguousarray(vv))
    lam = w[:, 0]
    used = (count >= int(min_points)) & (n_poses >= int(min_poses)) & np.isfinite(lam)
    if max_variance is not None and max_variance >= 0:
        with np.errstate(invalid="ignore"):
            used &= ~(lam > max_variance)
    return AdjustmentLeaves(node[first].astype(np.int32), count, mean, np.ascontiguousarray(v[:, :, 0]), lam, used)


def _block_terms(n, s2, M2, nrm, e, u, dtype, magnitude: bool):
    """(B, 28) terms A Q A^T (upper triangle), A Q pi, pi^T Q pi / 2 of blocks with plane normal nrm, e = a - c,
    u = a - mean.  magnitude: every product by absolute values."""
    B = len(n)
    fix = np.abs if magnitude else (lambda x: x)
    nrm, e, u = fix(nrm.astype(dtype)), fix(e), fix(u)
    K = np.zeros((B, 3, 3), dtype=dtype)              # K v = v x nrm
    K[:, 0, 1], K[:, 0, 2] = nrm[:, 2], -nrm[:, 1]
    K[:, 1, 0], K[:, 1, 2] = -nrm[:, 2], nrm[:, 0]
    K[:, 2, 0], K[:, 2, 1] = nrm[:, 1], -nrm[:, 0]
    K = fix(K)
    if magnitude:
        ke = np.stack([e[:, 1] * nrm[:, 2] + e[:, 2] * nrm[:, 1], e[:, 2] * nrm[:, 0] + e[:, 0] * nrm[:, 2],
                       e[:, 0] * nrm[:, 1] + e[:, 1] * nrm[:, 0]], axis=1)
    else:
        ke = np.cross(e, nrm).reshape(-1, 3)
    A = np.zeros((B, 6, 4), dtype=dtype)
    A[:, :3, :3], A[:, :3, 3], A[:, 3:, 3] = K, ke, nrm
    pi = np.concatenate([nrm, _dot3([nrm[:, 0], nrm[:, 1], nrm[:, 2]], [u[:, 0], u[:, 1], u[:, 2]])[:, None]], axis=1)
    Q = np.zeros((B, 4, 4), dtype=dtype)
    Q[:, :3, :3], Q[:, :3, 3], Q[:, 3, :3], Q[:, 3, 3] = M2, s2, s2, n
    out = np.zeros((B, 28), dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        QA = np.matmul(Q, np.swapaxes(A, 1, 2))       # (B, 4, 6)
        H = np.matmul(A, QA)
        Qp = np.matmul(Q, pi[:, :, None])[:, :, 0]
        out[:, :21] = H[:, _TRIU[0], _TRIU[1]]
        out[:, 21:27] = np.matmul(A, Qp[:, :, None])[:, :, 0]
        out[:, 27] = (pi * Qp).sum(axis=1) / 2
    return out


def adjustment_system_np(blocks: BlockMoments, transforms=None, origin=None, min_points: int = 8, min_poses: int = 2,
                         max_variance: Optional[float] = None, dtype=np.float64, leaves: bool = False,
                         planes: Optional[AdjustmentLeaves] = None, magnitude: bool = False) -> AdjustmentSystem:
    """The definition (module docstring), on the host, from the block moments.  transforms: (S, 4, 4) or (S, 3, 4) in
    the order of blocks.pose_numbers (None: identities); origin None: blocks.origin.  The moved moments, the pooling
    and the sums are formed in `dtype` (np.longdouble for a reference of higher precision).  planes: take this leaf
    table (normal, mean, used) as given instead of forming it here - the reference of a sum over exactly the terms
    another implementation selected, from exactly its plane bits.  magnitude (with planes): every sum becomes the sum
    of the absolute values of the products it is made of - what the rounding errors of forming and adding the terms
    are relative to.  leaves: the leaf table and the blocks come back with the system."""
    S = len(blocks.pose_numbers)
    T = as_transforms(transforms, S)
    c = blocks.origin if origin is None else _as_origin(origin)
    if c is None:
        raise ValueError("the origin must be three finite numbers")
    c = _as_origin(c)
    if magnitude and planes is None:
        raise ValueError("magnitude needs the leaf table the sums were formed with")
    n, s2, M2 = _moved(blocks, T, dtype, magnitude)
    if planes is None:
        planes = _leaf_planes(blocks, n, s2, M2, min_points, min_poses, max_variance, dtype)
    B = len(blocks)
    H = np.zeros((S, 6, 6), dtype=dtype)
    g = np.zeros((S, 6), dtype=dtype)
    cost = np.zeros(S, dtype=dtype)
    n_points = np.zeros(S, dtype=np.int64)
    n_blocks = np.zeros(S, dtype=np.int64)
    if B:
        row = np.searchsorted(planes.node, blocks.node)
        keep = np.nonzero(np.asarray(planes.used, dtype=bool)[row])[0]
        row = row[keep]
        a = blocks.anchor[keep].astype(dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            terms = _block_terms(n[keep], s2[keep], M2[keep], np.asarray(planes.normal)[row], a - c.astype(dtype),
                                 a - np.asarray(planes.mean)[row].astype(dtype), dtype, magnitude)
            for k in range(S):
                mine = blocks.pose[keep] == k
                tk = terms[mine]
                acc = tk.sum(axis=0, dtype=dtype) if len(tk) else np.zeros(28, dtype=dtype)
                H[k][_TRIU] = acc[:21]
                H[k] = H[k] + np.triu(H[k], 1).T
                g[k], cost[k] = acc[21:27], acc[27]
                n_points[k] = int(blocks.count[keep][mine].sum())
                n_blocks[k] = int(mine.sum())
    out = AdjustmentSystem(H, g, cost, n_points, n_blocks, (len(planes), int(np.sum(planes.used))), c,
                           list(blocks.pose_numbers))
    if leaves:
        out.leaves, out.blocks = planes, blocks
    return out


def system_from_device(sums, counts, n_leaves, origin, pose_numbers) -> AdjustmentSystem:
    """AdjustmentSystem of the device's S x 28 sums and S x 2 counts."""
    s = np.asarray(sums, dtype=np.float64).reshape(-1, 28)
    S = len(s)
    H = np.zeros((S, 6, 6))
    H[:, _TRIU[0], _TRIU[1]] = s[:, :21]
    H = H + np.swapaxes(np.triu(H, 1), 1, 2)
    cnt = np.asarray(counts, dtype=np.int64).reshape(-1, 2)
    return AdjustmentSystem(H, s[:, 21:27].copy(), s[:, 27].copy(), cnt[:, 0].copy(), cnt[:, 1].copy(),
                            (int(n_leaves[0]), int(n_leaves[1])), np.array(origin, dtype=np.float64),
                            list(pose_numbers))


def adjust_np(system: Callable, n_poses: int, initial=None, fixed=None, max_iterations: int = 200,
              tolerance: float = 1e-9, damping: float = 0.0) -> Adjustment:
    """Block-Jacobi plane adjustment over system(T (S, 4, 4)) -> AdjustmentSystem (one origin for the whole run).  Per
    iteration: xi = system.solve(damping, fixed), T_p <- se3_exp(xi_p, origin) T_p.  Ends converged when max_p |xi_p|
    < tolerance; otherwise at max_iterations, or - with the last good transforms - when a free pose has fewer than six
    used points ("no correspondences") or a system cannot be solved ("singular system")."""
    T34 = as_transforms(initial, n_poses)
    T = np.stack([_matrix(t[:, :3], t[:, 3]) for t in T34]) if n_poses else np.zeros((0, 4, 4))
    costs: List[float] = []
    poses: list = []
    for it in range(int(max_iterations)):
        s = system(T)
        poses = list(s.pose_numbers)
        try:
            xi = s.solve(damping, fixed)
        except ValueError:
            return Adjustment(T, it, False, costs, "no correspondences", poses)
        except np.linalg.LinAlgError:
            xi = None
        if xi is None or not np.all(np.isfinite(xi)):
            return Adjustment(T, it, False, costs, "singular system", poses)
        costs.append(float(s.total_cost))
        for k in range(n_poses):
            T[k] = se3_exp(xi[k], s.origin) @ T[k]
            T[k, 3] = [0.0, 0.0, 0.0, 1.0]
        step = float(np.max(np.linalg.norm(xi, axis=1))) if n_poses else 0.0
        if step < tolerance:
            return Adjustment(T, it + 1, True, costs, "converged", poses)
    return Adjustment(T, int(max_iterations), False, costs, "max_iterations", poses)
