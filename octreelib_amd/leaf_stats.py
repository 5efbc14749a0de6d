"""
Per-leaf point statistics: what a plane-based SLAM front end keeps of each octree leaf after RANSAC and apply_mask -
the point count, the centroid and the covariance (second moments, the input of a plane factor), and the covariance's
eigen-decomposition, whose smallest eigenvalue's vector is the leaf's least-squares plane normal.

Grid.leaf_statistics / OctreeManager.leaf_statistics / Octree.leaf_statistics compute them on the device in one call
(Forest.leaf_stats, octl_forest_leaf_stats); leaf_statistics_np is the same on the host, for the classes built on the
caller's own plug types and as a reference at higher precision.
"""

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

__all__ = ["LeafStatistics", "leaf_statistics_np", "leaf_statistics_of_leaves", "cov6_to_full", "orient_eigenvectors"]

_UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def cov6_to_full(c6: np.ndarray) -> np.ndarray:
    """(n, 6) upper triangles xx xy xz yy yz zz -> (n, 3, 3) symmetric matrices."""
    c6 = np.asarray(c6)
    out = np.empty((len(c6), 3, 3), dtype=c6.dtype)
    for k, (i, j) in enumerate(_UPPER):
        out[:, i, j] = c6[:, k]
        out[:, j, i] = c6[:, k]
    return out


def orient_eigenvectors(v: np.ndarray) -> np.ndarray:
    """The library's sign rule, in place on (n, 3, 3) eigenvector columns: each column's largest-magnitude component
    is made positive (on equal magnitudes the lowest index)."""
    if len(v) == 0:
        return v
    for col in range(3):
        x = v[:, :, col]
        k = np.argmax(np.abs(x), axis=1)   # (first maximum: the lowest index on ties)
        neg = x[np.arange(len(x)), k] < 0
        x[neg] = -x[neg]
    return v


@dataclass
class LeafStatistics:
    """Statistics of n leaves; row i describes the i-th leaf of the listing they were computed for
    (get_leaf_points(pose_number) with non_empty=True)."""

    count: np.ndarray                          # (n,) int64
    mean: np.ndarray                           # (n, 3)
    covariance: np.ndarray                     # (n, 3, 3) population covariance (np.cov(..., bias=True))
    eigenvalues: Optional[np.ndarray] = None   # (n, 3) ascending
    eigenvectors: Optional[np.ndarray] = None  # (n, 3, 3) columns are the eigenvectors

    def __len__(self) -> int:
        return len(self.count)

    @property
    def normal(self) -> np.ndarray:
        """(n, 3) unit normal of each leaf's least-squares plane: the smallest eigenvalue's eigenvector."""
        return self.eigenvectors[:, :, 0]

    @property
    def offset(self) -> np.ndarray:
        """(n,) d of the plane normal . p + d = 0 through the mean: [normal, offset] has the ax + by + cz + d form of
        the RANSAC plane."""
        return -np.einsum("ij,ij->i", self.normal, self.mean)

    @property
    def surface_variation(self) -> np.ndarray:
        """(n,) lambda0 / (lambda0 + lambda1 + lambda2): 0 for a perfect plane, 1/3 for isotropic scatter; 0 where
        the sum is 0 (a single point, coincident points)."""
        w = self.eigenvalues
        s = w.sum(axis=1)
        out = np.zeros(len(w), dtype=w.dtype)
        nz = s != 0
        out[nz] = w[nz, 0] / s[nz]
        return out


def leaf_statistics_np(point_arrays: Sequence, dtype=np.float64, eigen: bool = True) -> LeafStatistics:
    """LeafStatistics of a list of (m_i, 3) point arrays on the host: two passes (mean, then the centred second
    moments) in `dtype` - np.longdouble for a reference of higher precision; mean and covariance are returned in that
    dtype.  The eigen-decomposition is np.linalg.eigh's (in float64) under the library's sign rule.  An empty array
    gives count 0 and zeros."""
    arrays = [np.asarray(a, dtype=dtype).reshape(-1, 3) for a in point_arrays]
    n = len(arrays)
    count = np.array([len(a) for a in arrays], dtype=np.int64)
    mean = np.zeros((n, 3), dtype=dtype)
    c6 = np.zeros((n, 6), dtype=dtype)
    nz = np.nonzero(count)[0]
    if len(nz):
        pts = np.concatenate([arrays[i] for i in nz])
        cnt = count[nz]
        starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        m = np.add.reduceat(pts, starts, axis=0) / cnt[:, None].astype(dtype)
        d = pts - np.repeat(m, cnt, axis=0)
        mean[nz] = m
        for k, (i, j) in enumerate(_UPPER):
            c6[nz, k] = np.add.reduceat(d[:, i] * d[:, j], starts) / cnt.astype(dtype)
    cov = cov6_to_full(c6)
    w = v = None
    if eigen:
        if n:
            w, v = np.linalg.eigh(cov.astype(np.float64))
            v = orient_eigenvectors(np.ascontiguousarray(v))
        else:
            w, v = np.zeros((0, 3)), np.zeros((0, 3, 3))
    return LeafStatistics(count, mean, cov, w, v)


def leaf_statistics_of_leaves(leaves) -> LeafStatistics:
    """LeafStatistics of the listed leaves' get_points() on the host (the classes on the caller's own plug types):
    moments in np.longdouble, returned as float64."""
    st = leaf_statistics_np([v.get_points() for v in leaves], dtype=np.longdouble)
    st.mean = st.mean.astype(np.float64)
    st.covariance = st.covariance.astype(np.float64)
    return st
