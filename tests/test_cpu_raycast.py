"""raycast_np, the brute-force definition of the ray query (octreelib_amd/query.py), and HostMap.raycast - what a grid on
the caller's own plug types answers with - on hand-built maps with known answers.  No GPU: the device kernel is compared
with raycast_np bit for bit in tests/test_gpu_raycast.py, and its traversal, compiled for the CPU, in
tests/test_cpu_raycast_host.py."""

import math

import numpy as np
import pytest

import octreelib_amd
from octreelib_amd import LeafPlanes, RayHits, normalize_directions, raycast_np
from octreelib_amd.query import RAY_CAP_EDGES, HostMap
from tests._raycast import DIRECTIONS, assert_hits_equal, box_rays
from tests.test_cpu_query import _Leaf

INF = float("inf")


# ---- the map: 2 x 2 x 2 unit voxels, (1, 0, 0) missing; node ids in voxel order -------------------------------------------
VOX = [v for v in np.ndindex(2, 2, 2) if v != (1, 0, 0)]
ID = {v: i for i, v in enumerate(VOX)}
CORNER = np.array(VOX, dtype=np.float64)
EDGE = np.ones(len(VOX))
NODE = np.arange(len(VOX))


def cast(o, d, t_max, t_min=0.0, count=None, **kw):
    o, d = np.atleast_2d(np.asarray(o, dtype=np.float64)), np.atleast_2d(np.asarray(d, dtype=np.float64))
    count = np.full(len(VOX), 5) if count is None else count
    return raycast_np(o, normalize_directions(d), t_max, NODE, CORNER, EDGE, t_min=t_min, count=count, **kw)


def one(o, d, t_max, **kw):
    h = cast(o, d, t_max, **kw)
    return int(h.node[0]), float(h.t[0])


def _python_reference(o, d, tmin, tmax, node, corner, edge, ok_leaf, plane=None):
    """The definition as a loop over Python floats (IEEE doubles, every operation rounded)."""
    out = []
    for i in range(len(o)):
        oi, di = o[i].tolist(), d[i].tolist()
        best = (INF, -1, -1)
        vals = oi + di + [float(tmin[i]), float(tmax[i])]
        inv = [(1.0 / x if x != 0.0 else INF) for x in di] if all(math.isfinite(v) for v in vals) else None
        zero = inv and [x == 0.0 or not math.isfinite(y) for x, y in zip(di, inv)]
        if inv is None or tmax[i] < tmin[i] or all(zero) or any(abs(x) > 1.0 for x in di):
            out.append(best)
            continue
        for j in np.argsort(node):
            if not ok_leaf[j]:
                continue
            t_in, t_out, crossed = float(tmin[i]), float(tmax[i]), True
            for a in range(3):
                lo, hi = float(corner[j][a]), float(corner[j][a] + edge[j])
                if zero[a]:
                    crossed = crossed and lo <= oi[a] <= hi
                else:
                    p, q = (lo - oi[a]) * inv[a], (hi - oi[a]) * inv[a]
                    t_in, t_out = max(t_in, min(p, q)), min(t_out, max(p, q))
            if not (crossed and t_in <= t_out):
                continue
            t, row = t_in, -1
            if plane is not None:
                nrm, mean, row = plane[0][j].tolist(), plane[1][j].tolist(), int(plane[2][j])
                num = (nrm[0] * (mean[0] - oi[0]) + nrm[1] * (mean[1] - oi[1])) + nrm[2] * (mean[2] - oi[2])
                den = (nrm[0] * di[0] + nrm[1] * di[1]) + nrm[2] * di[2]
                if den == 0.0:
                    continue
                t = num / den
                if not (t_in <= t <= t_out):
                    continue
            if t < best[0]:                      # (ascending node id: the first of equal t stays)
                best = (t, int(node[j]), row)
        out.append(best)
    return out


# ---- known answers ------------------------------------------------------------------------------------------------------
def test_axis_rays_through_the_block_with_a_gap_and_their_mirrors():
    assert one([-1.0, 0.5, 0.5], [1, 0, 0], 10.0) == (ID[(0, 0, 0)], 1.0)
    assert one([-1.0, 0.5, 0.5], [5, 0, 0], 10.0) == (ID[(0, 0, 0)], 1.0)          # (directions are normalised)
    assert one([3.0, 0.5, 0.5], [-1, 0, 0], 10.0) == (ID[(0, 0, 0)], 2.0)          # across the missing voxel
    assert one([3.0, 0.5, 0.5], [-1, 0, 0], 1.5) == (-1, INF)                       # ... which holds nothing
    assert one([3.0, 1.5, 0.5], [-1, 0, 0], 10.0) == (ID[(1, 1, 0)], 1.0)
    assert one([-1.0, 1.5, 0.5], [1, 0, 0], 10.0) == (ID[(0, 1, 0)], 1.0)
    # max_range is inclusive: the wall at t = 1 is reached by a ray of range 1, not by one an ulp shorter
    assert one([-1.0, 0.5, 0.5], [1, 0, 0], 1.0) == (ID[(0, 0, 0)], 1.0)
    assert one([-1.0, 0.5, 0.5], [1, 0, 0], np.nextafter(1.0, 0.0)) == (-1, INF)
    for axis in range(3):                       # every axis, both signs: the mirrored ray gives the mirrored answer
        o = np.full(3, 1.5)
        o[axis] = -2.0
        d = np.zeros(3)
        d[axis] = 1.0
        v = [1, 1, 1]
        v[axis] = 0
        assert one(o, d, 10.0) == (ID[tuple(v)], 2.0)
        o[axis], v[axis] = 4.0, 1
        assert one(o, -d, 10.0) == (ID[tuple(v)], 2.0)


def test_shared_face_edge_and_corner_go_to_the_lower_node_id():
    # along the face y = 1: the leaves on both sides are crossed at the same t
    assert one([-1.0, 1.0, 0.5], [1, 0, 0], 10.0) == (ID[(0, 0, 0)], 1.0)
    assert one([3.0, 1.0, 0.5], [-1, 0, 0], 10.0) == (ID[(1, 1, 0)], 1.0)           # ((1, 0, 0) is missing)
    # along the edge y = 1, z = 1: four leaves
    assert one([-1.0, 1.0, 1.0], [1, 0, 0], 10.0) == (ID[(0, 0, 0)], 1.0)
    assert one([3.0, 1.0, 1.0], [-1, 0, 0], 10.0) == (ID[(1, 0, 1)], 1.0)
    # through the corner (1, 1, 1) along the space diagonal: t is the formula's
    d = normalize_directions([[1.0, 1.0, 1.0]])[0]
    node, t = one([-1.0, -1.0, -1.0], [1, 1, 1], 10.0)
    assert node == ID[(0, 0, 0)] and t == (0.0 - -1.0) * (1.0 / d[0])
    node, t = one([-1.0, -1.0, -1.0], [1, 1, 1], 10.0, t_min=3.0)
    assert node == ID[(0, 0, 0)] and t == 3.0                       # still inside (0, 0, 0): it ends at sqrt(12)
    node, t = one([-1.0, -1.0, -1.0], [1, 1, 1], 10.0, t_min=3.5)
    assert node == ID[(1, 1, 1)] and t == 3.5
    # a ray that only touches the corner (1, 1) of (0, 0, 0): crossed there, at one point
    inv = 1.0 / normalize_directions([[1.0, -1.0, 0.0]])[0, 0]
    node, t = one([-1.0, 3.0, 0.5], [1, -1, 0], 10.0, count=np.array([5, 0, 0, 0, 0, 0, 0]))
    assert node == ID[(0, 0, 0)] and t == 2.0 * inv


def test_start_inside_min_range_and_zero_components():
    assert one([0.5, 0.5, 0.5], [1, 0, 0], 10.0) == (ID[(0, 0, 0)], 0.0)             # inside: t = t_min
    assert one([0.5, 0.5, 0.5], [1, 0, 0], 10.0, t_min=0.25) == (ID[(0, 0, 0)], 0.25)
    assert one([0.5, 1.5, 0.5], [1, 0, 0], 10.0, t_min=0.75) == (ID[(1, 1, 0)], 0.75)  # past the exit: the next leaf
    assert one([0.5, 1.5, 0.5], [1, 0, 0], 10.0, t_min=0.5) == (ID[(0, 1, 0)], 0.5)    # the exit itself is inclusive
    assert one([0.5, 0.5, 0.5], [1, 0, 0], 10.0, t_min=0.75) == (-1, INF)             # ... the missing voxel
    # zero components: the origin on a face is inside both neighbours, off it in one, outside the block in none
    assert one([-1.0, 2.0, 0.5], [1, 0, 0], 10.0) == (ID[(0, 1, 0)], 1.0)             # on the outer face y = 2
    assert one([-1.0, np.nextafter(2.0, 3.0), 0.5], [1, 0, 0], 10.0) == (-1, INF)
    assert one([-1.0, np.nextafter(1.0, 2.0), 0.5], [1, 0, 0], 10.0) == (ID[(0, 1, 0)], 1.0)
    assert one([-1.0, np.nextafter(1.0, 0.0), 0.5], [1, 0, 0], 10.0) == (ID[(0, 0, 0)], 1.0)
    # a denormal component has no finite reciprocal: the axis is treated as a zero one
    h = raycast_np([[-1.0, 0.5, 0.5]], [[1.0, 1e-320, 0.0]], 10.0, NODE, CORNER, EDGE, count=np.full(7, 1))
    assert (int(h.node[0]), float(h.t[0])) == (ID[(0, 0, 0)], 1.0)


def test_dead_rays_and_input_forms():
    nan = float("nan")
    O = np.array([[-1.0, 0.5, 0.5]] * 8)
    D = np.array([[1.0, 0, 0]] * 8)
    tmin, tmax = np.zeros(8), np.full(8, 10.0)
    O[1, 0], D[2, 1], tmin[3], tmax[4] = nan, INF, nan, INF
    D[5] = 0.0
    tmin[6], tmax[6] = 2.0, 1.0
    h = raycast_np(O, D, tmax, NODE, CORNER, EDGE, t_min=tmin, count=np.full(7, 1))
    assert isinstance(h, RayHits) and h.node.dtype == np.int32 and h.row.dtype == np.int32 and h.t.dtype == np.float64
    assert h.node.tolist() == [0, -1, -1, -1, -1, -1, -1, 0] and np.all(h.row == -1)
    assert h.hit.tolist() == [True] + [False] * 6 + [True] and np.all(np.isinf(h.t[1:7]))
    # the definition takes directions as given: a component above 1 is a dead ray, the methods normalise first
    assert raycast_np(O[:1], [[2.0, 0, 0]], 10.0, NODE, CORNER, EDGE, count=np.full(7, 1)).node[0] == -1
    assert np.array_equal(normalize_directions([[0.0, 0.0, 0.0], [3.0, 0.0, 4.0]]), [[0, 0, 0], [0.6, 0, 0.8]])
    assert np.all(np.abs(normalize_directions(np.random.default_rng(0).normal(size=(20000, 3)) * 1e3)) <= 1.0)
    p = h.points(O, D)
    assert p[0].tolist() == [0.0, 0.5, 0.5] and np.all(np.isnan(p[1:7]))
    e = raycast_np(np.empty((0, 3)), np.empty((0, 3)), 1.0, NODE, CORNER, EDGE, count=np.full(7, 1))
    assert e.node.shape == e.t.shape == e.row.shape == (0,)
    with pytest.raises(ValueError):
        raycast_np(O, D[:3], 1.0, NODE, CORNER, EDGE, count=np.full(7, 1))
    with pytest.raises(ValueError):
        raycast_np(O, D, np.ones(3), NODE, CORNER, EDGE, count=np.full(7, 1))
    with pytest.raises(ValueError):
        raycast_np(O, D, 1.0, NODE, CORNER, EDGE, count=np.full(7, 1), surface="sphere")
    assert {"RayHits", "raycast_np", "normalize_directions"} <= set(octreelib_amd.__all__)


def test_min_points_and_random_rays_against_a_python_loop():
    count = np.array([1, 0, 3, 8, 2, 0, 9])
    assert one([-1.0, 0.5, 1.5], [1, 0, 0], 10.0, count=count) == (ID[(1, 0, 1)], 2.0)   # (0, 0, 1) holds nothing
    assert one([-1.0, 0.5, 0.5], [1, 0, 0], 10.0, count=count, min_points=2) == (-1, INF)
    assert one([-1.0, 1.5, 1.5], [1, 0, 0], 10.0, count=count, min_points=9) == (ID[(1, 1, 1)], 2.0)
    rng = np.random.default_rng(3)
    O, D = box_rays(rng, [0, 0, 0], [2, 2, 2], 300, 1.5)
    O = np.concatenate([O, np.repeat([[1.0, 1.0, 1.0], [0.0, 2.0, 1.0], [-1.0, 1.0, 0.5]], len(DIRECTIONS), axis=0)])
    D = normalize_directions(np.concatenate([D, np.tile(DIRECTIONS, (3, 1))]))
    tmin, tmax = rng.uniform(0.0, 1.0, len(O)), rng.uniform(0.5, 6.0, len(O))
    for mp in (1, 3):
        got = raycast_np(O, D, tmax, NODE, CORNER, EDGE, t_min=tmin, count=count, min_points=mp)
        ref = _python_reference(O, D, tmin, tmax, NODE, CORNER, EDGE, count >= mp)
        assert [(float(t), int(n), int(r)) for n, t, r in zip(got.node, got.t, got.row)] == ref
        assert 0.2 < got.hit.mean() < 0.95


# ---- the plane form ---------------------------------------------------------------------------------------------------
def _tilted_planes():
    """Rows for the leaves (0, 0, 0), (0, 1, 0), (1, 1, 0): a plane tilted about z through the leaf's centre; the second
    one's mean lies outside its cube along x, the third has too few points."""
    n = np.array([math.cos(0.3), math.sin(0.3), 0.0])
    vecs = np.zeros((3, 3, 3))
    vecs[:, :, 0] = n
    mean = np.array([[0.5, 0.5, 0.5], [1.5, 1.5, 0.5], [1.5, 1.5, 0.5]])
    return LeafPlanes(np.array([20, 20, 3]), mean, np.zeros((3, 3, 3)), np.array([[1e-4, 1, 1]] * 3), vecs,
                      np.array([ID[(0, 0, 0)], ID[(0, 1, 0)], ID[(1, 1, 0)]], dtype=np.int32))


def test_plane_form_on_a_tilted_plane():
    planes = _tilted_planes()
    n = planes.normal[0]

    def plane(o, d, t_max, **kw):
        h = raycast_np([o], normalize_directions([d]), t_max, NODE, CORNER, EDGE, planes=planes, surface="plane", **kw)
        return int(h.node[0]), float(h.t[0]), int(h.row[0])

    # t is the formula's, on the plane through the leaf's centre
    o, d = [-1.0, 0.25, 0.5], [1.0, 0.0, 0.0]
    num = (n[0] * (0.5 - o[0]) + n[1] * (0.5 - o[1])) + n[2] * (0.5 - o[2])
    den = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]
    assert plane(o, d, 10.0) == (ID[(0, 0, 0)], num / den, 0)
    assert 1.0 < num / den < 2.0
    # (0, 1, 0)'s plane is met outside its cube (beyond x = 1): rejected, and (1, 1, 0) has too few points
    assert plane([-1.0, 1.5, 0.5], d, 10.0) == (-1, INF, -1)
    node, t, row = plane([-1.0, 1.5, 0.5], d, 10.0, min_points=3)
    assert (node, row) == (ID[(1, 1, 0)], 2) and t == (n[0] * (1.5 - -1.0) + n[1] * 0.0) / n[0]
    assert plane([-1.0, 1.5, 0.5], d, 10.0, min_points=3, max_variance=1e-5) == (-1, INF, -1)
    # ... while the cube form stops at (0, 1, 0)
    assert one([-1.0, 1.5, 0.5], d, 10.0) == (ID[(0, 1, 0)], 1.0)
    # a ray in the plane (den == 0) meets nothing; one that starts behind the plane does not see it
    assert plane([0.5, 0.5, -1.0], [0.0, 0.0, 1.0], 10.0) == (-1, INF, -1)
    assert plane([0.9, 0.5, 0.5], d, 10.0) == (-1, INF, -1)
    # against the loop, rays from everywhere
    rng = np.random.default_rng(5)
    O, D = box_rays(rng, [0, 0, 0], [2, 2, 1], 300, 1.0)
    D = normalize_directions(D)
    got = raycast_np(O, D, 5.0, NODE, CORNER, EDGE, planes=planes, surface="plane", min_points=3)
    ok = np.zeros(7, dtype=bool)
    ok[planes.node] = True
    per_leaf = (np.zeros((7, 3)), np.zeros((7, 3)), np.full(7, -1))
    per_leaf[0][planes.node], per_leaf[1][planes.node], per_leaf[2][planes.node] = planes.normal, planes.mean, [0, 1, 2]
    ref = _python_reference(O, D, np.zeros(300), np.full(300, 5.0), NODE, CORNER, EDGE, ok, per_leaf)
    assert [(float(t), int(n_), int(r)) for n_, t, r in zip(got.node, got.t, got.row)] == ref
    assert got.hit.sum() > 30 and set(got.row[got.hit].tolist()) == {0, 2}     # (row 1's plane misses its cube)


# ---- HostMap.raycast: pose selection, the cap ------------------------------------------------------------------------------
def _host_grid():
    roots = [(np.array(v, dtype=np.float64), 1.0) for v in VOX]
    rng = np.random.default_rng(9)
    pts = {v: np.array(v) + rng.uniform(0.1, 0.9, (4, 3)) for v in VOX}
    pose0 = [_Leaf(np.array(v, dtype=np.float64), 1.0, pts[v] if v[2] == 0 else np.empty((0, 3))) for v in VOX]
    pose1 = [_Leaf(np.array(v, dtype=np.float64), 1.0, pts[v][:2] if v[2] == 1 else np.empty((0, 3))) for v in VOX]
    return HostMap(0, 1.0, roots, {4: pose0, 9: pose1})


def test_host_map_pose_selection_min_points_and_the_cap():
    hm = _host_grid()
    o, d = [[0.5, 0.5, -1.0]], [[0.0, 0.0, 2.0]]
    both = hm.raycast(o, d, 10.0)
    assert (int(both.node[0]), float(both.t[0])) == (ID[(0, 0, 0)], 1.0)
    only9 = hm.raycast(o, d, 10.0, pose_numbers=[9])
    assert (int(only9.node[0]), float(only9.t[0])) == (ID[(0, 0, 1)], 2.0)
    assert hm.raycast(o, d, 10.0, pose_numbers=[9], min_points=3).node[0] == -1
    assert hm.raycast(o, d, 10.0, min_points=3).node[0] == ID[(0, 0, 0)]
    assert hm.raycast(o, d, 10.0, min_range=2.5, min_points=3).node[0] == -1
    # the cap: 256 voxel edges between min_range and max_range, dead rays excepted
    assert hm.raycast(o, d, RAY_CAP_EDGES).hit[0] and hm.raycast(o, d, 300.0, min_range=44.0).node[0] == -1
    with pytest.raises(ValueError, match="voxel edges"):
        hm.raycast(o, d, np.nextafter(RAY_CAP_EDGES, 1e9))
    with pytest.raises(ValueError, match="voxel edges"):
        hm.raycast(o, d, 2.0 ** 41, min_range=2.0 ** 41 - 1.0)
    assert hm.raycast(o, d, float("inf")).node[0] == -1 and hm.raycast(o, d, 1.0, min_range=1e9).node[0] == -1
    cube = HostMap(1, 2.0, [(np.zeros(3), 2.0)], {0: [_Leaf(np.zeros(3), 2.0, np.ones((3, 3)))]})
    far = cube.raycast([[1.0, 1.0, -1e6]], [[0.0, 0.0, 1.0]], 2e6)                  # one cube has no cap
    assert (int(far.node[0]), float(far.t[0])) == (0, 1e6)
    with pytest.raises(ValueError):
        hm.raycast(o, d, 10.0, surface="plain")
    with pytest.raises(ValueError):
        hm.raycast(np.zeros((2, 3)), d, 10.0)
