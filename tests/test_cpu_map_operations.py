"""The map operations of Grid and OctreeManager without a GPU: each is written once (octreelib_amd/_map_ops.py) and
both classes inherit that one function; the public surface of Grid, OctreeManager and Octree - names, signatures,
which methods are documented - is the recorded one; on the caller's own plug types the six operations that change the
device-resident map are refused with the class's name before any pose is looked up, and the shared pose lookup of the
queries works against the pose table of either plug."""

import inspect

import numpy as np
import pytest

from octreelib_amd.grid import Grid, GridConfig
from octreelib_amd.octree import Octree
from octreelib_amd.octree.octree_base import OctreeConfigBase
from octreelib_amd.octree_manager import OctreeManager

from tests.test_cpu_query import HostManager, HostOctree

SHARED = [
    "locate", "nearest", "raycast", "ray_evidence", "carve", "carve_rays", "radius_count", "remove_sparse",
    "leaf_planes", "plane_segments", "point_to_plane",
    "registration_system", "align", "point_registration_system", "align_points",
    "adjustment_system", "adjust",
    "transform_poses", "remove_poses", "prune",
    "node_cubes",
    "_adjust_names", "_query_slots",
]

# {class: {method: (str(inspect.signature(method)), the method had a docstring)}} of every public callable, recorded
# before the operations moved into MapOperations.  _BOTH: the rows that Grid and OctreeManager have in common.
_BOTH = {
    'adjust': ('(self, initial=None, pose_numbers: Optional[List[int]] = None, origin=None, min_points: int = 8, '
               'min_poses: int = 2, max_variance: Optional[float] = None, fixed=None, max_iterations: int = 200, '
               'tolerance: float = 1e-09, damping: float = 0.0) -> octreelib_amd.adjustment.Adjustment',
               True),
    'adjustment_system': ('(self, transforms=None, pose_numbers: Optional[List[int]] = None, origin=None, '
                          'min_points: int = 8, min_poses: int = 2, max_variance: Optional[float] = None, '
                          'leaves: bool = False) -> octreelib_amd.adjustment.AdjustmentSystem',
                          True),
    'align': ('(self, points, initial=None, pose_numbers: Optional[List[int]] = None, min_points: int = 8, '
              'max_variance: Optional[float] = None, max_distance: Optional[float] = None, huber_delta: '
              'Optional[float] = None, max_iterations: int = 20, tolerance: float = 1e-09, damping: float = 0.0) -> '
              'octreelib_amd.registration.Alignment',
              True),
    'align_points': ('(self, points, initial=None, *, max_distance: float, pose_numbers: Optional[List[int]] = None, '
                     'huber_delta: Optional[float] = None, max_iterations: int = 20, tolerance: float = 1e-09, '
                     'damping: float = 0.0) -> octreelib_amd.registration.Alignment',
                     True),
    'carve': ('(self, evidence: octreelib_amd.query.RayEvidence, min_through: int = 2, max_hits: int = 0, '
              'pose_numbers: Optional[List[int]] = None) -> int',
              True),
    'carve_rays': ('(self, origins, directions, ranges, margin, min_range=0.0, returned=None, min_through: int = 2, '
                   'max_hits: int = 0, pose_numbers: Optional[List[int]] = None) -> int',
                   True),
    'insert_points': ('(self, pose_number: int, points, *, transform=None, segment=None)', True),
    'leaf_planes': ('(self, pose_numbers: Optional[List[int]] = None) -> octreelib_amd.query.LeafPlanes', True),
    'leaf_statistics': ('(self, pose_number: int) -> octreelib_amd.leaf_stats.LeafStatistics', True),
    'locate': ('(self, points) -> numpy.ndarray', True),
    'map_leaf_points': ('(self, function: Callable, pose_numbers: Optional[List[int]] = None)', False),
    'n_leaves': ('(self, pose_number: int) -> int', False),
    'n_nodes': ('(self, pose_number: int) -> int', False),
    'nearest': ('(self, points, k: int = 1, *, max_distance: float, pose_numbers: Optional[List[int]] = None) -> '
                'octreelib_amd.query.Neighbours',
                True),
    'node_cubes': ('(self)', True),
    'plane_segments': ('(self, pose_numbers: Optional[List[int]] = None, min_points: int = 8, max_variance: '
                       'Optional[float] = None, max_angle: float = 0.1, max_offset: float = 0.05) -> '
                       'octreelib_amd.query.PlaneSegments',
                       True),
    'point_registration_system': ('(self, points, transform=None, *, max_distance: float, pose_numbers: '
                                  'Optional[List[int]] = None, huber_delta: Optional[float] = None, origin=None, '
                                  'per_point: bool = False) -> octreelib_amd.registration.RegistrationSystem',
                                  True),
    'point_to_plane': ('(self, points, pose_numbers: Optional[List[int]] = None, min_points: int = 8, max_variance: '
                       'Optional[float] = None) -> octreelib_amd.query.PointToPlane',
                       True),
    'prune': ('(self)', True),
    'radius_count': ('(self, points, radius, *, max_count: Optional[int] = None, pose_numbers: Optional[List[int]] = '
                     'None) -> numpy.ndarray',
                     True),
    'ray_evidence': ('(self, origins, directions, ranges, margin, min_range=0.0, returned=None) -> '
                     'octreelib_amd.query.RayEvidence',
                     True),
    'raycast': ('(self, origins, directions, max_range, *, min_range=0.0, pose_numbers: Optional[List[int]] = None, '
                "surface: str = 'cube', min_points: Optional[int] = None, max_variance: Optional[float] = None) -> "
                'octreelib_amd.query.RayHits',
                True),
    'registration_system': ('(self, points, transform=None, pose_numbers: Optional[List[int]] = None, min_points: '
                            'int = 8, max_variance: Optional[float] = None, max_distance: Optional[float] = None, '
                            'huber_delta: Optional[float] = None, origin=None, per_point: bool = False) -> '
                            'octreelib_amd.registration.RegistrationSystem',
                            True),
    'remove_poses': ('(self, pose_numbers: List[int]) -> int', True),
    'remove_sparse': ('(self, radius, min_neighbours: int, *, pose_numbers: Optional[List[int]] = None, among: '
                      'Optional[List[int]] = None) -> int',
                      True),
    'subdivide': ('(self, subdivision_criteria: List[Callable], pose_numbers: Optional[List[int]] = None)', False),
    'transform_poses': ('(self, transforms, pose_numbers: Optional[List[int]] = None) -> None', True),
}
SURFACE = {
    "Grid": {
        **_BOTH,
        'filter': ('(self, filtering_criteria: List[Callable])', False),
        'get_leaf_points': ('(self, pose_number: int, non_empty: bool = True) -> '
                            'List[octreelib_amd.internal.voxel.Voxel]',
                            False),
        'get_points': ('(self, pose_number: int)', False),
        'map_leaf_points_cuda_ransac': ('(self, poses_per_batch: int = 10, threshold: float = 0.01, '
                                        'hypotheses_number: int = 1024, initial_points_number: int = 6, *, '
                                        'hypotheses=None)',
                                        True),
        'n_points': ('(self, pose_number: int) -> int', False),
        'visualize': ('(self, config: octreelib_amd.grid.grid_base.VisualizationConfig = '
                      "VisualizationConfig(type=<GridVisualizationType.VOXEL: 'voxel'>, point_size=0.1, "
                      "line_width_size=0.01, line_color=16711680, filepath='visualization.html', seed=0, "
                      'unused_voxels=[])) -> None',
                      False),
    },
    "OctreeManager": {
        **_BOTH,
        'apply_mask': ('(self, mask, pose_number: int)', False),
        'filter': ('(self, filtering_criteria: List[Callable], pose_numbers: Optional[List[int]] = None)', False),
        'get_leaf_points': ('(self, non_empty: bool = True, pose_number: Optional[int] = None) -> '
                            'List[octreelib_amd.internal.voxel.Voxel]',
                            False),
        'get_points': ('(self, pose_number: Optional[int] = None)', False),
        'n_points': ('(self, pose_number: Optional[int] = None) -> int', False),
    },
    "Octree": {
        'align': ('(self, points, initial=None, min_points: int = 8, max_variance=None, max_distance=None, '
                  'huber_delta=None, max_iterations: int = 20, tolerance: float = 1e-09, damping: float = 0.0)',
                  True),
        'align_points': ('(self, points, initial=None, *, max_distance: float, huber_delta=None, max_iterations: '
                         'int = 20, tolerance: float = 1e-09, damping: float = 0.0)',
                         True),
        'apply_mask': ('(self, mask)', False),
        'carve': ('(self, evidence, min_through: int = 2, max_hits: int = 0) -> int', True),
        'carve_rays': ('(self, origins, directions, ranges, margin, min_range=0.0, returned=None, min_through: int = '
                       '2, max_hits: int = 0) -> int',
                       True),
        'filter': ('(self, filtering_criteria: List[Callable])', False),
        'get_leaf_points': ('(self, non_empty: bool = True) -> List[octreelib_amd.internal.voxel.Voxel]', False),
        'get_points': ('(self)', True),
        'insert_points': ('(self, points, *, transform=None, segment=None)', True),
        'leaf_planes': ('(self)', True),
        'leaf_statistics': ('(self) -> octreelib_amd.leaf_stats.LeafStatistics', True),
        'locate': ('(self, points) -> numpy.ndarray', True),
        'map_leaf_points': ('(self, function: Callable)', False),
        'nearest': ('(self, points, k: int = 1, *, max_distance: float)', True),
        'node_cubes': ('(self)', True),
        'plane_segments': ('(self, min_points: int = 8, max_variance=None, max_angle: float = 0.1, max_offset: '
                           'float = 0.05)',
                           True),
        'point_registration_system': ('(self, points, transform=None, *, max_distance: float, huber_delta=None, '
                                      'origin=None, per_point: bool = False)',
                                      True),
        'point_to_plane': ('(self, points, min_points: int = 8, max_variance=None)', True),
        'prune': ('(self)', True),
        'radius_count': ('(self, points, radius, *, max_count=None) -> numpy.ndarray', True),
        'ray_evidence': ('(self, origins, directions, ranges, margin, min_range=0.0, returned=None)', True),
        'raycast': ("(self, origins, directions, max_range, *, min_range=0.0, surface: str = 'cube', "
                    'min_points=None, max_variance=None)',
                    True),
        'registration_system': ('(self, points, transform=None, min_points: int = 8, max_variance=None, '
                                'max_distance=None, huber_delta=None, origin=None, per_point: bool = False)',
                                True),
        'remove_sparse': ('(self, radius, min_neighbours) -> int', True),
        'subdivide': ('(self, subdivision_criteria: List[Callable])', True),
        'subdivide_as': ("(self, other_octree: 'Octree')", True),
    },
}


@pytest.mark.parametrize("name", SHARED)
def test_shared_operation_is_written_once(name):
    assert name not in Grid.__dict__ and name not in OctreeManager.__dict__
    assert inspect.isfunction(getattr(Grid, name))      # an ordinary def, not a generated or forwarding object
    assert getattr(Grid, name) is getattr(OctreeManager, name)


@pytest.mark.parametrize("cls", [Grid, OctreeManager, Octree])
def test_public_surface_is_the_recorded_one(cls):
    want = SURFACE[cls.__name__]
    public = {n: getattr(cls, n) for n in dir(cls) if not n.startswith("_") and callable(getattr(cls, n))}
    assert sorted(public) == sorted(want)
    for name, (signature, had_doc) in want.items():
        assert str(inspect.signature(public[name])) == signature, name
        if had_doc:
            assert (public[name].__doc__ or "").strip(), f"{cls.__name__}.{name} lost its docstring"


UNKNOWN = 99


def _on_plug_types(name):
    """A Grid or an OctreeManager on the caller's own types that holds pose 0: 50 points in the unit cube."""
    points = np.random.default_rng(1).random((50, 3))
    if name == "OctreeManager":
        obj = OctreeManager(HostOctree, OctreeConfigBase(), np.zeros(3), 4.0)
        obj.insert_points(0, points)
    else:
        obj = Grid(GridConfig(octree_manager_type=HostManager, octree_type=HostOctree,
                              octree_config=OctreeConfigBase(), voxel_edge_length=2))
        # insert_points of the plug path buckets the voxels on the device (grid/_plugged.py): without a GPU the one
        # voxel goes to the plug by hand, as in tests/test_cpu_query.py
        obj._plug._managers[(0, 0, 0)] = HostManager(HostOctree, OctreeConfigBase(), np.zeros(3), 2)
        obj._plug._managers[(0, 0, 0)].insert_points(0, points)
        obj._plug._pose_voxels[0] = [(0, 0, 0)]
    assert obj._plug is not None
    return obj


@pytest.mark.parametrize("name", ["Grid", "OctreeManager"])
def test_plug_types_are_refused_by_name_before_the_pose_lookup(name):
    obj = _on_plug_types(name)
    refused = [
        (NotImplementedError, lambda: obj.carve(None, pose_numbers=[UNKNOWN])),
        (NotImplementedError, lambda: obj.carve_rays(None, None, None, None, pose_numbers=[UNKNOWN])),
        (NotImplementedError, lambda: obj.remove_sparse(0.1, 1, pose_numbers=[UNKNOWN], among=[UNKNOWN])),
        (NotImplementedError, lambda: obj.transform_poses([np.eye(4)], pose_numbers=[UNKNOWN])),
        (ValueError, lambda: obj.remove_poses([UNKNOWN])),
        (ValueError, lambda: obj.prune()),
    ]
    for error, call in refused:
        with pytest.raises(error) as raised:
            call()
        assert type(raised.value) is error      # (a KeyError is no ValueError; this keeps a subclass out too)
        assert "plug types" in str(raised.value) and name in str(raised.value)


@pytest.mark.parametrize("name", ["Grid", "OctreeManager"])
def test_queries_look_poses_up_in_the_plug_table(name):
    obj = _on_plug_types(name)
    q = np.full((1, 3), 0.5)
    with pytest.raises(KeyError):
        obj.nearest(q, max_distance=0.5, pose_numbers=[UNKNOWN])
    with pytest.raises(KeyError):
        obj.leaf_planes([UNKNOWN])
    assert obj._query_slots([0]) == [0] and obj._query_slots(None) is None    # pose numbers pass through
    assert obj.nearest(q, max_distance=0.5, pose_numbers=[0]).count.shape == (1,)
