"""
octreelib_amd - MI355X-native implementation of octreelib's point-cloud -> octree-grid
build-and-query path (Grid / OctreeManager / Octree / ransac), as a drop-in for that path:

    from octreelib_amd.grid import Grid, GridConfig
    from octreelib_amd.octree import Octree, OctreeConfig
    from octreelib_amd.octree_manager import OctreeManager
    from octreelib_amd.ransac import CudaRansac

Python host code over a C ABI (include/octreelib_hip.h, ctypes) over hand-written HIP kernels
for gfx950.  There is no CPU fallback: without liboctree_hip.so and a GPU every operation
raises.
"""

from octreelib_amd.adjustment import (Adjustment, AdjustmentLeaves, AdjustmentSystem, BlockMoments, adjust_np,
                                      adjustment_system_np, block_moments_np)
from octreelib_amd.clustering import (Clusters, check_cluster_args, cluster, cluster_labels_np, remove_small_clusters,
                                      small_cluster_keep_np)
from octreelib_amd.criteria import MaxPoints, NotPlanar
from octreelib_amd.feed import DeviceCloud, ScanPipeline, pinned_empty, upload_async
from octreelib_amd.query import (LeafPlanes, Neighbours, PlaneSegments, PointToPlane, PruneResult, RayEvidence,
                                 RayHits, carve_keep_np, locate_np, nearest_np, normalize_directions, plane_segments_np,
                                 point_to_plane_np, pooled_leaf_statistics_np, prune_np, radius_count_np, ray_evidence_np,
                                 raycast_np, sparse_keep_np)
from octreelib_amd.matching import align_nearest_planes, nearest_plane_registration_system
from octreelib_amd.neighbourhood import (PointStatistics, neighbourhood_statistics, neighbourhood_statistics_np,
                                         orient_towards, point_statistics, point_statistics_np)
from octreelib_amd.registration import (Alignment, RegistrationSystem, align_np, nearest_plane_registration_system_np,
                                        point_registration_system_np, registration_system_np, se3_exp, transform_np,
                                        transform_rows_np)
from octreelib_amd.thinning import cell_count, cell_count_np, cell_index_np, check_cell_args, thin, thin_keep_np

__version__ = "0.1.0"
__all__ = ["MaxPoints", "NotPlanar", "DeviceCloud", "ScanPipeline", "pinned_empty", "upload_async", "LeafPlanes",
           "PointToPlane", "locate_np", "pooled_leaf_statistics_np", "point_to_plane_np", "RegistrationSystem",
           "Alignment", "registration_system_np", "point_registration_system_np", "align_np", "se3_exp",
           "transform_np", "transform_rows_np", "AdjustmentSystem", "Adjustment",
           "AdjustmentLeaves", "BlockMoments", "adjustment_system_np", "adjust_np", "block_moments_np", "Neighbours",
           "nearest_np", "PlaneSegments", "plane_segments_np", "RayHits", "raycast_np", "normalize_directions",
           "RayEvidence", "ray_evidence_np", "carve_keep_np", "PruneResult", "prune_np", "radius_count_np",
           "sparse_keep_np", "nearest_plane_registration_system_np", "nearest_plane_registration_system",
           "align_nearest_planes", "cell_index_np", "cell_count_np", "thin_keep_np", "check_cell_args", "cell_count",
           "thin", "PointStatistics", "neighbourhood_statistics", "neighbourhood_statistics_np", "point_statistics",
           "point_statistics_np", "orient_towards", "Clusters", "cluster_labels_np", "small_cluster_keep_np",
           "check_cluster_args", "cluster", "remove_small_clusters", "__version__"]
