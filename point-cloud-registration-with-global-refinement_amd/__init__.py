"""MI355X-native pairwise point-cloud registration (FGR + multiscale GICP) behind the reference's
``ALL_FUNCTIONS.py`` call surface.  Compute lives in ``libpcr_hip.so`` (``csrc/``, C ABI in
``include/pcr_hip.h``); this package is the host-side mirror of the reference interface.

The directory name contains hyphens; import it with ``importlib.import_module`` or through the
``pcr_amd`` alias module at the repository root.
"""
from . import _lib, drivers, functions, geometry, io, multiway, o3d, place, posegraph, refinement, registration, search, sharding  # noqa: F401
from .functions import (Coarse_to_fine_FGR_M_GICP, GICP_robusto, Multiscale_GICP, amostragem_multiescala_otimizada, calculate_RMSE_and_fitness,  # noqa: F401
                        create_scales, extract_eigen_features, knn_distance_table, radius_from_cloud_pair, registro_FGR, registro_manual, remove_boundary_points, remove_plane, remove_small_clusters,
                        script1, script2)
from .geometry import (KDTreeSearchParamHybrid, KDTreeSearchParamKNN, KDTreeSearchParamRadius, PointCloud, boundary_point_indices, compute_iss_keypoints,  # noqa: F401
                       euclidean_minimum_spanning_tree, farthest_point_indices, iss_keypoint_indices)
from .place import ScanContextDatabase, scan_context, scan_context_distance, shift_to_transformation  # noqa: F401
from .multiway import MultiwayProblem, MultiwayResult, circuit_edges, expand_edge, multiway_registration  # noqa: F401
from .posegraph import loop_closure_edges, pose_graph_from_odometry, refine_pose_graph  # noqa: F401
from .registration import (SpatialCompatibility, SpatialCompatibilityOption, registration_sc2_based_on_correspondence,  # noqa: F401
                           registration_sc2_based_on_feature_matching, spatial_compatibility)
from .search import KDTreeFlann, NearestNeighborSearch  # noqa: F401

__version__ = "0.1.0"
