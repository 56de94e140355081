"""ctypes loader of ``libpcr_hip.so`` (C ABI: ``include/pcr_hip.h``).

There is NO CPU fallback: if the shared library is missing, or no HIP device is visible, every
compute entry point raises ``RuntimeError`` (the CPU oracle under ``oracle/`` is test
infrastructure and is never imported from here).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("PCR_HIP_SO") or os.path.join(_HERE, "libpcr_hip.so")      # (PCR_HIP_SO: diagnostic builds of tools/build_variant.sh)

PCR_OK, PCR_EINVAL, PCR_ENOMEM, PCR_EHIP, PCR_ENUMERIC, PCR_ECAPACITY = 0, -1, -2, -3, -4, -5
PCR_DECLINED = 1          # pcr_debug_scale_clouds: the form asked for does not serve the inputs
SEARCH_KNN, SEARCH_RADIUS, SEARCH_HYBRID = 0, 1, 2
LOSS_L2, LOSS_L1, LOSS_GM = 0, 1, 2


class PcrResult(C.Structure):
    _fields_ = [("transformation", C.c_double * 16), ("fitness", C.c_double), ("inlier_rmse", C.c_double),
                ("n_correspondences", C.c_int64), ("iterations", C.c_int32), ("converged", C.c_int32)]


class PcrGicpParams(C.Structure):
    _fields_ = [("loss", C.c_int32), ("loss_k", C.c_double), ("epsilon", C.c_double), ("relative_fitness", C.c_double),
                ("relative_rmse", C.c_double), ("max_iteration", C.c_int32)]


ICP_POINT_TO_POINT, ICP_POINT_TO_PLANE = 1, 2          # pcr_icp_estimation


class PcrIcpParams(C.Structure):
    _fields_ = [("estimation", C.c_int32), ("with_scaling", C.c_int32), ("loss", C.c_int32), ("loss_k", C.c_double),
                ("relative_fitness", C.c_double), ("relative_rmse", C.c_double), ("max_iteration", C.c_int32)]


class PcrColoredIcpParams(C.Structure):
    _fields_ = [("lambda_geometric", C.c_double), ("loss", C.c_int32), ("loss_k", C.c_double), ("relative_fitness", C.c_double),
                ("relative_rmse", C.c_double), ("max_iteration", C.c_int32)]


class PcrVgicpParams(C.Structure):
    _fields_ = [("loss", C.c_int32), ("loss_k", C.c_double), ("epsilon", C.c_double), ("relative_fitness", C.c_double),
                ("relative_rmse", C.c_double), ("max_iteration", C.c_int32), ("neighborhood", C.c_int32), ("min_points_per_voxel", C.c_int32)]


class PcrNdtParams(C.Structure):
    _fields_ = [("relative_fitness", C.c_double), ("relative_rmse", C.c_double), ("max_iteration", C.c_int32), ("neighborhood", C.c_int32),
                ("outlier_ratio", C.c_double)]


class PcrRansacParams(C.Structure):
    _fields_ = [("ransac_n", C.c_int32), ("with_scaling", C.c_int32), ("max_iteration", C.c_int32), ("confidence", C.c_double),
                ("seed", C.c_uint64), ("edge_length_threshold", C.c_double), ("distance_threshold", C.c_double),
                ("normal_angle_threshold", C.c_double)]


class PcrRansacInfo(C.Structure):
    _fields_ = [("iterations_run", C.c_int64), ("best_iteration", C.c_int64), ("n_valid", C.c_int64), ("n_corres", C.c_int64)]


class PcrSc2Option(C.Structure):
    _fields_ = [("inlier_threshold", C.c_double), ("nms_radius", C.c_double), ("k1", C.c_int32), ("k2", C.c_int32), ("seed_ratio", C.c_double),
                ("max_seeds", C.c_int32), ("refine_iterations", C.c_int32)]


class PcrSc2Info(C.Structure):
    _fields_ = [("n_corres", C.c_int64), ("n_seeds", C.c_int64), ("n_valid", C.c_int64), ("best_seed", C.c_int64), ("best_seed_count", C.c_int64),
                ("refine_iterations_run", C.c_int64)]


EST_POINT_TO_POINT, EST_POINT_TO_PLANE, EST_GENERALIZED_ICP = 1, 2, 3          # pcr_estimation_kind
MULTIWAY_TILE = 256          # PCR_MULTIWAY_TILE: source points per tile of pcr_multiway_linearize


class PcrEstimation(C.Structure):
    _fields_ = [("kind", C.c_int32), ("with_scaling", C.c_int32), ("loss", C.c_int32), ("loss_k", C.c_double), ("epsilon", C.c_double)]


class PcrPointMapParams(C.Structure):
    _fields_ = [("estimation", PcrEstimation), ("relative_fitness", C.c_double), ("relative_rmse", C.c_double), ("max_iteration", C.c_int32),
                ("neighborhood", C.c_int32)]


class PcrPlaneParams(C.Structure):
    _fields_ = [("ransac_n", C.c_int32), ("num_iterations", C.c_int32), ("probability", C.c_double), ("seed", C.c_uint64)]


class PcrPlaneInfo(C.Structure):
    _fields_ = [("iterations_run", C.c_int64), ("best_iteration", C.c_int64), ("n_valid", C.c_int64), ("n_inliers", C.c_int64),
                ("fitness", C.c_double), ("inlier_rmse", C.c_double)]


class PcrFpsInfo(C.Structure):
    _fields_ = [("form", C.c_int32), ("workgroups", C.c_int32), ("fell_back", C.c_int32), ("cover_dist2", C.c_double)]


class PcrOrientInfo(C.Structure):
    _fields_ = [("emst_rounds", C.c_int32), ("tree_rounds", C.c_int32), ("walked_rows", C.c_int64), ("n_flipped", C.c_int64), ("root", C.c_int64)]


class PcrScanContextParams(C.Structure):
    _fields_ = [("num_rings", C.c_int32), ("num_sectors", C.c_int32), ("max_range", C.c_double), ("height_offset", C.c_double)]


class PcrScanContextTables(C.Structure):
    _fields_ = [("ring_bound2", C.POINTER(C.c_double)), ("cos_k", C.POINTER(C.c_double)), ("sin_k", C.POINTER(C.c_double)), ("range2", C.c_double)]


class PcrScanContextInfo(C.Structure):
    _fields_ = [("used", C.c_int64), ("dropped_nonfinite", C.c_int64), ("dropped_range", C.c_int64)]


class PcrScaleRecord(C.Structure):
    _fields_ = [("n_voxel", C.c_int64 * 2), ("n_clean", C.c_int64 * 2), ("icp", PcrResult)]


class PcrPair(C.Structure):
    _fields_ = [("src_xyz", C.c_void_p), ("src_normals", C.c_void_p), ("n_src", C.c_int64),
                ("tgt_xyz", C.c_void_p), ("tgt_normals", C.c_void_p), ("n_tgt", C.c_int64),
                ("init_T", C.c_double * 16), ("records", C.POINTER(PcrScaleRecord)), ("correspondences", C.c_void_p),
                ("status", C.c_int32), ("error", C.c_char * 120)]


class PcrFgrOption(C.Structure):
    _fields_ = [("division_factor", C.c_double), ("use_absolute_scale", C.c_int32), ("decrease_mu", C.c_int32),
                ("maximum_correspondence_distance", C.c_double), ("iteration_number", C.c_int32),
                ("tuple_scale", C.c_double), ("maximum_tuple_count", C.c_int32), ("tuple_test", C.c_int32),
                ("seed", C.c_uint64)]


class PcrFgrParams(C.Structure):
    _fields_ = [("normal_radius", C.c_double), ("normal_max_nn", C.c_int32), ("feature_radius", C.c_double),
                ("feature_max_nn", C.c_int32), ("option", PcrFgrOption)]


class PcrPairsPlan(C.Structure):
    _fields_ = [("stage", C.c_int32), ("fgr", C.POINTER(PcrFgrParams)), ("voxel_sizes", C.POINTER(C.c_double)),
                ("max_distances", C.POINTER(C.c_double)), ("n_scales", C.c_int32), ("radius_rule", C.c_int32),
                ("sor_k", C.c_int32), ("sor_std", C.c_double), ("normal_k", C.c_int32), ("gicp", C.POINTER(PcrGicpParams)),
                ("gicp_prior_from_fgr", C.c_int32), ("info_max_dist", C.c_double), ("inflight", C.c_int32), ("group", C.c_int32), ("pair_forms", C.c_int32), ("fgr_group", C.c_int32)]


class PcrPairEx(C.Structure):
    _fields_ = [("base", PcrPair), ("fgr", PcrResult), ("src_normals_out", C.c_void_p), ("tgt_normals_out", C.c_void_p),
                ("max_distances", C.c_double * 8), ("info36", C.c_double * 36)]


STAGE_GICP, STAGE_FGR, STAGE_FGR_GICP = 1, 2, 3

# every symbol include/pcr_hip.h declares (tests check the export table against this list)
EXPORTS = [
    "pcr_create", "pcr_destroy", "pcr_set_stream", "pcr_last_error", "pcr_version", "pcr_bounds",
    "pcr_voxel_down_sample", "pcr_remove_statistical_outlier", "pcr_estimate_normals", "pcr_estimate_covariances",
    "pcr_registration_generalized_icp", "pcr_multiscale_gicp", "pcr_evaluate_registration", "pcr_information_matrix",
    "pcr_compute_fpfh_feature", "pcr_registration_fgr", "pcr_debug_knn", "pcr_debug_gicp_linearize",
    "pcr_profile_enable", "pcr_profile_read", "pcr_registration_generalized_icp_cov", "pcr_register_pairs", "pcr_pool_profile",
    "pcr_registro_fgr", "pcr_register_pairs_plan", "pcr_debug_feature_nn", "pcr_set_option", "pcr_counter", "pcr_debug_radius_lists", "pcr_debug_voxel_grids",
    "pcr_debug_scale_clouds",
    "pcr_registration_icp", "pcr_registration_ransac_correspondence", "pcr_registration_ransac_feature_matching", "pcr_debug_ransac_hypotheses",
    "pcr_registration_colored_icp", "pcr_color_gradient", "pcr_voxel_down_sample_ex",
    "pcr_nearest_neighbor_distance", "pcr_point_cloud_distance", "pcr_remove_radius_outlier", "pcr_mean_and_covariance",
    "pcr_iss_keypoints", "pcr_cluster_dbscan", "pcr_segment_plane", "pcr_debug_plane_hypotheses",
    "pcr_index_create", "pcr_index_destroy", "pcr_index_knn", "pcr_index_hybrid", "pcr_index_radius_count", "pcr_index_radius_fill",
    "pcr_farthest_point_sample",
    "pcr_euclidean_mst", "pcr_orient_normals_tangent_plane", "pcr_orient_normals", "pcr_normalize_normals",
    "pcr_estimation_compute_transformation", "pcr_estimation_compute_rmse", "pcr_correspondences_from_features", "pcr_registration_fgr_correspondence",
    "pcr_boundary_points",
    "pcr_voxel_map_create", "pcr_voxel_map_destroy", "pcr_voxel_map_size", "pcr_voxel_map_read", "pcr_voxel_map_correspondences",
    "pcr_registration_voxelized_gicp",
    "pcr_voxel_map_create_on_grid", "pcr_voxel_map_insert", "pcr_voxel_map_merge", "pcr_voxel_map_remove_far", "pcr_voxel_map_grid",
    "pcr_scan_context", "pcr_scan_context_distance",
    "pcr_multiway_create", "pcr_multiway_destroy", "pcr_multiway_linearize",
    "pcr_ndt_map_create", "pcr_ndt_map_destroy", "pcr_ndt_map_size", "pcr_ndt_map_read", "pcr_ndt_map_grid", "pcr_ndt_map_correspondences",
    "pcr_ndt_linearize", "pcr_registration_ndt",
    "pcr_ndt_map_create_on_grid", "pcr_ndt_map_insert", "pcr_ndt_map_merge", "pcr_ndt_map_remove_far", "pcr_ndt_map_rule",
    "pcr_registration_sc2_correspondence", "pcr_spatial_compatibility", "pcr_debug_sc2_seeds",
    "pcr_point_map_create", "pcr_point_map_create_on_grid", "pcr_point_map_destroy", "pcr_point_map_size", "pcr_point_map_read", "pcr_point_map_grid",
    "pcr_point_map_insert", "pcr_point_map_merge", "pcr_point_map_remove_far", "pcr_point_map_correspondences", "pcr_point_map_linearize",
    "pcr_registration_point_map", "pcr_point_map_estimate_normals", "pcr_point_map_read_normal_counts", "pcr_point_map_normal_rule",
    "pcr_deskew", "pcr_point_map_linearize_continuous",
]

# prototypes of the cloud queries, the keypoint detector, the clustering, the plane segmentation, the search index, the farthest point sampler, the normal orientation, the calls on a correspondence list, the boundary detector and the multiway problem (include/pcr_hip.h), set on the handle by load(): (argtypes, restype)
QUERY_PROTOTYPES = {
    "pcr_nearest_neighbor_distance": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p], C.c_int),
    "pcr_point_cloud_distance": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p], C.c_int),
    "pcr_remove_radius_outlier": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_int64)], C.c_int),
    "pcr_mean_and_covariance": ([C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double)], C.c_int),
    "pcr_iss_keypoints": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                           C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.POINTER(C.c_double)], C.c_int),
    "pcr_cluster_dbscan": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)], C.c_int),
    "pcr_segment_plane": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.POINTER(PcrPlaneParams), C.POINTER(C.c_double), C.c_void_p, C.c_void_p,
                           C.POINTER(C.c_int64), C.POINTER(PcrPlaneInfo)], C.c_int),
    "pcr_debug_plane_hypotheses": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.POINTER(PcrPlaneParams), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p], C.c_int),
    "pcr_index_create": ([C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)], C.c_int),
    "pcr_index_destroy": ([C.c_void_p], C.c_int),
    "pcr_index_knn": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p], C.c_int),
    "pcr_index_hybrid": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "pcr_index_radius_count": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p], C.c_int),
    "pcr_index_radius_fill": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int], C.c_int),
    "pcr_farthest_point_sample": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(PcrFpsInfo)], C.c_int),
    "pcr_euclidean_mst": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(PcrOrientInfo)], C.c_int),
    "pcr_orient_normals_tangent_plane": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(PcrOrientInfo)], C.c_int),
    "pcr_orient_normals": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_double)], C.c_int),
    "pcr_normalize_normals": ([C.c_void_p, C.c_void_p, C.c_int64], C.c_int),
    "pcr_estimation_compute_transformation": ([C.c_void_p, C.POINTER(PcrEstimation), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_double)], C.c_int),
    "pcr_estimation_compute_rmse": ([C.c_void_p, C.POINTER(PcrEstimation), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_double)], C.c_int),
    "pcr_correspondences_from_features": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_void_p,
                                           C.POINTER(C.c_int64)], C.c_int),
    "pcr_registration_fgr_correspondence": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(PcrFgrOption),
                                             C.POINTER(PcrResult), C.c_void_p], C.c_int),
    "pcr_boundary_points": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.POINTER(C.c_int64), C.c_void_p, C.c_void_p], C.c_int),
    "pcr_voxel_map_create": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.POINTER(C.c_void_p)], C.c_int),
    "pcr_voxel_map_destroy": ([C.c_void_p], C.c_int),
    "pcr_voxel_map_size": ([C.c_void_p, C.POINTER(C.c_int64)], C.c_int),
    "pcr_voxel_map_read": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "pcr_voxel_map_correspondences": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_void_p,
                                       C.POINTER(C.c_int64)], C.c_int),
    "pcr_registration_voxelized_gicp": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_double), C.POINTER(PcrVgicpParams),
                                         C.POINTER(PcrResult), C.c_void_p], C.c_int),
    "pcr_voxel_map_create_on_grid": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_void_p)], C.c_int),
    "pcr_voxel_map_insert": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.POINTER(C.c_double)], C.c_int),
    "pcr_voxel_map_merge": ([C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "pcr_voxel_map_remove_far": ([C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_int64)], C.c_int),
    "pcr_voxel_map_grid": ([C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)], C.c_int),
    "pcr_scan_context": ([C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(PcrScanContextParams), C.POINTER(PcrScanContextTables), C.c_void_p,
                          C.POINTER(PcrScanContextInfo)], C.c_int),
    "pcr_scan_context_distance": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p], C.c_int),
    "pcr_multiway_create": ([C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_void_p)], C.c_int),
    "pcr_multiway_destroy": ([C.c_void_p], C.c_int),
    "pcr_multiway_linearize": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.c_double, C.POINTER(PcrEstimation), C.POINTER(C.c_double),
                                C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_void_p], C.c_int),
    "pcr_ndt_map_create": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int, C.c_double, C.POINTER(C.c_void_p)], C.c_int),
    "pcr_ndt_map_destroy": ([C.c_void_p], C.c_int),
    "pcr_ndt_map_size": ([C.c_void_p, C.POINTER(C.c_int64)], C.c_int),
    "pcr_ndt_map_read": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "pcr_ndt_map_grid": ([C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)], C.c_int),
    "pcr_ndt_map_correspondences": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.c_int, C.c_void_p, C.POINTER(C.c_int64)], C.c_int),
    "pcr_ndt_linearize": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                           C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)], C.c_int),
    "pcr_registration_ndt": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_double), C.POINTER(PcrNdtParams), C.POINTER(PcrResult), C.c_void_p], C.c_int),
    "pcr_ndt_map_create_on_grid": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    C.POINTER(C.c_void_p)], C.c_int),
    "pcr_ndt_map_insert": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double)], C.c_int),
    "pcr_ndt_map_merge": ([C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "pcr_ndt_map_remove_far": ([C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_int64)], C.c_int),
    "pcr_ndt_map_rule": ([C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double)], C.c_int),
    "pcr_registration_sc2_correspondence": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(PcrSc2Option),
                                             C.POINTER(PcrResult), C.c_void_p, C.POINTER(PcrSc2Info)], C.c_int),
    "pcr_spatial_compatibility": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p,
                                   C.c_void_p], C.c_int),
    "pcr_debug_sc2_seeds": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(PcrSc2Option), C.POINTER(C.c_int64),
                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "pcr_point_map_create": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int, C.POINTER(C.c_void_p)], C.c_int),
    "pcr_point_map_create_on_grid": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_void_p)], C.c_int),
    "pcr_point_map_destroy": ([C.c_void_p], C.c_int),
    "pcr_point_map_size": ([C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)], C.c_int),
    "pcr_point_map_read": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "pcr_point_map_grid": ([C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
    "pcr_point_map_estimate_normals": ([C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_int64)], C.c_int),
    "pcr_point_map_read_normal_counts": ([C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "pcr_point_map_normal_rule": ([C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int)], C.c_int),
    "pcr_point_map_insert": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double)], C.c_int),
    "pcr_point_map_merge": ([C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "pcr_point_map_remove_far": ([C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_int64)], C.c_int),
    "pcr_point_map_correspondences": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.c_double, C.c_int, C.c_void_p,
                                       C.POINTER(C.c_int64)], C.c_int),
    "pcr_point_map_linearize": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.c_double, C.c_int, C.POINTER(PcrEstimation),
                                 C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)], C.c_int),
    "pcr_registration_point_map": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.POINTER(C.c_double), C.POINTER(PcrPointMapParams),
                                    C.POINTER(PcrResult), C.c_void_p], C.c_int),
    "pcr_deskew": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p], C.c_int),
    "pcr_point_map_linearize_continuous": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_double,
                                            C.c_double, C.c_int, C.POINTER(PcrEstimation), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                            C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p], C.c_int),
    "pcr_debug_scale_clouds": ([C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
}

_lib = None
_lock = threading.Lock()


def build(force: bool = False) -> str:
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    script = os.path.join(_HERE, "csrc", "build.sh")
    env = dict(os.environ)
    if force:
        for f in os.listdir(os.path.join(_HERE, "csrc")):
            if f.endswith(".o"):
                os.remove(os.path.join(_HERE, "csrc", f))
    subprocess.check_call(["bash", script], env=env)
    return SO_PATH


def load():
    """Return the ctypes handle of libpcr_hip.so; raise RuntimeError if it is not built."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(SO_PATH):
                raise RuntimeError(
                    f"libpcr_hip.so not found at {SO_PATH}: the HIP extension is not built "
                    "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
            # torch bundles its own HIP runtime: load it FIRST so that libpcr_hip.so binds to the same one
            # (two HIP runtimes in one process cannot share a device context)
            import torch  # noqa: F401
            lib = C.CDLL(SO_PATH)
            lib.pcr_last_error.restype = C.c_char_p
            lib.pcr_last_error.argtypes = [C.c_void_p]
            lib.pcr_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
            lib.pcr_destroy.argtypes = [C.c_void_p]
            lib.pcr_set_stream.argtypes = [C.c_void_p, C.c_void_p]
            if hasattr(lib, "pcr_set_option"):       # (absent only from older diagnostic builds loaded through PCR_HIP_SO)
                lib.pcr_set_option.argtypes = [C.c_char_p, C.c_longlong]
            for name, (argtypes, restype) in QUERY_PROTOTYPES.items():
                if not hasattr(lib, name):
                    raise RuntimeError(f"{SO_PATH} does not export {name}: it was built from older sources (rebuild it; see include/pcr_hip.h)")
                fn = getattr(lib, name)
                fn.argtypes, fn.restype = argtypes, restype
            _lib = lib
    return _lib


def counter(name: str, reset: bool = False) -> int:
    """Process-wide event counter of the library (``pcr_counter``, include/pcr_hip.h), e.g. ``counter("fgr_group_barrier_timeouts")``."""
    lib = load()
    lib.pcr_counter.argtypes = [C.c_char_p, C.c_int]; lib.pcr_counter.restype = C.c_longlong
    v = int(lib.pcr_counter(name.encode(), int(bool(reset))))
    if v < 0:
        raise ValueError(f"pcr_counter: unknown counter {name!r}")
    return v


def set_option(name: str, value: int) -> None:
    """Test / diagnostic switch of the process (``pcr_set_option``, include/pcr_hip.h), e.g. ``set_option("knn_wave", 1)``."""
    rc = load().pcr_set_option(name.encode(), int(value))
    if rc != PCR_OK:
        raise ValueError(f"pcr_set_option: unknown option {name!r}")


def debug_scale_clouds(clouds, priors, voxels, sor_k, sor_std, normal_k, form, fill=-7.0):
    """Test hook ``pcr_debug_scale_clouds`` (include/pcr_hip.h): the scale clouds the GICP loops consume, made by the preparation code of the
    path ``form`` names (0 scale by scale, 1 all scales of a cloud batched, 2 all clouds and scales as one batch).  clouds: float32 arrays
    (n x 3), cloud c a source for even c and a target for odd c; priors: None, or one array / None per cloud.  Returns None when the form
    declines, else ``out[c][s] = (points, normals, n_voxel, untouched)``: the cleaned rows in the loop's order, the rows of the voxel cloud,
    and whether every row past the clean count still holds ``fill``."""
    import numpy as np
    import torch
    ctx = Context.current()
    m, S = len(clouds), len(voxels)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)).cuda()
    dx = [up(p) for p in clouds]
    dn = [up(q) if q is not None else None for q in priors] if priors is not None else None
    ox = [torch.full((len(p), 3), fill, dtype=torch.float32, device="cuda") for p in dx for _ in range(S)]
    on = [torch.full((len(p), 3), fill, dtype=torch.float32, device="cuda") for p in dx for _ in range(S)]
    ptr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])
    nv = (C.c_int32 * (m * S))(*([-1] * (m * S))); nc = (C.c_int32 * (m * S))(*([-1] * (m * S)))
    torch.cuda.synchronize()
    rc = ctx.lib.pcr_debug_scale_clouds(ctx.handle, m, ptr(dx), ptr(dn) if dn is not None else None, (C.c_int64 * m)(*[len(p) for p in dx]),
                                        (C.c_double * S)(*voxels), S, int(sor_k), float(sor_std), int(normal_k), int(form), ptr(ox), ptr(on), nv, nc)
    torch.cuda.synchronize()
    if rc == PCR_DECLINED:
        if not (all((t == fill).all().item() for t in ox + on) and all(v == -1 for v in list(nv) + list(nc))):
            raise RuntimeError("pcr_debug_scale_clouds declined but wrote to the caller's buffers")
        return None
    ctx.check(rc, "debug_scale_clouds")
    out = []
    for c in range(m):
        row = []
        for s in range(S):
            k = c * S + s
            cnt = nc[k]
            untouched = bool((ox[k][cnt:] == fill).all().item() and (on[k][cnt:] == fill).all().item())
            row.append((ox[k][:cnt].cpu().numpy(), on[k][:cnt].cpu().numpy(), int(nv[k]), untouched))
        out.append(row)
    return out


class Context:
    """One libpcr_hip context (scratch arena + stream) per (device, torch stream, thread).

    The cache is bounded (least recently used contexts are destroyed: each holds a device arena of hundreds of MB) and guarded
    by a lock; ``close()`` destroys a context explicitly.  ``stream_ptr == 0`` is torch's default stream = the legacy default
    stream: the library then runs on a stream of its own and fences every call against the default stream on both sides
    (``pcr_set_stream(ctx, NULL)``, include/pcr_hip.h)."""

    _cache: "dict" = {}
    _cache_lock = threading.Lock()
    MAX_CACHED = 16

    def __init__(self, device: int, stream_ptr: int):
        lib = load()
        h = C.c_void_p()
        rc = lib.pcr_create(int(device), C.byref(h))
        if rc != PCR_OK:
            raise RuntimeError(f"pcr_create(device={device}) failed with code {rc}: no usable HIP device "
                               "(the MI355X path has no CPU fallback)")
        self.handle = h
        self.device = device
        self.lib = lib
        lib.pcr_set_stream(h, C.c_void_p(stream_ptr))

    def close(self):
        """Destroy the library context (waits for its stream, frees the arena)."""
        h, self.handle = self.handle, None
        if h is not None and h.value:
            self.lib.pcr_destroy(h)

    @classmethod
    def current(cls) -> "Context":
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible to torch: the MI355X registration path cannot run (no CPU fallback)")
        dev = torch.cuda.current_device()
        sp = int(torch.cuda.current_stream(dev).cuda_stream)
        key = (dev, sp, threading.get_ident())
        stale = []
        with cls._cache_lock:
            ctx = cls._cache.pop(key, None)
            if ctx is None or ctx.handle is None:
                ctx = cls(dev, sp)
            cls._cache[key] = ctx                       # most recently used last
            while len(cls._cache) > cls.MAX_CACHED:
                stale.append(cls._cache.pop(next(iter(cls._cache))))
        for c in stale:
            c.close()
        return ctx

    @classmethod
    def close_all(cls):
        with cls._cache_lock:
            ctxs = list(cls._cache.values()); cls._cache.clear()
        for c in ctxs:
            c.close()

    def check(self, rc: int, what: str):
        if rc == PCR_OK:
            return
        msg = self.lib.pcr_last_error(self.handle)
        msg = msg.decode() if msg else ""
        # Open3D raises RuntimeError for invalid arguments; mirror that (SURVEY.md §8b error convention)
        raise RuntimeError(f"{what}: {msg} (pcr status {rc})")
