"""Host-side mirror of the reference's function surface for the pairwise-registration hot path:
same names, positional order and return objects as ``ALL_FUNCTIONS.py`` (library variants, this
module's top level) and as the private copies pasted into scripts 1 and 2 (``script1`` / ``script2``
namespaces below).  SURVEY.md §8b lists the surface; App. C lists the quirks preserved here.

Everything heavy runs in ``libpcr_hip.so`` on the MI355X.  The multiscale loop body is ONE C-ABI call
(``pcr_multiscale_gicp``) so that the clouds stay resident in HBM across all scales.  The reference's
call-by-call sequences are replayed through the PointCloud stand-ins by the tests (tests/test_gpu_fgr.py,
tests/test_gpu_gicp.py), not here: this module is signatures, constants and one library call each.
"""
from __future__ import annotations

import numpy as np

from . import geometry as _g
from . import registration as _r

KNN_FILTRO = 30          # ALL_FUNCTIONS.py:280, 2_MGICP...py:134
STD_FILTRO = 1.0         # ALL_FUNCTIONS.py:281, 2_MGICP...py:135
KNN_NORMAIS = 20         # ALL_FUNCTIONS.py:301, 2_MGICP...py:152
RETENTION_A, RETENTION_B = 1.18397758, 5.09388767     # ALL_FUNCTIONS.py:241-242: share of the points a voxel grid keeps ~ a * exp(-b * voxel)


# ------------------------------------------------------------------------------- ALL_FUNCTIONS.py variants
def registro_FGR(source, target, voxel_size, _use_absolute_scale=True, seed=None):
    """ALL_FUNCTIONS.py:178-203: normals Hybrid(2v, 20), FPFH Hybrid(10v, 200), FGR option (1.4, absolute scale, decrease_mu, 2v, 300,
    0.95, int(0.2 * n_pontos)), feature-matching FGR.  Mutates ``source``/``target`` (adds normals), like the reference.  One library
    call (``pcr_registro_fgr``: each cloud is sorted and indexed once)."""
    return _r.registro_fgr(source, target, voxel_size, _use_absolute_scale, seed)


def GICP_robusto(source, target, max_corres_dist, initial_T, iterations):
    """ALL_FUNCTIONS.py:211-227: radius-0.20 normals, raw 30-NN covariances (``estimate_covariances()`` default search),
    GICP with ``GMLoss(k=1.0)``.  Mutates ``source``/``target`` (normals and covariances), like the reference."""
    for cloud in (source, target):
        cloud.estimate_normals(_g.KDTreeSearchParamRadius(radius=0.20))
    for cloud in (source, target):
        cloud.estimate_covariances()
    return _r.registration_icp(source, target, max_corres_dist, initial_T, _r.TransformationEstimationForGeneralizedICP(_r.GMLoss(k=1.0)),
                               _r.ICPConvergenceCriteria(max_iteration=iterations))


def registro_manual(source, target, picked_id_source, picked_id_target):
    """The compute half of ALL_FUNCTIONS.py:423-442: the point pairs a user picked in the two clouds (the reference's ``escolher_pontos``
    windows; the picking itself is not part of this package) give the starting pose of a registration,
    ``TransformationEstimationPointToPoint().compute_transformation`` over them.  At least 3 picks per cloud and as many in one as in the
    other, asserted as in the reference.  Returns ``T_inicial`` (4x4 float64, source -> target)."""
    from . import o3d
    assert (len(picked_id_source) >= 3 and len(picked_id_target) >= 3)
    assert (len(picked_id_source) == len(picked_id_target))
    corr = np.zeros((len(picked_id_source), 2))
    corr[:, 0] = picked_id_source
    corr[:, 1] = picked_id_target
    p2p = _r.TransformationEstimationPointToPoint()
    return p2p.compute_transformation(source, target, o3d.utility.Vector2iVector(corr))


def amostragem_multiescala_otimizada(nuvem, n_escalas, voxel_inicial, seed=None):
    """ALL_FUNCTIONS.py:233-254: one voxel grid at ``voxel_inicial`` and ``n_escalas - 1`` random subsets of it whose sizes imitate
    coarser voxel grids (retention model a*exp(-b*voxel), a = 1.18397758, b = 5.09388767, normalised as the reference does);
    returned as the reference returns them: the random subsets in reverse order of creation, the voxel cloud last.  ``seed``
    (not in the reference, whose draws come from Open3D's random device) makes the subsets repeatable."""
    base = nuvem.voxel_down_sample(voxel_inicial)
    voxels = voxel_inicial + voxel_inicial * np.arange(n_escalas)                    # the grids being imitated: v, 2v, 3v, ...
    share = RETENTION_A * np.exp(-RETENTION_B * voxels) * len(nuvem.points) / len(base.points)
    share = (share / np.linalg.norm(share))[1:10]                                    # the reference's normalisation; entry 0 is the voxel cloud itself
    subsets = [base.random_down_sample(share[k], seed=None if seed is None else seed + k) for k in range(n_escalas - 1)]
    return subsets[::-1] + [base]


def create_scales(n_scales):
    """ALL_FUNCTIONS.py:260-264: doubling voxel sizes [0.1, 0.2, 0.4, ...] (a product with a power of two is the repeated sum, bit for bit)."""
    return [0.1 * 2.0 ** k for k in range(n_scales)]


def radius_from_cloud_pair(source, target):
    """ALL_FUNCTIONS.py:1092-1101: mean of the cube roots of the two AABB volumes."""
    edge = [np.prod(c.get_max_bound() - c.get_min_bound()) ** (1 / 3) for c in (source, target)]
    return (edge[0] + edge[1]) / 2


def _multiscale(source, target, voxel_sizes, distances, itera_escala, T_ini):
    """The loop body of ALL_FUNCTIONS.py:286-312 / 2_MGICP...py:140-163 for all scales in one library call: per scale voxel grid ->
    outlier filter (30, 1.0) -> 20-NN normals -> GICP with L1Loss and criteria (1e-6, 1e-6, itera_escala), poses chained."""
    est = _r.TransformationEstimationForGeneralizedICP(_r.L1Loss())
    crit = _r.ICPConvergenceCriteria(relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=itera_escala)
    return _r.multiscale_gicp(source, target, voxel_sizes, distances, T_ini, est, crit, KNN_FILTRO, STD_FILTRO, KNN_NORMAIS)


def Multiscale_GICP(source, target, n_scales, itera_escala, T_ini):
    """ALL_FUNCTIONS.py:272-313: voxels 0.1*2^k coarse-to-fine, search radius = AABB radius * 2^-i."""
    radius = radius_from_cloud_pair(source, target)
    return _multiscale(source, target, create_scales(n_scales)[::-1], [radius * 2 ** -k for k in range(n_scales)], itera_escala, T_ini)


def Coarse_to_fine_FGR_M_GICP(source, target, voxel_size, seed=None):
    """ALL_FUNCTIONS.py:317-332 -> (RegistrationResult, 6x6 information matrix)."""
    coarse = registro_FGR(source, target, voxel_size, seed=seed)
    fine = Multiscale_GICP(source, target, 3, 100, coarse.transformation)                      # 3 scales, 100 iterations each (:320-321)
    return fine, _r.get_information_matrix_from_point_clouds(source, target, voxel_size, fine.transformation)


def calculate_RMSE_and_fitness(lista_nuvens, T_circuito, distancia):
    """ALL_FUNCTIONS.py:801-824: ``evaluate_registration`` of every pose of a circuit -- pose i moves cloud i+1 onto cloud i; with as
    many poses as clouds the last one closes the loop (cloud 0 onto the last cloud); any other count prints the reference's message
    and returns two empty lists."""
    n = len(lista_nuvens)
    if len(T_circuito) == n:
        pairs = [((i + 1) % n, i) for i in range(n)]
    elif len(T_circuito) == n - 1:
        pairs = [(i + 1, i) for i in range(n - 1)]
    else:
        print("The number of clouds and poses are inconsistent")
        return [], []
    results = [_r.evaluate_registration(lista_nuvens[s], lista_nuvens[t], distancia, T) for (s, t), T in zip(pairs, T_circuito)]
    return [r.inlier_rmse for r in results], [r.fitness for r in results]


def extract_eigen_features(pc):
    """ALL_FUNCTIONS.py:1033-1058 -> the 7-vector (lin, pla, esf, cur, ani, omn, eig_sum) of eigenvalue features of a cloud.  The points are
    centred on ``get_center()`` and scaled by the larger norm of their per-axis maxima and minima; the singular values of the covariance of
    THAT cloud (``compute_mean_and_covariance``) give eig_sum as they are and the six ratios after division by their norm -- ``ani`` as the
    reference has it, s0 - s2 / s0, not (s0 - s2) / s0.  The scaled cloud is a stand-in cloud too, so its points are float32 (the reference
    keeps float64 there): the features agree with the reference to float32 rounding of the points."""
    offsets = np.asarray(pc.points) - pc.get_center()
    extent = max(np.linalg.norm(offsets.max(axis=0)), np.linalg.norm(offsets.min(axis=0)))
    _, cov = _g.PointCloud(offsets / extent).compute_mean_and_covariance()
    sv = np.linalg.svd(cov, compute_uv=False)
    s0, s1, s2 = sv / np.linalg.norm(sv)
    return np.array([(s0 - s1) / s0,                  # lin
                     (s1 - s2) / s0,                  # pla
                     s2 / s0,                         # esf
                     s2 / (s0 + s1 + s2),             # cur
                     s0 - s2 / s0,                    # ani
                     (s0 * s1 * s2) ** (1 / 3),       # omn
                     sv[0] + sv[1] + sv[2]])          # eig_sum, of the singular values before they are normalised


KNN_DISTANCE_LABELS = ("Voxel downsampling", "Hybrid downsampling")      # ALL_FUNCTIONS.py:1080, :1082


def knn_distance_table(pc1, pc2):
    """The data half of ``plot_cloud_knn_distances`` (ALL_FUNCTIONS.py:1076-1084): the nearest-neighbour distances of the two clouds
    with the class label the reference gives each, as ``[(distances1, label1), (distances2, label2)]`` -- the two columns of its data
    frame per cloud.  The box plot itself (pandas, seaborn) is not part of this package."""
    return [(pc.compute_nearest_neighbor_distance(), label) for pc, label in zip((pc1, pc2), KNN_DISTANCE_LABELS)]


def remove_small_clusters(cloud, eps, min_points, min_cluster_size):
    """DBSCAN (``cluster_dbscan(eps, min_points)``) as a filter, not in the reference: keeps the points whose cluster has at least
    ``min_cluster_size`` members -- the large static structures of a scan, without the small movable ones -- and drops the noise.  Returns
    ``(PointCloud, indices)``; the indices are a device int64 tensor, ascending.  Labels, counts and selection stay on the device."""
    import torch
    labels, _, n_clusters = _g._cluster_dbscan(cloud, eps, min_points)
    labels = labels.long()
    sizes = torch.bincount(labels[labels >= 0], minlength=max(n_clusters, 1))
    keep = (labels >= 0) & (sizes[labels.clamp(min=0)] >= int(min_cluster_size))
    indices = torch.nonzero(keep).reshape(-1)
    return cloud.select_by_index(indices), indices


def remove_plane(cloud, distance_threshold, ransac_n=3, num_iterations=100, probability=0.99999999, seed=None):
    """``segment_plane`` as a filter, not in the reference: takes the dominant plane -- the ground of a LiDAR scan, which would otherwise join
    every object standing on it into one DBSCAN cluster -- out of the cloud.  Returns ``(rest, plane_model, removed)``: the cloud without the
    plane's inliers, the plane ``(a, b, c, d)`` (numpy float64) and the removed rows as a device int64 tensor, ascending.  Mask and selection
    stay on the device."""
    import torch
    plane, removed, info = _g._segment_plane(cloud, distance_threshold, ransac_n, num_iterations, probability, seed)
    return cloud.select_by_index(torch.nonzero(~info["mask"]).reshape(-1)), plane, removed


def remove_boundary_points(cloud, radius, max_nn=30, angle_threshold=90.0):
    """``compute_boundary_points`` as a filter, not in the reference: takes the rim of the sampled surface -- where normals and FPFH rows come
    from half a neighbourhood -- out of the cloud.  Returns ``(interior, removed)``: the cloud without its boundary points and the removed rows
    as a device int64 tensor, ascending.  Mask and selection stay on the device."""
    import torch
    radius, max_nn, angle_threshold = _g._boundary_args(radius, max_nn, angle_threshold)
    cloud._need_normals("remove_boundary_points")
    removed, mask, _, _ = _g._boundary_call(cloud, radius, max_nn, angle_threshold)
    return cloud.select_by_index(torch.nonzero(~mask).reshape(-1)), removed


# ------------------------------------------------------------------------------------ script variants
class script1:
    """Private copies in 1_FGR_pairwise_registration_in_NCLT_dataset.py."""

    @staticmethod
    def registro_FGR(source, target, voxel_size, seed=None):
        """Script 1:41-66: identical to the library version except ``use_absolute_scale=False`` (:54)."""
        return registro_FGR(source, target, voxel_size, _use_absolute_scale=False, seed=seed)


class script2:
    """Private copies in 2_MGICP_refinement_in_NCLT_dataset.py."""

    @staticmethod
    def create_scales(n_scales):
        """Script 2:102-106: linear voxel sizes, already coarse-to-fine."""
        return [0.1 + 0.1 * k for k in reversed(range(n_scales))]

    @staticmethod
    def max_correspondence_distances(scales):
        """Script 2:112-120 (defined for 3, 4 or 5 scales only; other counts raise like the reference's
        UnboundLocalError, here as a ValueError subclass-compatible NameError)."""
        factors = {3: (3, 2, 1), 4: (3, 2.5, 2, 1), 5: (3, 2.5, 2, 1.5, 1)}.get(len(scales))
        if factors is None:
            raise UnboundLocalError("local variable 'max_correspondence_distances' referenced before assignment")
        return [f * v for f, v in zip(factors, scales)]

    @staticmethod
    def Multiscale_GICP(source, target, n_scales, itera_escala, T_ini):
        """Script 2:128-164."""
        voxel_sizes = script2.create_scales(n_scales)
        search_distances = script2.max_correspondence_distances(voxel_sizes)
        return _multiscale(source, target, voxel_sizes, search_distances, itera_escala, T_ini)
