/*
 * pcr_hip.h -- C ABI of libpcr_hip.so, the MI355X (gfx950) pairwise-registration hot path.
 *
 * The reference has no FFI of its own: its hot path is reached through Open3D's pybind
 * module from ALL_FUNCTIONS.py / scripts 1-2.  Each entry point below
 * therefore names the Open3D binding call it replaces and the reference line that makes
 * that call.  INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every cloud/normal/feature pointer is a DEVICE pointer (HIP, current device of the
 *     context); `T`, option structs and result structs are HOST pointers;
 *   - clouds are packed float32 xyz rows (N x 3), normals likewise, FPFH is N x 33 float32;
 *   - poses are row-major 4x4 float64, source -> target;
 *   - caller owns every buffer; the library owns a per-context scratch arena;
 *   - return 0 on success, negative pcr_status otherwise; degenerate-but-valid results
 *     (no correspondences: fitness 0, rmse 0, T = init) are NOT errors (Open3D behaviour);
 *   - calls are ordered on the context's stream (pcr_set_stream).  Entry points with host outputs (counts, poses, results)
 *     return after those are on the host; entry points whose outputs are all device buffers (pcr_estimate_normals,
 *     pcr_estimate_covariances, pcr_compute_fpfh_feature, pcr_debug_knn, and the four searches pcr_index_knn, pcr_index_hybrid,
 *     pcr_index_radius_count, pcr_index_radius_fill) only enqueue and return;
 *   - stream NULL = the legacy default stream: the library works on a stream of its own and fences every call against the
 *     default stream on both sides (the call sees everything enqueued there before it; work enqueued there after the call
 *     sees its results);
 *   - every kernel launch is followed by hipGetLastError(); a failed launch turns the call into PCR_EHIP with file:line
 *     in pcr_last_error().
 */
#ifndef PCR_HIP_H
#define PCR_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PCR_OK = 0,
    PCR_EINVAL = -1,      /* Open3D would raise (voxel_size<=0, max_dist<=0, nb_neighbors<1, std_ratio<=0 ...) */
    PCR_ENOMEM = -2,
    PCR_EHIP = -3,        /* a HIP runtime call failed; see pcr_last_error() */
    PCR_ENUMERIC = -4,    /* non-finite pose */
    PCR_ECAPACITY = -5,   /* caller buffer too small */
    PCR_DECLINED = 1      /* pcr_debug_scale_clouds only: the form asked for does not serve these inputs; nothing was written */
} pcr_status;

/* == o3d.geometry.KDTreeSearchParam{KNN,Radius,Hybrid}  (ALL_FUNCTIONS.py:181,185,213,301) */
typedef enum { PCR_SEARCH_KNN = 0, PCR_SEARCH_RADIUS = 1, PCR_SEARCH_HYBRID = 2 } pcr_search_kind;
/* == o3d.pipelines.registration.{L2Loss,L1Loss,GMLoss} (ALL_FUNCTIONS.py:219,284) */
typedef enum { PCR_LOSS_L2 = 0, PCR_LOSS_L1 = 1, PCR_LOSS_GM = 2 } pcr_loss_kind;

typedef struct pcr_context pcr_context;

/* == o3d.pipelines.registration.RegistrationResult (fields read at ALL_FUNCTIONS.py:312,323,369) */
typedef struct {
    double transformation[16];
    double fitness;
    double inlier_rmse;
    int64_t n_correspondences;
    int32_t iterations;       /* pose updates applied */
    int32_t converged;
} pcr_result;

/* == TransformationEstimationForGeneralizedICP(loss) + ICPConvergenceCriteria(...)
 *    (ALL_FUNCTIONS.py:308-311, 2_MGICP...py:159-162)                                   */
typedef struct {
    int32_t loss;             /* pcr_loss_kind */
    double loss_k;            /* GMLoss k */
    double epsilon;           /* GICP covariance regulariser, Open3D default 1e-3 */
    double relative_fitness;
    double relative_rmse;
    int32_t max_iteration;
} pcr_gicp_params;

/* == TransformationEstimationPointToPoint(with_scaling) / TransformationEstimationPointToPlane(kernel) + ICPConvergenceCriteria(...)
 *    (Open3D registration_icp; the reference itself only calls the GICP estimator)                                             */
typedef enum { PCR_ICP_POINT_TO_POINT = 1, PCR_ICP_POINT_TO_PLANE = 2 } pcr_icp_estimation;
typedef struct {
    int32_t estimation;       /* pcr_icp_estimation */
    int32_t with_scaling;     /* point-to-point: also estimate a uniform scale (Umeyama) */
    int32_t loss;             /* point-to-plane: pcr_loss_kind of the robust kernel */
    double loss_k;            /* GMLoss k */
    double relative_fitness;
    double relative_rmse;
    int32_t max_iteration;
} pcr_icp_params;

/* == TransformationEstimationForColoredICP(lambda_geometric, kernel) + ICPConvergenceCriteria(...)  (pcr_registration_colored_icp below) */
typedef struct {
    double lambda_geometric;  /* weight of the geometric term, 0.968; a value outside [0, 1] is reset to 0.968 */
    int32_t loss;             /* pcr_loss_kind of the robust kernel */
    double loss_k;            /* GMLoss k */
    double relative_fitness;
    double relative_rmse;
    int32_t max_iteration;
} pcr_colored_icp_params;

/* per-scale record of pcr_multiscale_gicp (what the roofline byte model needs) */
typedef struct {
    int64_t n_voxel[2];       /* D_k: source, target after voxel_down_sample           */
    int64_t n_clean[2];       /* C_k: after remove_statistical_outlier                 */
    pcr_result icp;
} pcr_scale_record;

/* == FastGlobalRegistrationOption (ALL_FUNCTIONS.py:189-196) */
typedef struct {
    double division_factor;
    int32_t use_absolute_scale;
    int32_t decrease_mu;
    double maximum_correspondence_distance;
    int32_t iteration_number;
    double tuple_scale;
    int32_t maximum_tuple_count;   /* pcr_registro_fgr / plans: < 0 = the reference's rule per pair, int(0.2 * int((n_src + n_tgt) / 2)) (ALL_FUNCTIONS.py:179,196) */
    int32_t tuple_test;
    uint64_t seed;            /* Open3D seeds from std::random_device; here explicit */
} pcr_fgr_option;

/* ---- context ---------------------------------------------------------------------- */
int pcr_create(int device, pcr_context **out);
int pcr_destroy(pcr_context *ctx);
int pcr_set_stream(pcr_context *ctx, void *hip_stream);       /* NULL = the legacy default stream (fenced, see above) */
const char *pcr_last_error(const pcr_context *ctx);
int pcr_version(void);

/* ---- geometry: PointCloud methods ------------------------------------------------- */
/* == PointCloud.get_min_bound/get_max_bound (ALL_FUNCTIONS.py:1093-1097); bounds6 host = min xyz, max xyz */
int pcr_bounds(pcr_context *ctx, const float *xyz, int64_t n, double *bounds6);

/* == PointCloud.voxel_down_sample (ALL_FUNCTIONS.py:293-294; 2_MGICP...py:146-147).
 * out capacity n rows. normals_in/out optional (mean, not re-normalised). Output is in Morton
 * order of the voxel index (Open3D's order is unspecified hash order).                      */
int pcr_voxel_down_sample(pcr_context *ctx, const float *xyz, const float *normals_in, int64_t n, double voxel_size,
                          float *out_xyz, float *out_normals, int64_t *out_n);

/* == PointCloud.voxel_down_sample of a cloud that also carries colours (N x 3 float32 in [0, 1], device; optional like the normals): out_colors
 * is the arithmetic mean per voxel, summed in float64 in input order like the points.  out_xyz and out_normals are bit for bit what
 * pcr_voxel_down_sample returns, in the same Morton order.                                                                             */
int pcr_voxel_down_sample_ex(pcr_context *ctx, const float *xyz, const float *normals_in, const float *colors_in, int64_t n, double voxel_size,
                             float *out_xyz, float *out_normals, float *out_colors, int64_t *out_n);

/* == PointCloud.remove_statistical_outlier (ALL_FUNCTIONS.py:297-298). keep_mask: n bytes (device),
 * out_xyz optional compacted cloud (capacity n), out_index optional int64 indices (device).      */
int pcr_remove_statistical_outlier(pcr_context *ctx, const float *xyz, int64_t n, int nb_neighbors, double std_ratio,
                                   uint8_t *keep_mask, float *out_xyz, int64_t *out_index, int64_t *out_n);

/* == PointCloud.estimate_normals(search_param) (ALL_FUNCTIONS.py:182-183, 214-215, 301-302).
 * prior_normals optional: new normal flipped to agree with it (Open3D when has_normals).         */
int pcr_estimate_normals(pcr_context *ctx, const float *xyz, int64_t n, int search_kind, int knn, double radius,
                         const float *prior_normals, float *normals);

/* == PointCloud.estimate_covariances(search_param) (ALL_FUNCTIONS.py:216-217); cov6 = xx,xy,xz,yy,yz,zz */
int pcr_estimate_covariances(pcr_context *ctx, const float *xyz, int64_t n, int search_kind, int knn, double radius,
                             float *cov6);

/* == PointCloud.compute_nearest_neighbor_distance (plot_cloud_knn_distances, ALL_FUNCTIONS.py:1077-1078).  dist: n float64 (device), caller order.
 * dist[i] = the square root of the SECOND smallest squared distance from point i to the points of the same cloud, point i itself included
 * (the second entry of Open3D's SearchKNN(p, 2)): a duplicated point gets 0, and with n < 2 every entry is 0.  The neighbour is selected by
 * float32 d^2 like the other exact searches; the distance is then recomputed in float64 from the float32 coordinates of the point and the chosen
 * neighbour -- differences, squares and sums in the order x, y, z, each rounded once -- and square-rooted in float64: exact for that neighbour,
 * which is a true second nearest up to a float32 tie.  Asynchronous on the context's stream. */
int pcr_nearest_neighbor_distance(pcr_context *ctx, const float *xyz, int64_t n, double *dist);

/* == PointCloud.compute_point_cloud_distance(target) (Open3D ComputePointCloudDistance; the reference judges pairs with the capped
 * evaluate_registration only).  dist: n_src float64 (device); dist[i] = distance from source point i to its nearest target point, the search
 * unbounded; nearest (optional, n_src int32, device) = that target point's caller index.  Selection and precision as for
 * pcr_nearest_neighbor_distance.  Among target points at the SAME float32 d^2 the one that comes first in the library's Morton order of the
 * target is returned, which need not be the one with the lowest caller index (in both calls; the distance is that of the point returned).
 * An empty target gives dist = 0 and nearest = -1; an empty source writes nothing.  Asynchronous. */
int pcr_point_cloud_distance(pcr_context *ctx, const float *src_xyz, int64_t n_src, const float *tgt_xyz, int64_t n_tgt,
                             double *dist, int32_t *nearest);

/* == PointCloud.remove_radius_outlier(nb_points, radius) (Open3D RemoveRadiusOutliers, the sibling of the filter at ALL_FUNCTIONS.py:297-298).
 * nb_points < 1 or radius <= 0: PCR_EINVAL.  Point i is kept iff the number of points of the cloud with d^2 < radius^2 -- point i included, the
 * test strict -- is GREATER than nb_points; d^2 in float64 on the float32 coordinates (the rule of the radius neighbourhoods of
 * pcr_estimate_normals).  The count may stop once it has passed nb_points.  keep_mask: n bytes (device, optional), out_xyz optional compacted
 * cloud (capacity n), out_index optional int64 indices (device), ascending: the layout of pcr_remove_statistical_outlier. */
int pcr_remove_radius_outlier(pcr_context *ctx, const float *xyz, int64_t n, int nb_points, double radius,
                              uint8_t *keep_mask, float *out_xyz, int64_t *out_index, int64_t *out_n);

/* == PointCloud.compute_mean_and_covariance / get_center (extract_eigen_features, ALL_FUNCTIONS.py:1035, :1043; colorir_voxels :1022).
 * mean3, cov9 (row-major 3x3) host, float64: the mean and the POPULATION covariance (divided by n) of the float32 points; n == 0 gives a zero
 * mean and the identity.  Float64 sums in a fixed order (same bits on every run), the second moments taken about the mean.  cov9 may be
 * NULL (get_center): the mean alone, the same bits, in one pass over the points instead of two. */
int pcr_mean_and_covariance(pcr_context *ctx, const float *xyz, int64_t n, double *mean3, double *cov9);

/* ============================================================================================ nearest-neighbour search index
 * == o3d.geometry.KDTreeFlann (SetGeometry, SearchKNN, SearchRadius, SearchHybrid) and o3d.core.nns.NearestNeighborSearch (knn_search,
 * fixed_radius_search, hybrid_search): an index over a cloud that outlives the call, searched with arbitrary query points.
 *
 * THE RESULT RULE, one for the three searches.  For a query q and a dataset point p, both float32 xyz, d^2 is taken in float64 --
 * differences, squares and sums in the order x, y, z, each rounded once, no fused multiply-add -- and the dataset is totally ordered for q
 * by (d^2, caller index of p), ascending.  knn: the first k points of that order, in that order.  radius: every point with d^2 < r^2, where
 * r^2 = radius * radius in float64 and the test is strict; sorted rows come in that order.  hybrid: the first max_nn of the radius set, in that
 * order.  The returned d^2 are those float64 values; there is no float32 tie clause, so a host recomputation gives the same rows bit for bit.
 *
 * All query, index and d^2 buffers are DEVICE buffers; rows are in the caller's query order and hold caller indices of the dataset.  A query
 * with a non-finite coordinate finds nothing.  Limits: k and max_nn in 1..200, radius > 0, m and n in 0..2^31 - 1; anything else is
 * PCR_EINVAL with a message.  The searches are asynchronous on the context's stream. */
typedef struct pcr_index pcr_index;

/* Builds the index over n float32 points (device): a Morton-sorted copy of the points with their caller indices and its octree, in ONE
 * device allocation of its own -- not in the context's arena, so the index survives the context that built it, and any context on the same
 * device may search it.  The build uses the context's arena as scratch and is finished when the call returns: the caller may free or
 * overwrite xyz.  n == 0 is valid: every search on such an index finds nothing. */
int pcr_index_create(pcr_context *ctx, const float *xyz, int64_t n, pcr_index **out);
/* Frees the index (waits for the device, so no search is still reading it).  NULL is allowed. */
int pcr_index_destroy(pcr_index *index);

/* == KDTreeFlann.search_knn_vector_3d / NearestNeighborSearch.knn_search.  idx: m x k int32, d2: m x k float64.  Places beyond the
 * dataset's size (k > n) hold idx = -1 and d2 = +inf. */
int pcr_index_knn(pcr_context *ctx, const pcr_index *index, const float *query_xyz, int64_t m, int k, int32_t *idx, double *d2);

/* == KDTreeFlann.search_hybrid_vector_3d / NearestNeighborSearch.hybrid_search.  idx: m x max_nn int32, d2: m x max_nn float64, counts: m int32 =
 * min(max_nn, size of the ball).  Places beyond the count hold idx = -1 and d2 = 0 (Open3D's padding). */
int pcr_index_hybrid(pcr_context *ctx, const pcr_index *index, const float *query_xyz, int64_t m, double radius, int max_nn,
                     int32_t *idx, double *d2, int32_t *counts);

/* == KDTreeFlann.search_radius_vector_3d / NearestNeighborSearch.fixed_radius_search, in two passes.  The count pass writes the size of every
 * query's ball (counts: m int32).  The caller scans the counts into row_splits (m + 1 int64, device, row_splits[0] = 0) and allocates idx and
 * d2 with row_splits[m] entries; the fill pass walks again and writes row i into [row_splits[i], row_splits[i + 1]) -- never beyond it.  With
 * sort != 0 every row obeys the order of the rule; with sort == 0 the order inside a row is free (the set is the same). */
int pcr_index_radius_count(pcr_context *ctx, const pcr_index *index, const float *query_xyz, int64_t m, double radius, int32_t *counts);
int pcr_index_radius_fill(pcr_context *ctx, const pcr_index *index, const float *query_xyz, int64_t m, double radius, const int64_t *row_splits,
                          int32_t *idx, double *d2, int sort);

/* == geometry.keypoint.compute_iss_keypoints (Open3D ComputeISSKeypoints, cpp/open3d/geometry/Keypoint.cpp; not called by the reference scripts,
 * the usual stage in front of a global registration).  Per point i: the neighbourhood with d^2 < salient_radius^2 (point i included, the test
 * strict, d^2 in float64 on the float32 coordinates: the rule of the other radius calls); fewer than min_neighbors members, or an all-zero
 * covariance, give saliency 0; otherwise l1 >= l2 >= l3 are the eigenvalues of the members' covariance (divided by their count, float64) and
 * the saliency is l3 when l2 / l1 < gamma_21 and l3 / l2 < gamma_32, else 0.  A point with saliency > 0 is a keypoint when its neighbourhood
 * at non_max_radius has at least min_neighbors members and none of them suppresses it.
 *   SUPPRESSION (a deliberate deviation): member j suppresses point i iff s_j > s_i + G with G = 1e-11 salient_radius^2; Open3D tests
 *   s_j > s_i.  Points with the same neighbourhood have the same saliency in exact arithmetic and Open3D keeps all of them on the exact tie;
 *   float64 sums taken in another order differ in the last bits (at most about 1e-12 salient_radius^2), and the strict test would then drop
 *   one of such a pair at random.  G is about 1e-7 of a typical l3.
 *   DEFAULT RADII: if salient_radius == 0 or non_max_radius == 0, BOTH are replaced (Open3D): resolution = the mean over all points of
 *   pcr_nearest_neighbor_distance (summed in float64 in a fixed order), salient_radius = 6 resolution, non_max_radius = 4 resolution.
 * Negative or non-finite radii, min_neighbors < 1, a non-finite gamma, a null cloud with n > 0: PCR_EINVAL.  n == 0: *out_n = 0.
 * Device, each optional: keep_mask (n bytes), out_xyz (capacity n x 3), out_index (capacity n int64, ascending: the layout of
 * pcr_remove_radius_outlier; Open3D's own order depends on its thread schedule), saliency (n float64, caller order), eigenvalues3 (n x 3 float64,
 * descending; zeros where the neighbourhood was too small).  Host: out_n, radii_used2 (optional: the salient and the non-max radius used).
 * Two runs give the same bits.                                                                                                          */
int pcr_iss_keypoints(pcr_context *ctx, const float *xyz, int64_t n, double salient_radius, double non_max_radius,
                      double gamma_21, double gamma_32, int min_neighbors,
                      uint8_t *keep_mask, float *out_xyz, int64_t *out_index, int64_t *out_n,
                      double *saliency, double *eigenvalues3, double *radii_used2);

/* == PointCloud.cluster_dbscan (Open3D PointCloud::ClusterDBSCAN, cpp/open3d/geometry/PointCloudCluster.cpp; not called by the reference scripts,
 * the usual stage between the outlier filters and a registration).  Open3D's sequential flood fill gives a result that the input alone
 * determines; these six rules restate it, and the labels are Open3D's row by row, not a renaming of them:
 *   1. NEIGHBOURHOOD: j is a neighbour of i iff d^2(i, j) < eps^2 -- strict, in float64 on the float32 coordinates, the point itself a member
 *      (the test of pcr_remove_radius_outlier and pcr_iss_keypoints).  d^2 = dx dx, += dy dy, += dz dz, every difference, square and sum
 *      rounded on its own (no fused multiply-add): a host recomputation in that order gives the same bits, so an exact tie d^2 == eps^2 is
 *      decided (not a neighbour).  eps^2 is the float64 product eps * eps.
 *   2. CORE: i is a core point iff its neighbourhood, itself included, has at least min_points members.
 *   3. CLUSTERS: the connected components of the graph on the core points whose edges are the core-core neighbour pairs.
 *   4. NUMBERING: clusters are numbered 0, 1, ... in ascending order of the smallest CALLER index among their core points (Open3D seeds a
 *      cluster at the first unvisited core point in index order; the smallest-index core point of a component cannot have been reached
 *      from an earlier seed).
 *   5. BORDER: a non-core point with at least one core neighbour gets the SMALLEST label among its core neighbours' clusters (Open3D's flood
 *      fills run in label order and relabel a point only from "unvisited" or "noise": the first cluster to reach the point keeps it).
 *   6. NOISE: every other point gets -1.
 * (sklearn.cluster.DBSCAN follows rules 2-6 with d <= eps.)
 * Device: xyz, labels (n int32, caller order), core_mask (optional, n bytes: 1 = core point).  Host: out_n_clusters (optional; without it the
 * call does not wait for the device).  n < 0 or over the int limit, a null xyz or labels with n > 0, eps not finite or <= 0,
 * min_points < 1: PCR_EINVAL with a message.  n == 0: PCR_OK and 0 clusters.  Two runs give the same labels.                      */
int pcr_cluster_dbscan(pcr_context *ctx, const float *xyz, int64_t n, double eps, int min_points,
                       int32_t *labels, uint8_t *core_mask, int64_t *out_n_clusters);

/* ---- registration ------------------------------------------------------------------ */
/* == registration_generalized_icp (ALL_FUNCTIONS.py:304-311; 2_MGICP...py:155-162).
 * correspondences optional device int32 [n_src x 2]; filled with n_correspondences rows.       */
int pcr_registration_generalized_icp(pcr_context *ctx, const float *src_xyz, const float *src_normals, int64_t n_src,
                                     const float *tgt_xyz, const float *tgt_normals, int64_t n_tgt,
                                     double max_correspondence_distance, const double *init_T,
                                     const pcr_gicp_params *params, pcr_result *result, int32_t *correspondences);

/* == registration_icp(..., TransformationEstimationForGeneralizedICP(loss), ...) on clouds that already carry
 *    covariances (GICP_robusto, ALL_FUNCTIONS.py:216-226): the given covariances are used untouched.
 *    cov6 = xx,xy,xz,yy,yz,zz per point, float32, device.                                                   */
int pcr_registration_generalized_icp_cov(pcr_context *ctx, const float *src_xyz, const float *src_cov6, int64_t n_src,
                                         const float *tgt_xyz, const float *tgt_cov6, int64_t n_tgt,
                                         double max_correspondence_distance, const double *init_T,
                                         const pcr_gicp_params *params, pcr_result *result, int32_t *correspondences);

/* == registration_icp(..., TransformationEstimationPointToPoint(with_scaling) / TransformationEstimationPointToPlane(kernel), criteria)
 *    (Open3D RegistrationICP; the reference itself only uses GICP).  The loop of pcr_registration_generalized_icp with the
 *    estimator's update: point-to-plane r = (T p - t).n over the target normals AS GIVEN (tgt_normals required, not normalised),
 *    weighted by the kernel, 6x6 LDLT; point-to-point Eigen::umeyama of the correspondences (a scaled pose when with_scaling).
 *    tgt_normals is optional for point-to-point, which does not read it.  correspondences optional device int32 [n_src x 2]. */
int pcr_registration_icp(pcr_context *ctx, const float *src_xyz, int64_t n_src, const float *tgt_xyz, const float *tgt_normals,
                         int64_t n_tgt, double max_correspondence_distance, const double *init_T,
                         const pcr_icp_params *params, pcr_result *result, int32_t *correspondences);

/* == registration_colored_icp(source, target, max_correspondence_distance, init, TransformationEstimationForColoredICP(lambda_geometric, kernel),
 *    criteria) (Park, Zhou, Koltun, ICCV 2017; Open3D ColoredICP.cpp).  Open3D is not at hand and the reference never calls it, so this statement
 *    is the specification.  The intensity of a point is I = (r + g + b) / 3, colours in [0, 1].
 *    Colour gradient of target point p with normal n (as given, not normalised) and intensity I_p (pcr_color_gradient; the registration uses the
 *    hybrid search radius = 2 * max_correspondence_distance, max_nn = 30): the search returns nn neighbours, the first is p itself; nn < 4: the
 *    gradient is 0.  Otherwise, for every other neighbour q_k, k = 1 .. nn-1: q'_k = q_k - ((q_k - p).n) n, row A_{k-1} = q'_k - p,
 *    b_{k-1} = I(q_k) - I_p; the last row is A_{nn-1} = (nn - 1) n with b = 0; the gradient d solves (A^T A) d = A^T b by LDLT.  The device keeps
 *    the 6 + 3 moments in float64, centred on p, summed in the list's order (float64 d^2, then caller index: the k-d tree's order).
 *    The loop is RegistrationICP's, as in pcr_registration_icp: search at init, then update / left-multiply / search, until |d fitness| <
 *    relative_fitness and |d RMSE| < relative_rmse, or max_iteration; fitness and inlier_rmse are the geometric ones of the search.
 *    Update: with lambda = lambda_geometric, s the transformed source point, t / n / d the target's point, normal and gradient and I_s, I_t the
 *    intensities, every correspondence gives two rows: r_G = sqrt(lambda) (s - t).n, J_G = sqrt(lambda) [s x n, n]; and, with
 *    s' = s - ((s - t).n) n and d_M = -d + (d.n) n, r_I = sqrt(1 - lambda) (I_s - (d.(s' - t) + I_t)), J_I = sqrt(1 - lambda) [s x d_M, d_M].  Each row is
 *    weighted by the kernel's weight of its own scaled residual (L2 / L1 / GM as for point-to-plane); both go into one 6x6 system, solved and
 *    turned into a pose exactly as the point-to-plane update (LDLT, Rz Ry Rx).  No correspondences: the update is the identity.
 *    src_colors, tgt_normals and tgt_colors are required (PCR_EINVAL names what is missing).  correspondences optional device int32 [n_src x 2]. */
int pcr_registration_colored_icp(pcr_context *ctx, const float *src_xyz, const float *src_colors, int64_t n_src, const float *tgt_xyz,
                                 const float *tgt_normals, const float *tgt_colors, int64_t n_tgt, double max_correspondence_distance,
                                 const double *init_T, const pcr_colored_icp_params *params, pcr_result *result, int32_t *correspondences);
/* the colour gradients of a cloud alone (the statement above) over the neighbours of search_kind / knn / radius (PCR_SEARCH_KNN or
 * PCR_SEARCH_HYBRID, knn in 1..32): gradient3 = n x 3 float32 (device), caller order.  Asynchronous on the context's stream. */
int pcr_color_gradient(pcr_context *ctx, const float *xyz, const float *normals, const float *colors, int64_t n, int search_kind, int knn,
                       double radius, float *gradient3);

/* ============================================================================================ voxelized GICP on a voxel covariance map
 * Voxelized GICP (Koide, Yokozuka, Oishi, Banno, ICRA 2021; fast_gicp's FastVGICP): the target becomes a grid of cells, each with a count, a mean
 * and a mean covariance, and a source point is matched to the cell it falls into (or to that cell and its neighbours) by a few hash probes
 * instead of a nearest-neighbour search.  The map is built once and serves any number of registrations (scan to map).  Open3D has no such call
 * and the reference never makes one, so this statement is the specification.
 *
 * MAP.  Input: n target points (float32) and one covariance per point (float32 cov6 = xx,xy,xz,yy,yz,zz) -- or normals, from which the member
 *   covariance is the one the GICP estimator uses, R diag(epsilon, 1, 1) R^T with R the rotation taking e1 onto the normal (identity when
 *   n.x < -0.99; the normal is not normalised), computed in float64 from the float32 normal and rounded to float32 before it is summed.
 *   The grid is pcr_voxel_down_sample's: in float64 on the float32 values, origin = min - voxel_size / 2 per axis,
 *   index = floor((p - origin) / voxel_size); indices must fit 21 bits (otherwise PCR_EINVAL, as pcr_voxel_down_sample).
 *   Per occupied cell v: the count N_v; the mean mu_v = (float64 sum of the members in input order) / N_v, rounded to float32; the covariance
 *   C_v = per channel (float64 sum of the members' cov6 in input order) / N_v, rounded to float32.  The rows are listed in Morton order of the
 *   cell index (bit b of ix, iy, iz at bits 3b, 3b + 1, 3b + 2): the order in which pcr_voxel_down_sample lists them.
 * ROWS AT A POSE T (float64 4x4, row-major).  For source point a = (x, y, z): q_r = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3 in float64, every
 *   operation rounded once, no fused multiply-add (numpy's elementwise expression gives the same bits); cell = floor((q - origin) / voxel_size);
 *   the candidate cells are cell + offset for the neighbourhood: 1: (0,0,0); 7: (0,0,0), (+1,0,0), (-1,0,0), (0,+1,0), (0,-1,0), (0,0,+1), (0,0,-1)
 *   in that order; 27: all (dx,dy,dz) in {-1,0,1}^3 in lexicographic order, dx slowest.  A candidate with an index outside [0, 2^21) on any
 *   axis, unoccupied, or with N_v < min_points_per_voxel gives no row.  The rows (i, v) are ordered by i, then by offset order; v is the map row.
 * UPDATE.  Row (i, v) contributes N_v times what the GICP estimator contributes for a correspondence with source point q_i, source covariance
 *   R C_i R^T, target point mu_v and target covariance C_v: W = (C_v + R C_i R^T)^(-1/2), three whitened rows r = W (q_i - mu_v),
 *   J = W [-skew(q_i) | I], each weighted by the kernel's weight of its own r (L2 / L1 / GM as in pcr_registration_generalized_icp) and then by
 *   N_v.  The 6x6 system is solved and turned into a pose exactly as the GICP update (LDLT, Rz Ry Rx, left-multiplied).  No rows: the identity.
 * LOOP.  RegistrationICP's, as in pcr_registration_icp: rows at init, then update / left-multiply / rows, until |d fitness| < relative_fitness
 *   and |d RMSE| < relative_rmse, or max_iteration.  fitness = (source points with at least one row) / n_src,
 *   inlier_rmse = sqrt(sum over the rows of |q_i - mu_v|^2 / rows), n_correspondences = the number of rows.  There is no
 *   max_correspondence_distance: the voxel size plays its part.
 *
 * A map that grows (pcr_voxel_map_create_on_grid / _insert / _merge / _remove_far).  Open3D has no such calls either; this is their specification.
 * GRID.  A map has a voxel size and a grid_min g (three float64); its origin is g - voxel_size / 2 per axis in float64, the expression of MAP with g
 *   standing in for the cloud's minimum.  A map made by pcr_voxel_map_create has g = the target's minimum.  Two maps are on the same grid iff
 *   their voxel sizes and their origins are equal bit for bit.
 * MAP ON A GIVEN GRID, AT A POSE.  Input: n >= 1 points with cov6 or normals (exactly one, as for MAP), a grid, and an optional pose T (float64
 *   4x4, row-major; none is the identity).  Member point: p' = float32(q) with q the float64 expression of ROWS,
 *   ((T_r0 x + T_r1 y) + T_r2 z) + T_r3, every operation rounded once, no fused multiply-add.  Member covariance: first formed as MAP forms it (the
 *   cov6 as given, or R diag(epsilon, 1, 1) R^T from the normal, in float32), then rotated: C' = float32((R C) R^T) with R the upper 3x3 of T in
 *   float64, both products entry by entry as (a0 b0 + a1 b1) + a2 b2 without contraction.  With T the identity p' and C' are the inputs bit for
 *   bit (but for the sign of a zero: -0 comes out as +0), so there is no special case.  The cells, counts, means and covariances are those of MAP over (p', C') on the given grid, rows in Morton order.  A member whose cell
 *   index lies outside [0, 2^21) on any axis -- below the origin counts too -- is PCR_EINVAL: xyz lies outside the map's grid; nothing is changed.
 * MERGE(A, B).  A and B are on the same grid (otherwise PCR_EINVAL).  One row per cell occupied in A or in B, in Morton order.  A cell in only one
 *   of them keeps that row bit for bit.  A cell in both gets N = N_a + N_b (a sum above 2^31 - 1 is PCR_EINVAL) and, for each of its nine channels
 *   (3 mean, 6 covariance), float32((float64(N_a) float64(a) + float64(N_b) float64(b)) / float64(N)): the sum, then the division, then one
 *   rounding to float32.  The two products are exact for counts below 2^29 (a 24-bit significand times an integer under 2^29 fits the 53 bits of
 *   a float64), so a fused multiply-add cannot change the result there.  MERGE is commutative bit for bit; it is not associative.
 * INSERT(map, cloud, T) = MERGE(map, the map of the cloud at T on the map's grid).
 * REMOVE_FAR(map, center c (float64 x3), max_distance r).  A row is kept iff d^2 < r^2 (strict), with d^2 in float64 from the float32 mean:
 *   differences, squares and sums in the order x, y, z, each rounded once, and r^2 = r r.  Kept rows keep their bits and their relative order.
 * A map never has zero rows: an operation that would leave none is PCR_EINVAL (would leave the map empty) and changes nothing.
 * All cloud, covariance and row buffers are DEVICE buffers.  The map lives in one device allocation of its own until it is destroyed, and any
 * context on the same device may use it for any number of calls.  _insert, _merge and _remove_far change it, all or nothing and finished when they
 * return: the new block is built, swapped in, and the old one freed (which waits for the device); on any error the map is exactly as before.
 * While such a call runs no other call may use the map, and map rows in an earlier correspondence set are stale afterwards (row indices change). */
typedef struct pcr_voxel_map pcr_voxel_map;
typedef struct {
    int32_t loss;             /* the fields of pcr_gicp_params ...            */
    double loss_k;
    double epsilon;           /* source covariances from normals (src_cov6 == NULL) */
    double relative_fitness;
    double relative_rmse;
    int32_t max_iteration;
    int32_t neighborhood;     /* ... plus: 1, 7 or 27 candidate cells per source point */
    int32_t min_points_per_voxel;   /* >= 1: cells with fewer members give no row */
} pcr_vgicp_params;

/* Exactly one of cov6 / normals must be given (n x 6 / n x 3 float32); n >= 1.  voxel_size <= 0, a non-finite voxel_size or epsilon, a non-finite
 * value in xyz / cov6 / normals, both or neither of cov6 / normals: PCR_EINVAL with a message naming the argument.  Finished when it returns. */
int pcr_voxel_map_create(pcr_context *ctx, const float *xyz, const float *cov6, const float *normals, int64_t n, double voxel_size, double epsilon,
                         pcr_voxel_map **out);
/* Frees the map (waits for the device, so no call is still reading it).  NULL is allowed. */
int pcr_voxel_map_destroy(pcr_voxel_map *map);
/* number of occupied cells = map rows */
int pcr_voxel_map_size(const pcr_voxel_map *map, int64_t *cells);
/* the map's rows in Morton order, each output optional: cell3 (cells x 3 int32: ix, iy, iz), count (cells int32), mean3 (cells x 3 float32),
 * cov6 (cells x 6 float32).  Asynchronous on the context's stream. */
int pcr_voxel_map_read(pcr_context *ctx, const pcr_voxel_map *map, int32_t *cell3, int32_t *count, float *mean3, float *cov6);
/* the rows (i, v) of the rule at the pose T: rows2 = int32 pairs, capacity n_src x neighborhood rows; *n_rows on the host. */
int pcr_voxel_map_correspondences(pcr_context *ctx, const pcr_voxel_map *map, const float *src_xyz, int64_t n_src, const double *T, int neighborhood,
                                  int min_points_per_voxel, int32_t *rows2, int64_t *n_rows);
/* the loop of the rule from init_T.  Exactly as for the map, the source carries src_cov6 or, without it, src_normals (covariances by
 * params->epsilon); neither is PCR_EINVAL naming src_cov6.  A neighborhood that is not 1, 7 or 27, min_points_per_voxel < 1, a non-finite
 * value in src_xyz / src_cov6 / src_normals / init_T: PCR_EINVAL with a message naming the argument.  correspondences: optional device int32,
 * capacity n_src x neighborhood rows: the rows at the returned pose (n_correspondences of them). */
int pcr_registration_voxelized_gicp(pcr_context *ctx, const float *src_xyz, const float *src_cov6, const float *src_normals, int64_t n_src,
                                    const pcr_voxel_map *map, const double *init_T, const pcr_vgicp_params *params, pcr_result *result,
                                    int32_t *correspondences);
/* The map of a cloud on the grid (grid_min3, voxel_size) at the pose T (MAP ON A GIVEN GRID; T optional: NULL is the identity).  The arguments of
 * pcr_voxel_map_create and their refusals, plus: a non-finite value in grid_min3 or T (named), a member outside the grid (xyz lies outside the
 * map's grid).  Finished when it returns. */
int pcr_voxel_map_create_on_grid(pcr_context *ctx, const float *xyz, const float *cov6, const float *normals, int64_t n, double voxel_size, double epsilon,
                                 const double *grid_min3, const double *T, pcr_voxel_map **out);
/* map <- INSERT(map, cloud, T); T optional.  A NULL map, a map on another device than the context, the cloud refusals of the call above. */
int pcr_voxel_map_insert(pcr_context *ctx, pcr_voxel_map *map, const float *xyz, const float *cov6, const float *normals, int64_t n, double epsilon,
                         const double *T);
/* map <- MERGE(map, other); other is unchanged.  other == map, a NULL map, maps on another device or on different grids: PCR_EINVAL. */
int pcr_voxel_map_merge(pcr_context *ctx, pcr_voxel_map *map, const pcr_voxel_map *other);
/* map <- REMOVE_FAR(map, center3, max_distance); *removed (optional, host) = rows dropped.  A non-finite center3, a max_distance that is not
 * finite or <= 0: PCR_EINVAL naming the argument. */
int pcr_voxel_map_remove_far(pcr_context *ctx, pcr_voxel_map *map, const double *center3, double max_distance, int64_t *removed);
/* the grid of a map, each output optional (host): grid_min3, origin3 = grid_min3 - voxel_size / 2, voxel_size */
int pcr_voxel_map_grid(const pcr_voxel_map *map, double *grid_min3, double *origin3, double *voxel_size);

/* ============================================================================================ NDT on a normal-distributions voxel map
 * The Normal Distributions Transform (Biber & Strasser, IROS 2003; Magnusson, 2009; PCL's NormalDistributionsTransform, ndt_omp): the target
 * becomes a grid of cells, each with the mean and the SAMPLE covariance of its member positions, and a source point is scored against the normal
 * distribution of the cell it falls into (or of that cell and its neighbours).  Nothing is needed per point, neither normals nor covariances, and
 * there is no nearest-neighbour search.  Open3D has no such call and the reference never makes one, so this statement is the specification.
 *
 * MAP.  Input: n >= 1 target points (float32), voxel_size, min_points_per_voxel >= 2 (PCL's default: 6) and eigenvalue_ratio in (0, 1] (PCL's
 *   min_covar_eigvalue_mult, default 0.01).  The grid, the cells, the counts N_v, the means mu_v (float32) and the Morton row order are exactly MAP
 *   of the voxelized GICP section above.  The member statistic of point i in cell v: d = float64(p_i) - float64(mu_v); its six products
 *   d_x d_x, d_x d_y, d_x d_z, d_y d_y, d_y d_z, d_z d_z are each rounded once to float64 and then to float32.  C_v = per channel (float64 sum of the
 *   members' values in input order) / N_v, rounded to float32: the ordered-sum rule that section applies to a member cov6.
 *   A cell is VALID iff N_v >= min_points_per_voxel and the largest eigenvalue lambda_max of S_v = C_v N_v / (N_v - 1) (float64) is > 0.
 *   The information matrix of a valid cell is A_v = V diag(1 / max(lambda_k, eigenvalue_ratio lambda_max)) V^T, in float64 from the symmetric
 *   eigendecomposition S_v = V diag(lambda) V^T, computed once at map creation and kept in float64 (six numbers per cell: xx,xy,xz,yy,yz,zz).
 *   An invalid cell keeps its row (count, mean, C_v) and has A_v = 0.
 * ROWS AT A POSE T.  Exactly ROWS of the voxelized GICP section with "valid" in place of "N_v >= min_points_per_voxel": the same expression for
 *   q, the same candidate offsets for the neighbourhoods 1, 7 and 27, the same order (by i, then by offset order).
 * SCORE CONSTANTS (Magnusson's and PCL's), from outlier_ratio p (default 0.55) and r = voxel_size, in float64 on the host:
 *   c1 = 10 (1 - p), c2 = p / r^3, d3 = -log c2, d1 = -log(c1 + c2) - d3, d2 = -2 log((-log(c1 e^(-1/2) + c2) - d3) / d1).
 * UPDATE.  Row (i, v): delta = q_i - float64(mu_v), m = delta^T A_v delta, e = exp(-d2 m / 2), w = -d1 d2 e (> 0), J = [-skew(q_i) | I].  The row
 *   adds w J^T A_v J to the 6x6 matrix and w J^T A_v delta to the right-hand side (the sign convention of the GICP update) and -d1 e to the score.
 *   Rows are NOT weighted by N_v.  The system is solved and turned into a pose exactly as the GICP update (LDLT, Rz Ry Rx, left-multiplied).
 *   No rows: the identity.  This is the Gauss-Newton (IRLS) form of the NDT objective: the exact gradient of the score, and its Hessian without the
 *   negative term and without the second-derivative terms, so the matrix is positive semi-definite.  PCL's Newton step with the More-Thuente line
 *   search is NOT what runs.
 * LOOP.  RegistrationICP's, as in the voxelized GICP section: rows at init, then update / left-multiply / rows, until |d fitness| <
 *   relative_fitness and |d RMSE| < relative_rmse, or max_iteration.  fitness = (source points with at least one row) / n_src,
 *   inlier_rmse = sqrt(sum over the rows of |q_i - mu_v|^2 / rows), n_correspondences = the number of rows.  The loop does not use the score.
 * All cloud and row buffers are DEVICE buffers.  The map lives in one device allocation of its own until it is destroyed and changes only through
 * the calls of "A normal-distributions map that grows" below; any context on the same device may use it for any number of calls. */
typedef struct pcr_ndt_map pcr_ndt_map;
typedef struct {
    double relative_fitness;
    double relative_rmse;
    int32_t max_iteration;
    int32_t neighborhood;     /* 1, 7 or 27 candidate cells per source point */
    double outlier_ratio;     /* p of the score constants, in (0, 1) */
} pcr_ndt_params;

/* n >= 1.  A non-finite value in xyz, voxel_size <= 0 (or not finite), min_points_per_voxel < 2, eigenvalue_ratio outside (0, 1], cell indices
 * that do not fit 21 bits: PCR_EINVAL with a message naming the argument.  Finished when it returns. */
int pcr_ndt_map_create(pcr_context *ctx, const float *xyz, int64_t n, double voxel_size, int min_points_per_voxel, double eigenvalue_ratio,
                       pcr_ndt_map **out);
/* Frees the map (waits for the device, so no call is still reading it).  NULL is allowed. */
int pcr_ndt_map_destroy(pcr_ndt_map *map);
/* number of occupied cells = map rows (valid or not) */
int pcr_ndt_map_size(const pcr_ndt_map *map, int64_t *cells);
/* the map's rows in Morton order, each output optional (device): cell3 (cells x 3 int32), count (cells int32), mean3 (cells x 3 float32),
 * cov6 (cells x 6 float32: C_v), info6 (cells x 6 float64: A_v), valid (cells uint8).  Asynchronous on the context's stream. */
int pcr_ndt_map_read(pcr_context *ctx, const pcr_ndt_map *map, int32_t *cell3, int32_t *count, float *mean3, float *cov6, double *info6,
                     uint8_t *valid);
/* the grid of a map, each output optional (host): origin3 = grid_min - voxel_size / 2 (grid_min: the target's minimum, or what
 * pcr_ndt_map_create_on_grid was given; pcr_ndt_map_rule reads it), voxel_size */
int pcr_ndt_map_grid(const pcr_ndt_map *map, double *origin3, double *voxel_size);
/* the rows (i, v) of the rule at the pose T: rows2 = int32 pairs, capacity n_src x neighborhood rows; *n_rows on the host.  A neighborhood that is
 * not 1, 7 or 27, a non-finite value in src_xyz / T, a map on another device than the context: PCR_EINVAL naming the argument. */
int pcr_ndt_map_correspondences(pcr_context *ctx, const pcr_ndt_map *map, const float *src_xyz, int64_t n_src, const double *T, int neighborhood,
                                int32_t *rows2, int64_t *n_rows);
/* UPDATE's sums at the pose T in ONE kernel launch, all outputs on the host and each optional: JTJ (36, the full symmetric matrix), JTr (6),
 * *score, *rows, *points_with_rows, *sum_d2 (sum over the rows of |q_i - mu_v|^2).  The sums are taken in a fixed order: the same bits on every
 * run.  outlier_ratio outside (0, 1) and the refusals of pcr_ndt_map_correspondences: PCR_EINVAL naming the argument. */
int pcr_ndt_linearize(pcr_context *ctx, const pcr_ndt_map *map, const float *src_xyz, int64_t n_src, const double *T, int neighborhood,
                      double outlier_ratio, double *JTJ, double *JTr, double *score, int64_t *rows, int64_t *points_with_rows, double *sum_d2);
/* the loop of the rule from init_T.  max_iteration < 0, outlier_ratio outside (0, 1), a neighborhood that is not 1, 7 or 27, a non-finite value
 * in src_xyz / init_T, a map on another device: PCR_EINVAL naming the argument.  A map without a valid cell is no error: no rows, the pose stays
 * init_T, fitness 0.  correspondences: optional device int32, capacity n_src x neighborhood rows: the rows at the returned pose. */
int pcr_registration_ndt(pcr_context *ctx, const float *src_xyz, int64_t n_src, const pcr_ndt_map *map, const double *init_T,
                         const pcr_ndt_params *params, pcr_result *result, int32_t *correspondences);

/* A normal-distributions map that grows (pcr_ndt_map_create_on_grid / _insert / _merge / _remove_far).  PCL and ndt_omp rebuild their target
 * grid; this is the specification of these calls.  All arithmetic is float64 on float32 inputs, every operation rounded once, no fused
 * multiply-add.
 * RULE OF A MAP.  A map carries voxel_size, grid_min g (three float64; its origin is g - voxel_size / 2 per axis in float64, the GRID rule of the
 *   voxel covariance map), min_points_per_voxel and eigenvalue_ratio.  A map made by pcr_ndt_map_create has g = the target's minimum.  Two maps are
 *   compatible iff all four are equal bit for bit.  In every row of every map, validity and A_v are a pure function of
 *   (N_v, C_v, min_points_per_voxel, eigenvalue_ratio): the one MAP states.
 * MAP ON A GIVEN GRID, AT A POSE.  Input: n >= 1 points, a rule, and an optional pose T (float64 4x4, row-major; none is the identity, applied all
 *   the same).  Member point: p' = float32(q) with q the float64 expression of ROWS, ((T_r0 x + T_r1 y) + T_r2 z) + T_r3.  The result is exactly
 *   MAP of this section over p' on the given grid: counts, float32 means, C_v, validity, A_v, Morton order.  A member whose cell index lies outside
 *   [0, 2^21) on any axis -- below the origin counts too -- is PCR_EINVAL: xyz lies outside the map's grid; nothing is changed.  With the cloud's
 *   own minimum as grid_min and no pose the result is that of pcr_ndt_map_create row for row and bit for bit.
 * MERGE(A, B).  A and B are compatible (otherwise PCR_EINVAL).  One row per cell occupied in A or in B, in Morton order.  A cell in only one of them
 *   keeps that row bit for bit: count, mean, C_v, A_v, validity.  A cell in both gets N = N_a + N_b (a sum above 2^31 - 1 is PCR_EINVAL and nothing
 *   is changed) and, per channel of the mean, mu = float32((float64(N_a) a + float64(N_b) b) / float64(N)): the two products, the sum, the
 *   division, one rounding to float32 -- the mean rule of the voxel covariance map's MERGE.  The covariances are taken about two different means, so
 *   they are moved to the new one by the parallel-axis term: with d_a = float64(mu_a) - float64(mu), d_b likewise and mu the NEW float32 mean,
 *   each channel rc of xx, xy, xz, yy, yz, zz is M_a = float64(C_a[rc]) + d_a[r] d_a[c] (the product rounded first, then the sum), M_b likewise,
 *   and C[rc] = float32((float64(N_a) M_a + float64(N_b) M_b) / float64(N)).  Validity and A_v of the merged cell are those of MAP from (N, C):
 *   A_v is recomputed, never averaged.  MERGE is commutative bit for bit (only sums and products swap their operands); it is not associative.
 * INSERT(map, cloud, T) = MERGE(map, the map of the cloud at T on the map's grid with the map's rule).
 * REMOVE_FAR(map, center c (float64 x3), max_distance r).  The voxel covariance map's rule on the float32 means: a row is kept iff d^2 < r^2
 *   (strict), d^2 in float64 by differences, squares and sums in the order x, y, z, and r^2 = r r.  Kept rows keep all their bits, A_v included,
 *   and their relative order.  A map never has zero rows: an operation that would leave none is PCR_EINVAL (would leave the map empty).
 * _insert, _merge and _remove_far change the map, all or nothing and finished when they return: the new block with its cell hash is built, swapped
 * in, and the old one freed (which waits for the device); on any error the map is exactly as before.  While such a call runs no other call may
 * use the map, and map rows in an earlier correspondence set are stale afterwards (row indices change). */
/* The map of a cloud on the grid (grid_min3, voxel_size) at the pose T (MAP ON A GIVEN GRID; T optional: NULL is the identity).  The arguments of
 * pcr_ndt_map_create and their refusals, plus: a non-finite value in grid_min3 or T (named), a member outside the grid (xyz lies outside the
 * map's grid).  Finished when it returns. */
int pcr_ndt_map_create_on_grid(pcr_context *ctx, const float *xyz, int64_t n, double voxel_size, int min_points_per_voxel, double eigenvalue_ratio,
                               const double *grid_min3, const double *T, pcr_ndt_map **out);
/* map <- INSERT(map, cloud, T); T optional.  A NULL map, a map on another device than the context, the cloud refusals of the call above. */
int pcr_ndt_map_insert(pcr_context *ctx, pcr_ndt_map *map, const float *xyz, int64_t n, const double *T);
/* map <- MERGE(map, other); other is unchanged.  other == map (itself), a NULL map, maps on another device, on different grids (not on the map's
 * grid) or with another min_points_per_voxel / eigenvalue_ratio (does not follow the map's rule): PCR_EINVAL. */
int pcr_ndt_map_merge(pcr_context *ctx, pcr_ndt_map *map, const pcr_ndt_map *other);
/* map <- REMOVE_FAR(map, center3, max_distance); *removed (optional, host) = rows dropped.  A non-finite center3, a max_distance that is not
 * finite or <= 0: PCR_EINVAL naming the argument. */
int pcr_ndt_map_remove_far(pcr_context *ctx, pcr_ndt_map *map, const double *center3, double max_distance, int64_t *removed);
/* the rule of a map, each output optional (host): grid_min3 (origin3 of pcr_ndt_map_grid = grid_min3 - voxel_size / 2), min_points_per_voxel,
 * eigenvalue_ratio */
int pcr_ndt_map_rule(const pcr_ndt_map *map, double *grid_min3, int *min_points_per_voxel, double *eigenvalue_ratio);

/* == the whole body of Multiscale_GICP (ALL_FUNCTIONS.py:286-312 / 2_MGICP...py:140-163), device resident:
 * per scale voxel_down_sample -> remove_statistical_outlier(sor_k, sor_std) -> estimate_normals(KNN normal_k)
 * -> registration_generalized_icp, chained.  src/tgt_normals optional (AF flow orientation prior).
 * records: n_scales entries (host). correspondences: optional device int32 [n_src x 2] of the last scale. */
int pcr_multiscale_gicp(pcr_context *ctx, const float *src_xyz, const float *src_normals, int64_t n_src,
                        const float *tgt_xyz, const float *tgt_normals, int64_t n_tgt, const double *voxel_sizes,
                        const double *max_distances, int n_scales, int sor_k, double sor_std, int normal_k,
                        const double *init_T, const pcr_gicp_params *params, pcr_scale_record *records,
                        int32_t *correspondences);

/* == the per-pair loops of the reference (1_FGR...py:134-147 is the FGR one; 2_MGICP...py:187-214 and
 *    ALL_FUNCTIONS.py:349-392 the GICP ones): MANY independent pairs in one call.  The library keeps `inflight` pairs in
 *    flight on `device` (one worker thread + context + stream each, taken from a process-wide pool), pair i runs exactly
 *    pcr_multiscale_gicp on pairs[i] with the shared scale tables, and the call returns when all pairs are done.
 *    `after_stream` is the HIP stream whose already-enqueued work produces the input clouds (NULL = the legacy default
 *    stream); the workers always wait for it.  Per-pair status and error text come back in the descriptor; the return value is PCR_OK iff every pair is. */
typedef struct {
    const float *src_xyz, *src_normals; int64_t n_src;      /* device; normals optional */
    const float *tgt_xyz, *tgt_normals; int64_t n_tgt;
    double init_T[16];
    pcr_scale_record *records;                              /* host, n_scales entries */
    int32_t *correspondences;                               /* optional device int32 [n_src x 2] of the last scale */
    int32_t status;                                         /* out */
    char error[120];                                        /* out */
} pcr_pair;
int pcr_register_pairs(int device, pcr_pair *pairs, int n_pairs, const double *voxel_sizes, const double *max_distances,
                       int n_scales, int sor_k, double sor_std, int normal_k, const pcr_gicp_params *params, int inflight,
                       void *after_stream);

/* == registro_FGR as ONE call (ALL_FUNCTIONS.py:178-203 / 1_FGR...py:41-66): estimate_normals(Hybrid(normal_radius, normal_max_nn))
 *    on both clouds -> compute_fpfh_feature(Hybrid(feature_radius, feature_max_nn)) on both -> FGR with `option` ->
 *    evaluate_registration.  Each cloud is Morton-sorted and indexed ONCE for all four uses.  The reference's side effect (both
 *    inputs gain normals) is returned through src/tgt_normals_out (optional, device, caller order); src/tgt_prior are the
 *    normals the clouds already carry, if any (Open3D flips the new normal to agree with them).                                */
typedef struct {
    double normal_radius;  int32_t normal_max_nn;      /* 2 * voxel_size, 20    (ALL_FUNCTIONS.py:181) */
    double feature_radius; int32_t feature_max_nn;     /* 10 * voxel_size, 200  (ALL_FUNCTIONS.py:185) */
    pcr_fgr_option option;                             /* ALL_FUNCTIONS.py:189-196 */
} pcr_fgr_params;
int pcr_registro_fgr(pcr_context *ctx, const float *src_xyz, const float *src_prior, int64_t n_src, const float *tgt_xyz,
                     const float *tgt_prior, int64_t n_tgt, const pcr_fgr_params *params, float *src_normals_out,
                     float *tgt_normals_out, pcr_result *result, int32_t *correspondences);

/* == the reference's per-pair loops with a choice of what runs per pair:
 *    PCR_STAGE_FGR       script 1 (1_FGR...py:134-147):                 registro_FGR                      -> pairs[i].fgr
 *    PCR_STAGE_GICP      script 2 (2_MGICP...py:187-214):               Multiscale_GICP from init_T       -> pairs[i].records
 *    PCR_STAGE_FGR_GICP  Coarse_to_fine_FGR_M_GICP (ALL_FUNCTIONS.py:317-332, full_registration :349-392): registro_FGR, then
 *                        Multiscale_GICP from its pose (init_T ignored)                                   -> both
 *    radius_rule 0: max_distances as given (script 2 table); 1: ALL_FUNCTIONS.py:277-278, radius_from_cloud_pair(source, target)
 *    * 2^-scale computed per pair from the two AABBs (max_distances ignored).  gicp_prior_from_fgr: the normals registro_FGR
 *    left on the clouds are the orientation prior of every scale (the ALL_FUNCTIONS flow; the scripts reload the clouds).
 *    info_max_dist > 0: pairs[i].info36 <- get_information_matrix_from_point_clouds(source, target, info_max_dist, final pose)
 *    (ALL_FUNCTIONS.py:327-331).  The library keeps `inflight` pairs (or groups, see `group`) in flight exactly as pcr_register_pairs does. */
typedef enum { PCR_STAGE_GICP = 1, PCR_STAGE_FGR = 2, PCR_STAGE_FGR_GICP = 3 } pcr_stage;
typedef struct {
    int32_t stage;
    const pcr_fgr_params *fgr;                          /* stages with FGR; option.seed + pair index seeds pair i */
    const double *voxel_sizes, *max_distances; int32_t n_scales;
    int32_t radius_rule;
    int32_t sor_k; double sor_std; int32_t normal_k;
    const pcr_gicp_params *gicp;
    int32_t gicp_prior_from_fgr;
    double info_max_dist;
    int32_t inflight;
    int32_t group;                                      /* > 1 (stages GICP and FGR + GICP, whose FGR part stays pair by pair): `group` consecutive pairs run in LOCKSTEP through the same
                                                           launches (blockIdx.y = pair: preprocessing batched over clouds and scales, one GICP loop per
                                                           scale for the whole group); `inflight` then counts groups.  Same per-pair arithmetic as the
                                                           pair-by-pair path; at most 24 (larger values are clamped).  Every unit of such a plan -- a ragged last group of ONE pair too --
                                                           runs the GROUP forms of the kernels (one-query-per-lane k-NN, 1024-point iteration tiles),
                                                           so a pair's bits do not depend on how the batch was cut */
    int32_t pair_forms;                                 /* != 0: the kernel forms are chosen by the PAIR alone (group forms iff both clouds hold fewer than
                                                           400 000 points; larger pairs run one by one with the single-pair forms) whatever `group` is:
                                                           a pair's pose bits are then the same in every batch, group size and shard (gathered
                                                           multi-GPU poses = the single-GPU run).  What registration.register_pairs_plan(group=None) sets. */
    int32_t fgr_group;                                  /* > 1 (stages with FGR): that many consecutive pairs go through registro_FGR in LOCKSTEP -- imports, sorts,
                                                           trees, hybrid normals, FPFH lists and histograms, the mutual feature search, cross check, tuple
                                                           test, GNC optimiser and evaluation of all of them in the same launches, six host waits per
                                                           GROUP instead of eight per pair (1_FGR...py:134-147 is ~125 small dependent launches per NCLT-size
                                                           pair).  Same bits per pair as pair by pair.  Pairs the group form does not take (from ~70k points:
                                                           the tile-pruned feature search) run one by one.  Stage FGR: `inflight` counts these groups. */
} pcr_pairs_plan;
typedef struct {
    pcr_pair base;                                      /* inputs, records (stages with GICP), correspondences of the LAST stage run, status */
    pcr_result fgr;                                     /* out, stages with FGR */
    float *src_normals_out, *tgt_normals_out;           /* optional device buffers (n x 3): the normals registro_FGR leaves on the clouds */
    double max_distances[8];                            /* out: the per-scale search radii actually used (radius_rule 1) */
    double info36[36];                                  /* out when info_max_dist > 0 */
} pcr_pair_ex;
int pcr_register_pairs_plan(int device, pcr_pair_ex *pairs, int n_pairs, const pcr_pairs_plan *plan, void *after_stream);

/* measurement hook for the worker contexts pcr_register_pairs keeps in its pool (all idle between calls): enable >= 0 switches
 * their instrumentation on/off, out16 (optional) receives the SUM of their pcr_profile_read counters, reset clears them. */
int pcr_pool_profile(int device, int enable, double *out16, int reset);

/* == evaluate_registration (ALL_FUNCTIONS.py:809-820) */
int pcr_evaluate_registration(pcr_context *ctx, const float *src_xyz, int64_t n_src, const float *tgt_xyz,
                              int64_t n_tgt, double max_correspondence_distance, const double *T, pcr_result *result,
                              int32_t *correspondences);

/* == get_information_matrix_from_point_clouds (ALL_FUNCTIONS.py:327-331); info36 host */
int pcr_information_matrix(pcr_context *ctx, const float *src_xyz, int64_t n_src, const float *tgt_xyz, int64_t n_tgt,
                           double max_correspondence_distance, const double *T, double *info36);

/* == compute_fpfh_feature (ALL_FUNCTIONS.py:186-187); feat33: n x 33 float32 (device)
 * Normals are used AS GIVEN, not normalised (Open3D does not normalise them either): with a normal longer than 1 a pair's
 * |n . dp| / |dp| can exceed 1, acos of it is NaN and the pair keeps the frame of its first point, as in Open3D.
 * Coincident points: a pair at distance 0 votes in the bins of f = 0 (bin 5 of each histogram) and has no weight in the sum.
 * A point with more than k coincident copies (KNN(k), or Hybrid(r, k)) lists k of them, itself among them or not; either way
 * all its pairs are at distance 0 and its row is 100 in bins 5, 16 and 27, which is also Open3D's row (k >= 2; k = 1 lists
 * nothing: a zero row).  tests/test_gpu_fpfh_rows.py */
int pcr_compute_fpfh_feature(pcr_context *ctx, const float *xyz, const float *normals, int64_t n, int search_kind,
                             int knn, double radius, float *feat33);

/* == registration_fgr_based_on_feature_matching (ALL_FUNCTIONS.py:198-202) */
int pcr_registration_fgr(pcr_context *ctx, const float *src_xyz, const float *src_feat33, int64_t n_src,
                         const float *tgt_xyz, const float *tgt_feat33, int64_t n_tgt, const pcr_fgr_option *option,
                         pcr_result *result, int32_t *correspondences);

/* == registration_ransac_based_on_correspondence / registration_ransac_based_on_feature_matching (Open3D 0.13 and later; the reference calls
 *    neither, so the algorithm is stated here).  ONE sequential, deterministic loop defines the answer; the device may run it in any order.
 *    Hypothesis i = 0, 1, ...: rows r_k = splitmix64(seed + ransac_n * i + k) % n_corres, k < ransac_n (the sampler of the FGR tuple test; repeats
 *    allowed).  CorrespondenceCheckerBasedOnEdgeLength(thr): over every pair a < b of the sample, ls = |s_a - s_b|, lt = |t_a - t_b|, fails if
 *    ls < lt * thr or lt < ls * thr.  T_i = Eigen::umeyama of the sampled pairs (with_scaling: a scaled pose).  CorrespondenceCheckerBasedOnDistance(thr)
 *    fails if a sampled pair has |T s - t| > thr; CorrespondenceCheckerBasedOnNormal(thr) fails if one has (T[:3,:3] n_s) . n_t < cos(thr), and
 *    passes when either cloud has no normals.  A hypothesis that fails a checker or has a non-finite T is invalid (it still uses up its iteration).
 *    A valid one is scored in float64 over all rows: inliers dis = |T s - t| < max_distance, count_i, err2_i = sum dis^2 (fixed order: same bits
 *    on every run).  i is better than the running best if count_i is larger, or equal with sqrt(err2_i / count_i) strictly smaller; count 0 is never
 *    better than the empty start; on a full tie the earlier iteration stays.  est_k = max_iteration at the start, iteration i runs iff i < est_k; when
 *    i becomes the best, k' = log(1 - confidence) / log(1 - (count_i / n_corres)^ransac_n) (the denominator evaluated as log1p(-rho^n), so that a tiny rho^n gives a
 *    huge k' and not a division by zero), and if k' is finite and 0 <= k' < est_k then est_k = ceil(k').
 *    result: transformation of the best hypothesis, fitness = count / n_corres, inlier_rmse = sqrt(err2 / count) -- over the correspondence LIST,
 *    as Open3D (evaluate_registration gives whole-cloud figures) --, iterations = iterations run, converged = a best hypothesis exists;
 *    correspondences (optional, device int32, capacity n_corres rows; n_src rows for the feature form) = the inlier rows of the list in input order.
 *    Fewer rows than ransac_n: the empty result (identity, fitness 0, rmse 0), not an error.  A negative threshold = that checker is absent. */
typedef struct {
    int32_t ransac_n;                 /* 3..8 */
    int32_t with_scaling;             /* TransformationEstimationPointToPoint(with_scaling) */
    int32_t max_iteration;            /* RANSACConvergenceCriteria: 100000 */
    double confidence;                /*                            0.999; in (0, 1], 1 never stops early */
    uint64_t seed;
    double edge_length_threshold;     /* CorrespondenceCheckerBasedOnEdgeLength(similarity_threshold) */
    double distance_threshold;        /* CorrespondenceCheckerBasedOnDistance(distance_threshold) */
    double normal_angle_threshold;    /* CorrespondenceCheckerBasedOnNormal(normal_angle_threshold), radians */
} pcr_ransac_params;
typedef struct {
    int64_t iterations_run;
    int64_t best_iteration;           /* -1: none */
    int64_t n_valid;                  /* hypotheses among those run that passed every checker */
    int64_t n_corres;                 /* rows of the correspondence list RANSAC ran on */
} pcr_ransac_info;
/* corres: device int32 [n_corres x 2] rows (source index, target index); normals optional (read by the normal checker only); info optional */
int pcr_registration_ransac_correspondence(pcr_context *ctx, const float *src_xyz, const float *src_normals, int64_t n_src, const float *tgt_xyz,
                                           const float *tgt_normals, int64_t n_tgt, const int32_t *corres, int64_t n_corres, double max_distance,
                                           const pcr_ransac_params *params, pcr_result *result, int32_t *correspondences, pcr_ransac_info *info);
/* the list is built first: every source row with its nearest target row in feature space (the exact searches of pcr_registration_fgr); with
 * mutual_filter only the rows whose target row points back, unless fewer than ransac_n of them remain (then all rows, as Open3D) */
int pcr_registration_ransac_feature_matching(pcr_context *ctx, const float *src_xyz, const float *src_normals, int64_t n_src, const float *src_feat33,
                                             const float *tgt_xyz, const float *tgt_normals, int64_t n_tgt, const float *tgt_feat33, int mutual_filter,
                                             double max_distance, const pcr_ransac_params *params, pcr_result *result, int32_t *correspondences,
                                             pcr_ransac_info *info);

/* == registration_sc2_based_on_correspondence / spatial_compatibility: global registration by second-order spatial compatibility (after SC2-PCR,
 *    Chen et al., CVPR 2022; Open3D has no such call, so this statement is the specification).  Deterministic: no random numbers, exact integer
 *    counts, float64 sums in a fixed order, no floating-point atomics.
 *    POINTS.  The list is range-checked as every call on a list checks it (PCR_EINVAL with a message).  s_i = source[corres[i,0]],
 *    t_i = target[corres[i,1]], the float32 coordinates widened to float64.  N = n_corres.
 *    LENGTHS.  d2(a, b) = dx*dx + dy*dy + dz*dz in float64, every difference, product and sum rounded once, summed in the order x, y, z (no fused
 *    multiply-add); ls_ij = sqrt(d2(s_i, s_j)), lt_ij = sqrt(d2(t_i, t_j)), IEEE square roots.
 *    COMPATIBLE.  C_ij = (i != j) and |ls_ij - lt_ij| < tau (strict), tau = inlier_threshold.  Symmetric; repeated rows are compatible with each other.
 *    BITS.  bits is N x ceil(N / 64) words of 64 bits; bit b of word w of row i is C_{i, 64 w + b}; the bits past column N - 1 are zero.
 *    COUNTS.  deg_i = sum_j C_ij.  SC2_ij = C_ij * |{k : C_ik and C_jk}|.  score_i = sum_j SC2_ij (int64: twice the triangles through i).
 *    ORDER.  i comes before j iff score_i > score_j, or the scores are equal and i < j.
 *    SEEDS.  i is suppressed iff some j before it has ls_ij < nms_radius (strict; whether j is itself suppressed does not matter; nms_radius = 0
 *    suppresses nothing).  Candidates: the unsuppressed rows with score_i > 0.  The seeds are the first
 *    min(candidates, max(1, (int64)(seed_ratio * N)), max_seeds) candidates in order.
 *    PER SEED m.  K1 = m followed by the first up to k1 rows j with C_mj taken by (SC2_mj descending, j ascending).  Inside K1,
 *    L_ab = C_ab * |{c in K1 : C_ac and C_bc}|.  Of the members a != m of K1 take the first up to k2 by (L_ma descending, position in K1 ascending);
 *    K2 = m followed by those of them with 2 L_ma >= max_a L_ma (the maximum over the members a != m), in that order.  |K2| < 3: the seed is
 *    invalid.  T_m = the Umeyama fit without scaling over the rows of K2; a non-finite T_m is invalid.
 *    SCORE.  As RANSAC: count_m = rows with d2(T s, t) < tau^2 where T s is ((T00 sx + T01 sy) + T02 sz) + T03 per coordinate, err2_m = the sum of
 *    those d2 in float64 in a fixed order.
 *    BEST.  A larger count wins; at equal counts the strictly smaller err2; otherwise the earlier seed stays; a count of 0 is never best.
 *    REFINEMENT.  At most refine_iterations times: I = the inlier rows under T in input order, T' = the point-to-point fit over I (Umeyama without
 *    scaling); T' replaces T iff its count is larger, or equal with a smaller err2; otherwise the loop stops and T stays.
 *    RESULT.  transformation = T, fitness = count / N, inlier_rmse = sqrt(err2 / count) (over the list, as RANSAC), iterations = refinement passes
 *    run, converged = a best seed exists; correspondences (optional, device int32, capacity N rows) = the inlier rows of the list in input order.
 *    N < 3, no seed or no valid seed: the empty result (identity, fitness 0), not an error.
 *    LIMITS (PCR_EINVAL with a message): N <= 65536 (the bit matrix is at most 512 MB; refused before anything is allocated: use the mutual
 *    filter or a keypoint subset), 2 <= k1 <= 63 (K1 fits one wavefront), 1 <= k2 <= k1, tau > 0 and finite, nms_radius >= 0,
 *    0 < seed_ratio <= 1, 1 <= max_seeds <= 65536, refine_iterations >= 0. */
typedef struct {
    double inlier_threshold;          /* tau; no default */
    double nms_radius;                /* the Python layer passes inlier_threshold for None */
    int32_t k1;                       /* 30 */
    int32_t k2;                       /* 20 */
    double seed_ratio;                /* 0.2 */
    int32_t max_seeds;                /* 2048 */
    int32_t refine_iterations;        /* 20 */
} pcr_sc2_option;
typedef struct {
    int64_t n_corres;                 /* rows of the list */
    int64_t n_seeds;
    int64_t n_valid;                  /* seeds with a hypothesis */
    int64_t best_seed;                /* position of the best seed in the order of the seeds; -1: none */
    int64_t best_seed_count;          /* its count before refinement */
    int64_t refine_iterations_run;
} pcr_sc2_info;
/* corres: device int32 [n_corres x 2]; correspondences and info optional */
int pcr_registration_sc2_correspondence(pcr_context *ctx, const float *src_xyz, int64_t n_src, const float *tgt_xyz, int64_t n_tgt, const int32_t *corres,
                                        int64_t n_corres, const pcr_sc2_option *option, pcr_result *result, int32_t *correspondences, pcr_sc2_info *info);
/* the compatibility graph alone; each output is optional (device): bits n_corres x ceil(n_corres / 64) int64, degrees n_corres int32, scores n_corres int64 */
int pcr_spatial_compatibility(pcr_context *ctx, const float *src_xyz, int64_t n_src, const float *tgt_xyz, int64_t n_tgt, const int32_t *corres, int64_t n_corres,
                              double inlier_threshold, int64_t *bits, int32_t *degrees, int64_t *scores);

/* == TransformationEstimationPointToPoint / PointToPlane / ForGeneralizedICP .compute_transformation(source, target, corres) and
 *    .compute_rmse(source, target, corres) (ALL_FUNCTIONS.py:438-439, registro_manual: picked point pairs give the starting pose of a registration).
 *    One fit, or one error figure, over a correspondence list the caller holds.  This statement is the specification.
 *    LIST.  corres: device int32 [n_corres x 2]; row (i, j) pairs source point i with target point j.  The float32 coordinates are widened to
 *    float64; the source is read as given (no pose is applied).  There is NO distance test: every row counts, as in Open3D.  A row may repeat a
 *    source or a target index, and the list may be shorter or longer than n_src: no buffer is sized by n_src.
 *    n_corres == 0: the identity and RMSE 0, not an error.  An index outside [0, n_src) or [0, n_tgt): PCR_EINVAL with a message; a kernel of its
 *    own checks every row, and its count is on the host before any row is read.
 *    SUMS.  Float64, in an order that depends on the list and on the launch geometry only; no floating-point atomics; the same call gives the same
 *    bits on every run.
 *    POINT TO POINT.  T = Eigen::umeyama of the rows (the fit of pcr_registration_icp's update; a scaled pose when with_scaling), the target's
 *    moments taken about the target point of row 0 and the source's about the source point of row 0, so that neither cancels far from the
 *    origin or far from the other cloud.  RMSE = sqrt(sum |s - t|^2 / C).  Rows that do not determine a rotation (one row, collinear rows)
 *    give what the fit gives on them -- for one row, or copies of one row, the identity rotation and the translation s -> t --, as Eigen
 *    does; with_scaling on source points without spread divides by a zero variance: 0 / 0, the pose is not finite (as Eigen's).
 *    POINT TO PLANE.  With n the target normal AS STORED (not normalised): r = (s - t).n, J = [s x n, n], w = the kernel's weight of r (L2: 1,
 *    L1: 1 / |r|, GM: k / (k + r^2)^2), JTJ = sum w J^T J, JTr = sum w J r, solved as the loop solves it (LDLT, pivoted when a pivot is not
 *    positive), the pose Rz Ry Rx and the translation.  A system that cannot be solved gives the identity, and so does a target without normals
 *    (Open3D).  RMSE = sqrt(sum r^2 / C), 0 without target normals.  "Cannot be solved" is decided by the pivots: a system whose rank
 *    deficiency is exact (a floor, a corridor, a sphere with exact normals: whole columns of J zero) meets an exact zero pivot and gives the
 *    identity bit for bit; one that is deficient only in exact arithmetic (fewer rows than unknowns, nearly dependent columns) has a last pivot
 *    of rounding size and either sign, and gives a finite pose that is not pinned.
 *    L1 AT r == 0.  Open3D divides by zero there: its sums turn NaN, its solve fails and it returns the identity.  Here the weight is
 *    1 / max(|r|, 1e-300): such a row enters JTJ with 1e300 J^T J, beside which every other row vanishes, and adds nothing to JTr.  The
 *    update is then finite and a negligible distance from the identity (|T - I| of 1e-280 and less has been seen) but NOT the identity bit for
 *    bit, and not the fit over the remaining rows either; it is the same bits on every run.  (The loop, pcr_registration_icp, does the same.)
 *    GENERALIZED ICP.  Both clouds carry covariances (cov6 = xx,xy,xz,yy,yz,zz, float32): the rows of pcr_registration_generalized_icp_cov at
 *    T = identity, M = Cs + Ct, W = M^(-1/2), three rows W (s - t) per pair, each weighted by the kernel.  Neither carries covariances and both
 *    carry normals: the rows of pcr_registration_generalized_icp at T = identity (normals normalised, e1 when n.x < -0.99, covariance
 *    I - (1 - epsilon) n n^T).  Any other case: the identity, what Open3D returns without covariances.  RMSE = sqrt(sum |s - t|^2 / C): Open3D's
 *    GICP RMSE is Euclidean.
 *    T16 and rmse are host pointers; the calls return when they are written. */
typedef enum { PCR_EST_POINT_TO_POINT = 1, PCR_EST_POINT_TO_PLANE = 2, PCR_EST_GENERALIZED_ICP = 3 } pcr_estimation_kind;
typedef struct {
    int32_t kind;             /* pcr_estimation_kind */
    int32_t with_scaling;     /* point-to-point */
    int32_t loss;             /* point-to-plane, GICP: pcr_loss_kind of the robust kernel */
    double loss_k;            /* GMLoss k */
    double epsilon;           /* GICP with normals: covariance regulariser, 1e-3 */
} pcr_estimation;
int pcr_estimation_compute_transformation(pcr_context *ctx, const pcr_estimation *estimation, const float *src_xyz, const float *src_normals,
                                          const float *src_cov6, int64_t n_src, const float *tgt_xyz, const float *tgt_normals, const float *tgt_cov6,
                                          int64_t n_tgt, const int32_t *corres, int64_t n_corres, double *T16);
int pcr_estimation_compute_rmse(pcr_context *ctx, const pcr_estimation *estimation, const float *src_xyz, const float *src_normals,
                                const float *src_cov6, int64_t n_src, const float *tgt_xyz, const float *tgt_normals, const float *tgt_cov6,
                                int64_t n_tgt, const int32_t *corres, int64_t n_corres, double *rmse);

/* == correspondences_from_features(source_features, target_features, mutual_filter, mutual_consistency_ratio) (Open3D 0.17 and later): the list
 *    the feature forms of RANSAC and FGR match on.  Row i of the source is paired with its nearest target row: the smallest sum (a_k - b_k)^2 in
 *    float64 over the float32 features, ties to the smaller index (the exact search of pcr_registration_fgr).  Without mutual_filter: rows
 *    (i, nearest(i)) for every source row, in source order.  With it: only the rows whose target row points back, provided their count is
 *    >= (int)(mutual_consistency_ratio * n_src); otherwise all rows (Open3D; its default ratio is 0.1).  A ratio of 0 always returns the mutual
 *    list, even an empty one.  feature_dim must be 33 (FPFH); any other dimension, a negative or non-finite ratio: PCR_EINVAL.
 *    corres: device int32, capacity n_src x 2; *n_corres (host) = rows written.  An empty cloud on either side gives 0 rows. */
int pcr_correspondences_from_features(pcr_context *ctx, const float *src_feat, int64_t n_src, const float *tgt_feat, int64_t n_tgt, int feature_dim,
                                      int mutual_filter, double mutual_consistency_ratio, int32_t *corres, int64_t *n_corres);

/* == registration_fgr_based_on_correspondence(source, target, corres, option): pcr_registration_fgr from the point where it holds its
 *    cross-checked list of feature matches, with the caller's list in that place (rows (source index, target index), device int32
 *    [n_corres x 2], checked as for the estimators above).  Both clouds are normalised as there.  With option.tuple_test (and
 *    maximum_tuple_count > 0; < 0 = the per-pair rule of pcr_registration_fgr) the tuple test draws its 100 * n_corres trials from the list in
 *    its given order with the same sampler and seed, so that a list equal to the feature form's gives the feature form's bits; otherwise every
 *    row goes to the optimiser, for any pair of cloud sizes.  [O3D ?] Open3D's own order of the rows inside this function (it may swap the
 *    clouds by size as the feature form does) is not pinned against a build of it.  Fewer than 10 rows for the optimiser: the identity pose.
 *    result / correspondences (optional, capacity n_src rows): evaluate_registration at maximum_correspondence_distance under the pose found,
 *    as in the feature form. */
int pcr_registration_fgr_correspondence(pcr_context *ctx, const float *src_xyz, int64_t n_src, const float *tgt_xyz, int64_t n_tgt,
                                        const int32_t *corres, int64_t n_corres, const pcr_fgr_option *option, pcr_result *result,
                                        int32_t *correspondences);

/* == PointCloud.segment_plane (Open3D PointCloud::SegmentPlane; the reference calls it nowhere and Open3D's own result depends on its random
 *    engine and thread timing, so the algorithm is stated here and this statement is the specification).  [O3D ?] marks what is recalled from
 *    SegmentPlane / GetPlaneFromPoints and not pinned against a build of Open3D.  ONE sequential loop over hypotheses i = 0, 1, ... defines the
 *    answer, bit for bit for a given seed; the device may only reorder work that cannot change it.
 *    SAMPLE.  Hypothesis i draws rows r_k = splitmix64(seed + ransac_n * i + k) % n, k < ransac_n (the sampler of the registration RANSAC above;
 *    repeats allowed).
 *    FIT.  Float64 on the float32 coordinates; every product, sum, quotient and square root rounded on its own (no fused multiply-add), in the
 *    order written here, so that a host recomputation gives the same bits (csrc/pcr_plane.h is that order in code, host and device).
 *    ransac_n == 3: u = p1 - p0, v = p2 - p0, normal N = u x v = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx), origin o = p0.
 *    ransac_n in 4..8, and the final refit: the moment fit [O3D ?].  Sums S = ((p_0 + p_1) + p_2) + ... over k = 0 .. ransac_n - 1 per
 *    coordinate, centroid o = S / count; second moments about it, q_k = p_k - o, xx = sum qx qx, xy = sum qx qy, xz, yy, yz, zz in the same order of
 *    k (sums, not divided by the count); det_x = yy zz - yz yz, det_y = xx zz - xz xz, det_z = xx yy - xy xy;
 *      det_x > det_y and det_x > det_z:  N = (det_x, xz yz - xy zz, xy yz - xz yy)
 *      else det_y > det_z:               N = (xz yz - xy zz, det_y, xy xz - yz xx)
 *      else:                             N = (xy yz - xz yy, xy xz - yz xx, det_z).
 *    Both: norm = sqrt((Nx Nx + Ny Ny) + Nz Nz), (a, b, c) = N / norm, d = -((a ox + b oy) + c oz).  A norm that is not > 0 or a plane that is
 *    not finite makes the hypothesis INVALID; it still uses up its iteration.
 *    SCORE.  dist_j = |((a x_j + b y_j) + c z_j) + d|, one expression for the score, the final inlier pass and the test hook.  Point j is an
 *    inlier iff dist_j < distance_threshold (strict).  count_i = number of inliers, err_i = sum of dist_j over them ([O3D ?]: Open3D sums the
 *    distance, not its square), rmse_i = err_i / sqrt(count_i).  The sum is taken in a fixed order: same bits on every run, no float atomics.
 *    BETTER.  i is better than the running best if count_i is larger, or equal with rmse_i strictly smaller; count 0 is never better than the
 *    empty start; on a full tie the earlier iteration stays.
 *    STOP.  est_k = num_iterations at the start, iteration i runs iff i < est_k.  When i becomes the best and probability < 1,
 *    k' = log(1 - probability) / log1p(-(count_i / n)^ransac_n), k' = 0 when count_i == n; if k' is finite and 0 <= k' < est_k then
 *    est_k = ceil(k').  probability == 1 never stops early.
 *    RESULT.  Inliers: the rows with dist_j < distance_threshold against the BEST HYPOTHESIS's plane, ascending.  plane4 = the moment fit over
 *    those inliers (Open3D's last step; the centroid is sum / count and the moments are summed about it, both in a fixed order on the device),
 *    with whatever sign the fit gives; a degenerate fit gives the zero plane.  No valid hypothesis with an inlier: the zero plane, no inliers,
 *    best_iteration = -1; not an error.  num_iterations == 0: the same empty result.
 *    PCR_EINVAL (the message names segment_plane): ransac_n outside 3..8 (Open3D has no upper limit; 8 is this library's RANSAC limit),
 *    n < ransac_n (Open3D raises too), n above the int range, a null xyz or plane4, distance_threshold negative or not finite,
 *    num_iterations < 0, probability outside (0, 1]. */
typedef struct {
    int32_t ransac_n;                 /* 3; 3..8 */
    int32_t num_iterations;           /* 100 */
    double probability;               /* 0.99999999; in (0, 1], 1 never stops early */
    uint64_t seed;
} pcr_plane_params;
typedef struct {
    int64_t iterations_run;
    int64_t best_iteration;           /* -1: none */
    int64_t n_valid;                  /* valid hypotheses among those run */
    int64_t n_inliers;                /* count of the best hypothesis = rows in the index list */
    double fitness, inlier_rmse;      /* of the best hypothesis: count / n and err / sqrt(count) */
} pcr_plane_info;
/* xyz: device, n x 3 float32.  plane4 (host): a, b, c, d.  inlier_mask (optional, device, n bytes) and out_index (optional, device int64, capacity n,
 * ascending) + out_n (optional, host): the layout of pcr_remove_radius_outlier.  info optional (host). */
int pcr_segment_plane(pcr_context *ctx, const float *xyz, int64_t n, double distance_threshold, const pcr_plane_params *params, double *plane4,
                      uint8_t *inlier_mask, int64_t *out_index, int64_t *out_n, pcr_plane_info *info);

/* == PointCloud.farthest_point_down_sample(num_samples, start_index) (Open3D PointCloud::FarthestPointDownSample; the reference calls it nowhere).
 *    Open3D is not at hand, so the loop is stated here as recalled and this statement is the specification; [O3D ?] marks what is recalled and
 *    not pinned against a build of Open3D: the whole loop below, its tie order and what it does once no point is
 *    away from the samples.  ONE sequential loop of num_samples dependent steps defines the answer, bit for bit and the same on every run; the
 *    device may only reorder work that cannot change it.
 *    DIST.  d^2(j, s) between rows j and s is taken in float64 on the float32 coordinates: differences, squares and sums in the order x, y, z,
 *    each rounded once, no fused multiply-add (the rule of the search index above), so a host recomputation gives the same bits.
 *    INIT.  dist_j = +inf for every row; a row with a non-finite coordinate instead has dist_j = -1, is never updated and is never chosen.
 *    cur = start_index.
 *    STEP i = 0 .. num_samples - 1.  sel[i] = cur.  For every finite row, dist_j = d^2 < dist_j ? d^2 : dist_j with d^2 = d^2(j, cur).
 *    m = max_j dist_j, with m starting from 0.  If m > 0, cur becomes the SMALLEST index with dist_j == m ([O3D ?]: Open3D scans the rows in
 *    ascending order with a strict >).  Otherwise cur stays: a cloud with no point away from its samples repeats the last index, as Open3D's
 *    loop does [O3D ?].
 *    RESULT.  out_index = sel, in selection order.  cover_dist2 = m after the last step: the largest squared distance of any finite row to the
 *    subset (its square root is the cover radius).  out_dist2 (optional, n float64) = the final dist_j, -1 on non-finite rows.
 *    ERRORS.  PCR_EINVAL, the message naming farthest_point_down_sample: num_samples < 0 or > n (Open3D raises too); start_index outside
 *    0..n-1 when num_samples > 0; start_index naming a non-finite row; n above the int range; a null cloud with n > 0; a null out_index with
 *    num_samples > 0.  num_samples == 0 returns PCR_OK and writes nothing.
 *    Two forms of the loop give the same bits: one launch per step, and one persistent launch of co-resident workgroups that keep the cloud
 *    in LDS and meet at a bounded barrier per step; if the barrier's wait runs out the call is repeated in the first form (fell_back). */
typedef struct {
    int32_t form;                     /* the form that produced the answer: 0 one launch per step, 1 one persistent launch */
    int32_t workgroups;               /* of that form */
    int32_t fell_back;                /* 1: the persistent launch gave up waiting and the step form redid the call */
    double cover_dist2;               /* m after the last step */
} pcr_fps_info;
/* xyz: device, n x 3 float32.  out_index: device int64, num_samples entries.  out_dist2: optional, device, n float64.  info: optional, host.
 * Runs on the context's stream with scratch from its arena; returns after the one read of the loop's small state record. */
int pcr_farthest_point_sample(pcr_context *ctx, const float *xyz, int64_t n, int64_t num_samples, int64_t start_index, int64_t *out_index,
                              double *out_dist2, pcr_fps_info *info);

/* == PointCloud.orient_normals_consistent_tangent_plane(k), orient_normals_to_align_with_direction, orient_normals_towards_camera_location and
 *    normalize_normals (Open3D PointCloud::OrientNormalsConsistentTangentPlane and its relatives in EstimateNormals.cpp; the reference calls
 *    none of them).  estimate_normals leaves every normal with the sign its eigen-solver gave it; these make the signs agree.  Open3D is not
 *    at hand and its Kruskal sorts with an unstable sort, so the statement below is the specification; [O3D ?] marks what is recalled from
 *    Open3D and not pinned against a build of it: the Riemannian graph as EMST plus k-NN graph with weight 1 - |n_i . n_j| [O3D ?], the root
 *    as the row with the largest z, turned to +z [O3D ?], the breadth-first walk that negates a child iff (oriented parent) . child < 0
 *    [O3D ?], and that the k of SearchKNN counts the query row itself [O3D ?].
 *    DIST.  d^2(i, j) follows the rule of the search index: float64 on the float32 coordinates, differences, squares and sums in the order
 *    x, y, z, each rounded once, no fused multiply-add.
 *    DOT.  c(i, j) = (nx_i nx_j + ny_i ny_j) + nz_i nz_j in float64 on the float32 normals, each operation rounded once.  w(i, j) = 1 - |c(i, j)|.
 *    ORDER.  An undirected edge {i, j} has the key (weight, lo, hi), lo = min(i, j), hi = max(i, j) in the caller's row numbers; keys are
 *    compared lexicographically, weights numerically.  This is a strict total order, so every "minimum spanning tree" below is unique and
 *    does not depend on the algorithm that finds it.  Two copies of the same edge are the same edge.
 *    EMST.  The minimum spanning tree of the complete graph under ORDER with weight d^2: n - 1 edges.  Duplicated points give d^2 = 0 edges,
 *    ordered by (lo, hi).
 *    KNN.  For row i, the first k rows of the whole cloud ordered by (d^2(i, .), index); row i takes part in that ordering and is then
 *    skipped.  k >= n means every row, k = 0 none.
 *    GRAPH.  E = EMST + { {i, j} : j in KNN(i) } with weight w(i, j): connected, because it contains the EMST.
 *    TREE.  The minimum spanning tree of (rows, E) under ORDER with weight w.
 *    ROOT.  r = the smallest row with the largest z (float32 comparison).  flip_r = (nz_r < 0).
 *    PROPAGATE.  For a tree edge s(i, j) = (c(i, j) < 0); flip_v = flip_r XOR the XOR of s over the tree path r -> v.  That is the
 *    breadth-first walk; a dot product of exactly 0 flips nothing in either direction.  The tree and every flip_v depend only on |c| and on
 *    the root rule, so the output does not depend on the input signs.
 *    RESULT.  Where flip_v holds all three components of the row are negated, otherwise the row's bits are untouched.  n = 0: PCR_OK,
 *    nothing is written.  n = 1: the root rule only.
 *    ERRORS.  PCR_EINVAL, the message naming orient_normals_consistent_tangent_plane: a null cloud or null normals with n > 0; n above the int
 *    range; k < 0 or above the search index's limit (200); any non-finite coordinate or normal component (the message says "non-finite").
 *    On error nothing is written.
 *    Both trees are found by Boruvka rounds (csrc/pcr_orient.hip; at most ceil(log2 n) each, the host reads one small record per round).
 *    The element-wise calls use float64 on the float32 data, sums in the order x, y, z.  direction(ref) [O3D ?]: a zero normal becomes ref
 *    rounded to float32, otherwise the normal is negated iff n . ref < 0.  camera(loc) [O3D ?]: v = loc - p_i; a zero normal becomes v / |v|,
 *    or (0, 0, 1) when v is zero, otherwise the normal is negated iff n . v < 0.  normalize [O3D ?]: n / |n|, a zero normal stays zero. */
typedef struct {
    int32_t emst_rounds, tree_rounds; /* Boruvka rounds of the two trees */
    int64_t walked_rows;              /* rows, over all EMST rounds, that walked the octree: their k-NN list held no row of another component */
    int64_t n_flipped;                /* rows negated */
    int64_t root;                     /* r (-1: none, pcr_euclidean_mst) */
} pcr_orient_info;
/* EMST alone (single-linkage clustering reads it directly).  xyz: device, n x 3 float32.  edges: device int32, (n - 1) x 2, rows (lo, hi) ascending
 * by (lo, hi).  d2: optional, device, n - 1 float64, aligned with edges.  info: optional, host.  n <= 1 writes nothing.  PCR_EINVAL (the message naming
 * euclidean_minimum_spanning_tree) for a null cloud with n > 0, null edges with n > 1, n above the int range or a non-finite coordinate. */
int pcr_euclidean_mst(pcr_context *ctx, const float *xyz, int64_t n, int32_t *edges, double *d2, pcr_orient_info *info);
/* normals: device, n x 3 float32, updated in place.  flipped: optional, device, n bytes (flip_v).  tree_edges: optional, device int32, (n - 1) x 2, the
 * layout of pcr_euclidean_mst.  info: optional, host. */
int pcr_orient_normals_tangent_plane(pcr_context *ctx, const float *xyz, float *normals, int64_t n, int k, uint8_t *flipped, int32_t *tree_edges,
                                     pcr_orient_info *info);
/* mode 0: direction(ref), xyz may be null; mode 1: camera(ref).  ref: host, 3 float64. */
int pcr_orient_normals(pcr_context *ctx, const float *xyz, float *normals, int64_t n, int mode, const double *ref);
int pcr_normalize_normals(pcr_context *ctx, float *normals, int64_t n);

/* == PointCloud.compute_boundary_points(radius, max_nn, angle_threshold) (Open3D t::geometry::PointCloud::ComputeBoundaryPoints, the angle
 *    criterion of PCL's BoundaryEstimation; the reference calls it nowhere): the points on the rim of the sampled surface -- occlusion shadows,
 *    the edge of the field of view, holes.  Open3D is not at hand, so the rule is stated here and this statement is the specification.  Per
 *    point i, with p the float32 coordinates and n the float32 normals, both read into float64:
 *    1. NEIGHBOURHOOD.  The row pcr_index_hybrid returns for the query p_i on the cloud itself: every point with d^2 < radius^2 (strict, d^2 in
 *       float64 on the float32 coordinates, unfused, in the order x, y, z), ordered by (d^2, caller index), the first max_nn of them.  The point
 *       itself and coincident points are members.  count_i is the row length.
 *    2. NORMAL.  Taken as a unit vector, as Open3D takes it: it is not normalised.  A row whose normal has a non-finite component or is
 *       (0, 0, 0) is undecided: not boundary, gap 0.  So is a row whose point has a non-finite coordinate: it finds nothing (count 0), and it
 *       is nobody's neighbour.
 *    3. TANGENT FRAME.  a = the axis with the smallest |n component|, on a tie x before y before z; e = that unit axis.  v = n x e, u = v x n.
 *       A cross product p x q is (p_y q_z - p_z q_y, p_z q_x - p_x q_z, p_x q_y - p_y q_x), every product and every difference rounded once, no
 *       fused multiply-add.
 *    4. ANGLES.  For every member j in row order: d = p_j - p_i, x = (u_x d_x + u_y d_y) + u_z d_z, y = (v_x d_x + v_y d_y) + v_z d_z, unfused.
 *       A member with x == 0 and y == 0 is skipped: the point itself, coincident points, a point exactly on the normal line.  Otherwise its
 *       angle is atan2(y, x) in float64.  m = the number of angles.
 *    5. GAP.  m == 0: gap 0, not boundary.  Otherwise, with the angles sorted ascending a_0 .. a_{m-1}:
 *       gap = max(the largest a_{t+1} - a_t, 2 pi - (a_{m-1} - a_0)), 2 pi = 2.0 * M_PI; m == 1 gives 2 pi.
 *    6. VERDICT.  Boundary iff gap > T, T = angle_threshold * M_PI / 180.0 evaluated left to right.
 *    Everything up to the arguments of atan2 is fixed bit for bit: a host recomputation in that order gives the same bits.  atan2 itself is
 *    not: the device's and libm's differ by ulps.  The largest circular gap is a continuous function of the angles (two nearly equal angles
 *    changing places, or one moving from pi to -pi, change it by rounding only), so the reported gap carries an error of a few 1e-16 and the
 *    verdict can differ from a host recomputation only for a gap within rounding of T.  Two runs give the same bits in every output.
 *    TWO DEVIATIONS from Open3D, [O3D ?] = recalled and not pinned against a build of it: the tangent frame is
 *    this library's (Open3D's GetCoordinateSystemOnPlane chooses another one [O3D ?]; in exact arithmetic the gap does not depend on the
 *    frame), and the row order -- which decides the members of a ball of more than max_nn points that has ties in d^2 -- is this library's
 *    total order (d^2, caller index) [O3D ?].
 *    ERRORS.  PCR_EINVAL with a message naming boundary_points: radius not finite or <= 0; max_nn outside 1..200 (the search index's limit);
 *    angle_threshold not finite or outside [0, 360]; n < 0 or above the int range; a null xyz or normals with n > 0.  n == 0: PCR_OK, *out_n = 0.
 * xyz, normals: device, n x 3 float32.  Device, each optional: boundary_mask (n bytes), out_xyz (capacity n x 3), out_index (capacity n int64,
 * ascending: the layout of pcr_remove_radius_outlier and pcr_iss_keypoints), max_gap (n float64, radians, caller order), counts (n int32, the
 * count_i of rule 1).  Host: out_n (optional).  Asynchronous on the context's stream except for the read of the count; scratch from the
 * context's arena (12 bytes per row place: n x max_nn x 12 for the rows). */
int pcr_boundary_points(pcr_context *ctx, const float *xyz, const float *normals, int64_t n, double radius, int max_nn, double angle_threshold,
                        uint8_t *boundary_mask, float *out_xyz, int64_t *out_index, int64_t *out_n, double *max_gap, int32_t *counts);

/* == Scan Context place recognition (Kim and Kim, "Scan Context: egocentric spatial descriptor for place recognition within 3D point cloud
 *    map", IROS 2018; the reference calls nothing like it): a polar height image of a ring-LiDAR scan, and the distance of two images that
 *    tells whether two scans were taken at the same place, whatever the heading.  The rule is stated here and this statement is the
 *    specification; tests/scan_context_reference.py restates it in numpy and the device gives its rows bit for bit, the same bits every run.
 *    PARAMETERS.  num_rings R in 1..64 (default 20), num_sectors S in 4..128 and a multiple of 4 (default 60), max_range L > 0 (default 80.0),
 *    height_offset h finite (default 2.0: the sensor's height, so that the ground is near 0).
 *    TABLES.  No transcendental function evaluated on the device decides a bin (atan2 and sqrt of different libms differ in the last bit, and a
 *    bin boundary would turn that into another descriptor).  The host passes, in float64: ring_bound2[k - 1] = ((double)k * L / R)^2 for
 *    k = 1..R-1; cos_k[k - 1] = cos(2 pi k / S) and sin_k[k - 1] = sin(2 pi k / S) for k = 1..S/4-1; range2 = L * L.
 *    DESCRIPTOR of a cloud of float32 points in the sensor's frame, z up:
 *    1. A row with a non-finite coordinate is dropped.
 *    2. With x, y widened to float64, rho2 = x * x + y * y (the products are exact, the sum is rounded once).  The row is dropped when
 *       rho2 >= range2 or rho2 == 0.
 *    3. ring = the number of k with rho2 >= ring_bound2[k - 1].
 *    4. The quadrant q is 0 for x > 0, y >= 0; 1 for x <= 0, y > 0; 2 for x < 0, y <= 0; 3 for x >= 0, y < 0.  (u, v) = (x, y), (y, -x),
 *       (-x, -y), (-y, x) for q = 0, 1, 2, 3, so u > 0 and v >= 0.
 *    5. within = the number of k in 1..S/4-1 with v * cos_k >= u * sin_k, each product rounded once in float64, nothing contracted.
 *       sector = q * S / 4 + within.
 *    6. The value of the row is (float)z + (float)h in float32.  The cell (ring, sector) holds the maximum value of its rows; a maximum of
 *       -0.0 is stored as +0.0; a cell without rows holds 0.  The descriptor is (R, S) float32, row-major.
 *    7. The info record counts the rows used, dropped as non-finite (rule 1) and dropped by range (rule 2).
 *    DISTANCE of descriptor A (the query) and descriptor B (the candidate), both widened to float64:
 *    1. nA[j] = the sum over r = 0..R-1, in that order, of A[r,j]^2; nB[j] likewise.  G[j,j'] = the sum over r, in that order, of
 *       A[r,j] * B[r,j'].  No multiply-add is contracted.
 *    2. A column pair (j, j') is valid when nA[j] > 0 and nB[j'] > 0; then C[j,j'] = G[j,j'] / (sqrt(nA[j]) * sqrt(nB[j'])).
 *    3. For the shift n in 0..S-1, with j' = (j - n) mod S (column j of B rolled right by n): m_n = the number of valid pairs (j, j'),
 *       d_n = 1 - (the sum over j ascending of the valid C[j,j']) / m_n, and d_n = 1 when m_n = 0.
 *    4. The distance is the smallest d_n, the shift the smallest n that attains it.
 *    MEANING OF THE SHIFT.  Turning B's cloud by +2 pi n / S about z lines it up with A's: Rz(2 pi n / S) is the initial pose of a
 *    registration with B's cloud as source and A's cloud as target.
 *    ARITHMETIC.  sqrt and the division of float64 are correctly rounded on gfx950 under this library's flags (measured against numpy on
 *    2^21 operands each), so the rule stands as the method's authors wrote it.  Descriptors with non-finite entries are outside
 *    the rule (their cosines are not numbers; the kernel marks a pair that is not valid with a NaN of its own).
 *    ERRORS.  PCR_EINVAL with a message naming scan_context / scan_context_distance: null params, tables, output or (with rows) input
 *    pointers; R or S out of range, S not a multiple of 4; max_range or range2 not finite or <= 0; height_offset not finite (as float32);
 *    a missing table that the shape needs, or ring bounds that are not positive and ascending; a negative row count, or one over the int range.
 * pcr_scan_context: xyz device, n x 3 float32; params, tables (and the arrays they name) host; out_desc device, R x S float32; out_info
 * optional, host (the call waits for the counts when it is given).  n == 0 gives the all-zero descriptor.  pcr_scan_context_distance: descA
 * (nA x R x S) and descB (nB x R x S) device float32; out_dist device, nA x nB float64, out_shift device, nA x nB int32, row-major.  nA == 0
 * or nB == 0 returns PCR_OK and writes nothing.  Both run asynchronously on the context's stream. */
typedef struct {
    int32_t num_rings, num_sectors;
    double max_range, height_offset;
} pcr_scan_context_params;
typedef struct {
    const double *ring_bound2;        /* R - 1 entries (may be null for R == 1) */
    const double *cos_k, *sin_k;      /* S / 4 - 1 entries each (may be null for S == 4) */
    double range2;
} pcr_scan_context_tables;
typedef struct {
    int64_t used, dropped_nonfinite, dropped_range;
} pcr_scan_context_info;
int pcr_scan_context(pcr_context *ctx, const float *xyz, int64_t n, const pcr_scan_context_params *params, const pcr_scan_context_tables *tables,
                     float *out_desc, pcr_scan_context_info *out_info);
int pcr_scan_context_distance(pcr_context *ctx, const float *descA, int64_t nA, const float *descB, int64_t nB, int R, int S, double *out_dist,
                              int32_t *out_shift);

/* == Joint multiway registration of a set of scans (Lu and Milios 1997; Borrmann et al., "Globally consistent 3D mapping with scan matching",
 *    RAS 2008; PCL ships it as registration::LUM.  Open3D has no such call and the reference's "LUM" works on poses alone).  All scans of a
 *    graph go into one least-squares problem whose correspondences are searched again, edge by edge, at the current poses of every
 *    iteration.  The device part is the linearisation of a whole edge list in one call; the assembly, the gauge, the solve and the loop are
 *    host float64 (multiway.py).  This statement is the specification; tests/multiway_reference.py restates it in numpy.
 *    PROBLEM.  n clouds; cloud i has float32 points and, where the estimator needs them, float32 normals.  A node pose T_i is float64 4x4 and
 *    maps cloud i into the common frame (PoseGraphNode.pose, poses_relativas_para_absolutas).  An edge (a, b), a != b, makes cloud a the source
 *    and cloud b the searched target.  The same pair may appear in both directions and more than once.
 *    ROWS OF AN EDGE AT M (M = the pose of a in the frame of b, float64, row-major 4x4 of which the first three rows are read, given by the
 *    caller; the loop passes inv(T_b) T_a with the rigid inverse (R^T, -R^T t)).
 *    1. For a source point p = (x, y, z): q_r = ((M_r0 x + M_r1 y) + M_r2 z) + M_r3 in float64, every product and sum rounded once, nothing
 *       contracted (numpy's elementwise expression gives the same bits).
 *    2. qf = (float)q, component by component.
 *    3. The correspondence is the row of the index rule (pcr_index_hybrid with max_nn = 1 and radius = max_correspondence_distance) for the
 *       query qf in cloud b: the smallest (float64 d^2, caller index) with d^2 < radius * radius, strict, or none.  A non-finite qf finds
 *       nothing, and so does every query in an empty cloud b.
 *    SUMS OF AN EDGE, in the frame of b.  s = q (the float64 of step 1, not qf), t and n_t the matched point and its normal as stored, widened
 *    to float64, w = the robust kernel's weight of a row's r as pcr_estimation_compute_transformation forms it (L2: 1, L1:
 *    1 / max(|r|, 1e-300), GM: k / (k + r^2)^2).
 *      PCR_EST_POINT_TO_PLANE    one row per match: r = (s - t).n_t, J = [s x n_t, n_t].
 *      PCR_EST_POINT_TO_POINT    three unweighted rows per match: r = s - t, J = [-skew(s) | I].  with_scaling != 0 is PCR_EINVAL.
 *      PCR_EST_GENERALIZED_ICP   from normals, the rows of pcr_registration_generalized_icp at the pose M: both normals normalised, e1 where
 *                                n.x < -0.99, C = I - (1 - epsilon) n n^T, W = (C_t + R C_s R^T)^(-1/2) with R the rotation of M, three rows
 *                                r = W (s - t), J = W [-skew(s) | I], each weighted by the kernel's weight of its own r.
 *    Per edge: JTJ = sum w J^T J (6 x 6, unknowns ordered rotation then translation), JTr = sum w J r (6), rows = the number of matched source
 *    points, stats = {sum_d2, sum_r2, sum_wr2}: the sums of the search's float64 d^2, of r^2 and of w r^2 over the rows.
 *    Everything is summed in float64 without floating-point atomics.  The source points are taken in the Morton order of the source's own
 *    index, in tiles of PCR_MULTIWAY_TILE; a tile's sum is a fixed tree over its points and an edge's sum adds its tiles in ascending order.
 *    The order of an edge's sum therefore depends on that edge's two clouds and the launch geometry only, not on what else is in the list:
 *    the same edge gives the same bits on every run, in any position of any list.
 *    JOINT SYSTEM (host).  The update is T_i <- V(x_i) T_i with V = TransformVector6dToMatrix4d (Rz Ry Rx, then the translation).  With
 *    A = Ad(inv(T_b)), for (R, t) the block matrix [[R, 0], [skew(t) R, R]], an edge contributes H_w = A^T JTJ A and g_w = A^T JTr: H_w is
 *    added to the blocks (a, a) and (b, b) and subtracted from (a, b) and (b, a); g_w is added to g_a and subtracted from g_b.  The step
 *    solves H x = -g.  GAUGE: the unknowns of reference_node are removed; a node touched by no edge with rows > 0 is removed too and keeps its
 *    pose; every connected component (over the edges with rows > 0) that does not hold the reference node has its lowest-numbered node
 *    removed as well.  A solve that fails or gives a non-finite x ends the loop: converged = false, the poses stay those of the last
 *    completed step.
 *    LOOP.  RegistrationICP's: linearise at the given poses, then update / linearise until |d fitness| < relative_fitness and
 *    |d rmse| < relative_rmse, or max_iteration updates; fitness = sum rows / sum over the edges of n_a, inlier_rmse =
 *    sqrt(sum sum_d2 / sum rows).
 *    ERRORS.  PCR_EINVAL with a message naming the argument: edges (an index outside [0, n_clouds), a == b), max_correspondence_distance
 *    (not finite or <= 0), M (a non-finite entry), estimation (null, an unknown kind or loss, with_scaling), normals (an estimator that needs
 *    normals a cloud does not carry: point-to-plane the target's, GICP both; the message names the cloud).
 * pcr_multiway_create: xyz[i] device, n[i] x 3 float32 (may be null when n[i] == 0, which is valid); normals may be null, and so may single
 * entries; the problem keeps a search index (pcr_index_create) and a copy of the normals per cloud in device memory of its own until
 * pcr_multiway_destroy, so the caller's arrays may be freed when it returns.  pcr_multiway_linearize: edges2 host int32 E x 2 rows (a, b); M
 * host float64 E x 16; JTJ host E x 36 (full symmetric matrices), JTr host E x 6, stats host E x 3, rows host int64 E; match optional, device
 * int32 with one entry per source point of every edge in edge order (edge e starts at the sum of n_a over the edges before it; entry i is
 * the caller index in b matched to caller point i of a, or -1).  E == 0 is valid.  The call is finished when it returns. */
#define PCR_MULTIWAY_TILE 256
typedef struct pcr_multiway pcr_multiway;
int pcr_multiway_create(pcr_context *ctx, int n_clouds, const float *const *xyz, const float *const *normals, const int64_t *n, pcr_multiway **problem);
int pcr_multiway_destroy(pcr_multiway *problem);
int pcr_multiway_linearize(pcr_context *ctx, const pcr_multiway *problem, const int32_t *edges2, int64_t E, const double *M,
                           double max_correspondence_distance, const pcr_estimation *estimation, double *JTJ, double *JTr, double *stats,
                           int64_t *rows, int32_t *match);

/* ============================================================================================ scan-to-map ICP on a voxel point map
 * The third map of the family keeps raw POINTS, not statistics: a voxel hash with at most M points per cell, the local map of KISS-ICP (Vizzo
 * et al., RA-L 2023).  Point-to-point and point-to-plane ICP run on it with a cost that follows the scan, not the map: a source point probes 1, 7
 * or 27 cells of the cell hash and scans their members.  Open3D has no such call; this statement is the specification, and
 * tests/point_map_reference.py restates it in numpy.
 *
 * MAP.  Input: n >= 1 float32 points; optionally one float32 normal per point (all rows or none; a map has normals or has none);
 *   voxel_size; max_points_per_voxel M in 1 .. 64; a grid by the GRID rule of the voxel covariance map: grid_min g (float64 x3),
 *   origin = g - voxel_size / 2, index = floor((p - origin) / voxel_size) in float64 on the float32 value, 21 bits per axis.  pcr_point_map_create
 *   takes g = the cloud's minimum.  The members of a cell are the input points that fall into it, in input order; the first min(count, M) are
 *   kept and the others are dropped.  The map's ROWS are the kept points, ordered by (Morton key of the cell as in the voxel covariance map,
 *   input order); a row is the float32 point, with its normal in a map that has normals, bit for bit.  The CELL TABLE lists the occupied cells in
 *   Morton order with their first row and member count (1 .. M); the cell hash holds cell -> (first row, count).  A map never has zero rows.
 * ON A GRID, AT A POSE T (float64 4x4, row-major).  Member point p' = float32(q), q the float64 ROWS expression of the voxel maps,
 *   q_r = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3, every operation rounded once.  Member normal n' = float32(R n) with R the upper 3x3 of T, entry by
 *   entry (a0 b0 + a1 b1) + a2 b2 in float64, uncontracted and NOT normalised.  T == NULL: the members are the inputs bit for bit (no expression
 *   is applied, so -0 stays -0).  A member whose cell index lies outside [0, 2^21) on any axis -- below the origin counts too -- or that is not
 *   finite is PCR_EINVAL (xyz lies outside the map's grid) and nothing changes.
 * MERGE(A, B).  Same grid bit for bit (voxel size and origin), same M, both with normals or both without: anything else is PCR_EINVAL.  A cell in
 *   one map keeps its rows bit for bit.  A cell in both gets A's members and then B's, cut at M.  MERGE IS NOT COMMUTATIVE: in a shared cell
 *   whose members add up past M, MERGE(A, B) keeps A's and drops B's tail, MERGE(B, A) the other way round.  It is associative.
 * INSERT(map, cloud, T) = MERGE(map, the map of the cloud at T on the map's grid with the map's M).  Consequence: inserting clouds one after
 *   another equals appending every point, in arrival order, to its cell's list while that list has fewer than M entries -- KISS-ICP's rule.
 * REMOVE_FAR(map, center c (float64 x3), max_distance r).  Per ROW: a row is kept iff d^2 < r^2 (strict), d^2 in float64 from the float32 point by
 *   differences, squares and sums in the order x, y, z, each rounded once, r^2 = r r (the arithmetic of the voxel covariance map's REMOVE_FAR).
 *   Kept rows keep their bits and their relative order; a cell left without rows disappears, a thinned one has room again.  A call that would
 *   leave no rows is PCR_EINVAL (would leave the map empty) and changes nothing.
 * ROW OF A SOURCE POINT AT T.  q as above, in float64 (it is NOT rounded to float32).  cell = floor((q - origin) / voxel_size).  Candidate cells:
 *   cell + offset for the neighbourhood 1, 7 or 27, the offsets of the voxelized GICP section (their order plays no part here).  Over all members of
 *   all candidate cells d^2 = ((q_x - p_x)^2 + (q_y - p_y)^2) + (q_z - p_z)^2 in float64 on the widened float32 member, every operation rounded
 *   once.  The match is the row with the smallest (d^2, row index); it is a correspondence iff d^2 < max_correspondence_distance^2 (strict, the
 *   square taken in float64).  At most one row (i, map row) per source point, ordered by i.
 *   EXACTNESS.  With neighbourhood 27 and max_correspondence_distance <= voxel_size the match is the nearest of ALL map rows within that
 *   distance, with the same tie rule: a row with |q - p| < voxel_size differs from q by less than a voxel on every axis, so its cell index
 *   differs from q's by at most one per axis, and it is a member of a candidate cell.  A larger distance is allowed and is simply the rule;
 *   neighbourhoods 1 and 7 are approximations by design.
 * UPDATE.  s = q, t and n the matched row widened to float64, w the kernel's weight as the multiway section states it (L2: 1, L1:
 *   1 / max(|r|, 1e-300), GM: k / (k + r^2)^2).
 *     PCR_EST_POINT_TO_PLANE   one row: r = ((s - t)_x n_x + (s - t)_y n_y) + (s - t)_z n_z, J = [s x n, n], weighted by w(r).  Needs a map
 *                              with normals (PCR_EINVAL names normals).
 *     PCR_EST_POINT_TO_POINT   three rows: r = s - t, J = [-skew(s) | I], all three weighted by w(|s - t|), |s - t| = sqrt(d^2).  This is
 *                              the Gauss-Newton form, which is what KISS-ICP runs, so the kernels apply.  It is NOT the Umeyama fit of
 *                              pcr_registration_icp: the two agree only in the limit of small updates.  with_scaling != 0 is PCR_EINVAL.
 *   The 6x6 system is solved and turned into a pose exactly as the point-to-plane update of pcr_registration_icp (LDLT, Rz Ry Rx,
 *   left-multiplied).  No rows: the identity.
 * LOOP.  RegistrationICP's, as in pcr_registration_icp: rows at init, then update / left-multiply / rows, until |d fitness| < relative_fitness
 *   and |d RMSE| < relative_rmse, or max_iteration.  fitness = rows / n_src, inlier_rmse = sqrt(sum d^2 / rows).
 * SUMS.  Float64, no floating-point atomics.  The source points are taken in caller order in tiles of 512; a tile's sum is a fixed tree over its
 *   points (three rows of a point in the order x, y, z) and the tiles are added in ascending order: the same bits on every run.
 * ESTIMATE(map, radius rho, min_neighbors k_min).  A third state of a map next to "has the caller's normals" and "has none": ESTIMATED normals, which
 *   the map computes from its own rows and keeps current by itself.  rho is finite and 0 < rho <= voxel_size; k_min >= 3.
 *   NEIGHBOURS OF ROW i.  p_i is the row's float32 point widened to float64; its cell is the row's own cell.  Candidates are the members of that
 *   cell and of its 26 neighbours; a candidate cell with an index outside [0, 2^21) on any axis does not exist (it is neither wrapped nor probed).
 *   Row j is a neighbour iff d^2 < rho^2 (strict), d^2 exactly the arithmetic of ROW OF A SOURCE POINT with q = p_i, rho^2 one float64 product.  Row
 *   i is its own neighbour.  count_i is the number of neighbours; by the EXACTNESS lemma they are ALL map rows within rho.
 *   COVARIANCE AND NORMAL.  e = p_j - p_i in float64 (exact for points this near, and the moments stay at the size of rho^2, not |p|^2).  The sums
 *   S_a = sum e_a and S_ab = sum e_a e_b (every product rounded once, then added) over the neighbours run in float64, uncontracted, in this order,
 *   which depends on the map's rows alone: the neighbours are split into eight shares by (rank of the member inside its cell) mod 8; a share is
 *   added up from zero in the order (candidate cell in the order {-1, 0, 1}^3 lexicographic with dx slowest, member rank ascending); the eight
 *   shares are added as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)).  C_ab = S_ab / count - (S_a / count)(S_b / count).  The rest is the rule of
 *   pcr_estimate_normals without a prior, with the same eigen solver: fewer than 3 neighbours give the identity covariance and so (0, 0, 1); the
 *   zero covariance gives (0, 0, 1) and a diagonal one the axis of its strictly smallest entry, else z; the output is rounded to float32.  There
 *   is NO sign rule: the point-to-plane row is invariant under n -> -n bit for bit.
 *   VALIDITY.  valid_i = count_i >= k_min.
 *   The normals and counts are a function of (rows, grid, rho, k_min) only: two maps with bit-equal rows on the same grid have bit-equal normals and
 *   equal counts, however they were reached.
 *   WHICH MAPS.  A map without normals, or an estimated one (estimated again with the new arguments).  A map with the caller's normals is
 *   PCR_EINVAL (names normals).
 *   GROWTH.  On an estimated map INSERT takes points only (normals != NULL is PCR_EINVAL).  MERGE(A, B) with A estimated takes a B without normals
 *   or an estimated one, whose normals are derived data and are not read; A without normals and B estimated gives a map without; B with the
 *   caller's normals is the mismatch it always was.  After INSERT, MERGE and REMOVE_FAR the whole new map is estimated again with the stored rho
 *   and k_min, inside the call and before the new block is swapped in: all or nothing like the rest, and on any error the rows, normals, counts
 *   and rule are exactly as before.
 *   USE.  pcr_point_map_correspondences is purely geometric and does not change.  With PCR_EST_POINT_TO_PLANE on an estimated map a match whose
 *   map row is not valid is NO ROW: it enters neither the 6x6 system nor rows, fitness, inlier_rmse, sum_d2, sum_r2, nor the correspondences of
 *   pcr_registration_point_map.  Point to point never reads validity: on an estimated map it returns the bits it returns on the same map without
 *   normals.  On a map with the caller's normals nothing changes.
 * All cloud and row buffers are DEVICE buffers.  The map lives in one device allocation of its own until it is destroyed; any context on the same
 * device may use it.  _insert, _merge, _remove_far and _estimate_normals change it, all or nothing and finished when they return: the new block with its cell hash is
 * built, swapped in, and the old one freed (which waits for the device); on any error the map is exactly as before.  While such a call runs no
 * other call may use the map, and map rows in an earlier correspondence set are stale afterwards (row indices change).
 * Every refusal is PCR_EINVAL with a message naming the argument: a non-finite value in xyz / normals / grid_min3 / T / center3 / src_xyz,
 * voxel_size <= 0, max_points_per_voxel outside 1 .. 64, a neighborhood that is not 1, 7 or 27, a max_correspondence_distance or max_distance
 * that is not finite or <= 0, a NULL map, a map on another device than the context, mismatched maps, normals given to a map without (or the
 * other way round, or to a map that estimates them), a radius that is not finite, <= 0 or above voxel_size, min_neighbors < 3, normal counts asked of a
 * map that is not estimated, an estimation that is null, of another kind, with scaling, or with no kernel of pcr_loss_kind. */
typedef struct pcr_point_map pcr_point_map;
typedef struct {
    pcr_estimation estimation;   /* kind: PCR_EST_POINT_TO_POINT or PCR_EST_POINT_TO_PLANE; loss, loss_k: the robust kernel of either; epsilon is not read */
    double relative_fitness;
    double relative_rmse;
    int32_t max_iteration;
    int32_t neighborhood;        /* 1, 7 or 27 candidate cells per source point */
} pcr_point_map_params;
/* MAP on the grid of the cloud's own minimum; normals optional (n x 3 float32).  Finished when it returns. */
int pcr_point_map_create(pcr_context *ctx, const float *xyz, const float *normals, int64_t n, double voxel_size, int max_points_per_voxel, pcr_point_map **out);
/* MAP ON A GRID, AT A POSE (T optional).  Finished when it returns. */
int pcr_point_map_create_on_grid(pcr_context *ctx, const float *xyz, const float *normals, int64_t n, double voxel_size, int max_points_per_voxel,
                                 const double *grid_min3, const double *T, pcr_point_map **out);
/* Frees the map (waits for the device, so no call is still reading it).  NULL is allowed. */
int pcr_point_map_destroy(pcr_point_map *map);
/* rows and occupied cells, each output optional (host) */
int pcr_point_map_size(const pcr_point_map *map, int64_t *rows, int64_t *cells);
/* each output optional (device): the cell table in Morton order -- cell3 (cells x 3 int32: ix, iy, iz), first_row (cells int32), count (cells
 * int32) -- and the rows -- xyz (rows x 3 float32), normals (rows x 3 float32; PCR_EINVAL on a map without).  Asynchronous on the context's stream. */
int pcr_point_map_read(pcr_context *ctx, const pcr_point_map *map, int32_t *cell3, int32_t *first_row, int32_t *count, float *xyz, float *normals);
/* the grid and the rule of a map, each output optional (host): grid_min3, origin3 = grid_min3 - voxel_size / 2, voxel_size, M, whether it has normals
 * (the caller's or estimated ones) */
int pcr_point_map_grid(const pcr_point_map *map, double *grid_min3, double *origin3, double *voxel_size, int *max_points_per_voxel, int *has_normals);
/* map <- INSERT(map, cloud, T); T optional; normals exactly when the map has the caller's normals (NULL for an estimated map). */
int pcr_point_map_insert(pcr_context *ctx, pcr_point_map *map, const float *xyz, const float *normals, int64_t n, const double *T);
/* map <- MERGE(map, other); other is unchanged and must not be the map itself. */
int pcr_point_map_merge(pcr_context *ctx, pcr_point_map *map, const pcr_point_map *other);
/* map <- REMOVE_FAR(map, center3, max_distance); *removed (optional, host) = rows dropped. */
int pcr_point_map_remove_far(pcr_context *ctx, pcr_point_map *map, const double *center3, double max_distance, int64_t *removed);
/* map <- ESTIMATE(map, radius, min_neighbors); *valid_rows (optional, host) = the rows with count >= min_neighbors.  Finished when it returns. */
int pcr_point_map_estimate_normals(pcr_context *ctx, pcr_point_map *map, double radius, int min_neighbors, int64_t *valid_rows);
/* count_i of every row of an estimated map: counts = device int32, one entry per row.  Asynchronous on the context's stream. */
int pcr_point_map_read_normal_counts(pcr_context *ctx, const pcr_point_map *map, int32_t *counts);
/* the normal rule of a map, each output optional (host): whether it is estimated, and then rho and k_min (0 otherwise) */
int pcr_point_map_normal_rule(const pcr_point_map *map, int *estimated, double *radius, int *min_neighbors);
/* the rows (i, map row) at the pose T: rows2 = int32 pairs, capacity n_src rows; *n_rows on the host. */
int pcr_point_map_correspondences(pcr_context *ctx, const pcr_point_map *map, const float *src_xyz, int64_t n_src, const double *T,
                                  double max_correspondence_distance, int neighborhood, int32_t *rows2, int64_t *n_rows);
/* UPDATE's sums at the pose T in ONE launch of the iteration kernel, all outputs on the host and each optional: JTJ (36, the full symmetric
 * matrix), JTr (6), *rows, *sum_d2, *sum_r2 (point to plane: sum of r^2; point to point: sum of |s - t|^2). */
int pcr_point_map_linearize(pcr_context *ctx, const pcr_point_map *map, const float *src_xyz, int64_t n_src, const double *T, double max_correspondence_distance,
                            int neighborhood, const pcr_estimation *estimation, double *JTJ, double *JTr, int64_t *rows, double *sum_d2, double *sum_r2);
/* the loop of the rule from init_T.  max_iteration < 0 is PCR_EINVAL.  A source without any row is no error: the pose stays init_T, fitness 0.
 * correspondences: optional device int32, capacity n_src rows: the rows at the returned pose (n_correspondences of them). */
int pcr_registration_point_map(pcr_context *ctx, const float *src_xyz, int64_t n_src, const pcr_point_map *map, double max_correspondence_distance,
                               const double *init_T, const pcr_point_map_params *params, pcr_result *result, int32_t *correspondences);

/* ============================================================================================ continuous time
 * A spinning LiDAR on a moving platform does not produce a rigid cloud: every point is measured at its own time, from its own pose.  A cloud may
 * carry one time per point; pcr_deskew moves every point by the fraction of a KNOWN relative motion that belongs to its time (KISS-ICP, Vizzo et
 * al. 2023), and pcr_point_map_linearize_continuous linearises a registration that ESTIMATES a begin pose and an end pose of the sweep, every point
 * placed at the pose interpolated at its own time (CT-ICP, Dellenbach et al. 2022), on the voxel point map above.  This statement is the
 * specification (tests/continuous_time_reference.py restates it in numpy on top of tests/point_map_reference.py).  Open3D has no such call.  The
 * rule is written from the papers' descriptions; NOBODY HAS COMPARED IT WITH KISS-ICP'S OR CT-ICP'S CODE.
 *   TIMES.  One float32 per point.  alpha_i = (time_i - t0) / (t1 - t0) in float64 on the widened float32, with t0 < t1 finite doubles (the Python
 *   layer defaults them to the cloud's minimum and maximum time).  alpha is NOT clamped: a time outside [t0, t1] extrapolates.  t1 <= t0 is
 *   PCR_EINVAL (names t1), a non-finite time PCR_EINVAL (names times / src_times).
 *   POSE AT alpha.  T_b = (R_b, t_b) and T_e = (R_e, t_e) are float64 4x4, row-major.  phi = Log(R_b^T R_e) is the rotation vector with its
 *   angle in [0, pi], computed ONCE per call on the host side of the C call, in float64.  R(alpha) = R_b E(alpha phi), a 3x3 product with every
 *   entry (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j, and t(alpha) = t_b + alpha (t_e - t_b): T_b == T_e gives t_b exactly.
 *   E(v) = I + A [v]x + B [v]x^2 with theta^2 = (x x + y y) + z z and theta its root: for theta >= 1e-4 A = sin(theta) / theta and
 *   B = (1 - cos(theta)) / theta^2; below that A = 1 - theta^2 / 6 and B = 1/2 - theta^2 / 24 (the truncation is below 1e-18); theta == 0
 *   gives I exactly.  The diagonal is 1 - B (y y + z z) and so on, an off-diagonal entry B x y -+ A z.
 *   q_i = R(alpha_i) p_i + t(alpha_i) in float64 by the ROWS expression of the voxel maps, ((r0 x + r1 y) + r2 z) + t, uncontracted; q_i is not
 *   rounded to float32.  u_i = (r0 x + r1 y) + r2 z, the sum before t is added, is the ROTATED POINT.
 *   DESKEW(cloud, D, alpha_ref).  D = T_b^-1 T_e is the relative motion over the sweep; the model is applied with T_b = I and T_e = D (R(alpha) is
 *   then E(alpha phi) itself).  With tau = t_D:  p'_i = float32( R(alpha_ref)^T ( (u_i + alpha_i tau) - alpha_ref tau ) ), the transposed product
 *   entry by entry (r_0d w_0 + r_1d w_1) + r_2d w_2 -- the point in the sensor frame at alpha_ref.  alpha_ref = 1, the end of the sweep, is the
 *   Python layer's default, so that the pose a registration then finds is the END pose (KISS-ICP's earlier releases used 0.5).  A normal becomes
 *   float32(R(alpha_ref)^T R(alpha_i) n), not normalised.  Times and colours are carried unchanged by the Python layer; COVARIANCES ARE NOT
 *   CARRIED (the deskewed cloud has none).  D = I returns the input values: theta == 0 and tau == 0 make every term exact.
 *   ROW.  The match of q_i is the ROW rule of the voxel point map, unchanged: the neighbourhood 1 / 7 / 27, the order (float64 d^2, row), the
 *   strict < max_correspondence_distance^2, and, for point to plane on an estimated map, the validity of the matched row.
 *   UPDATE.  With m and n the matched row and w the kernels of the UPDATE rule above:  point to plane, one row, r = ((q - m) . n) grouped as
 *   there, J6 = [u x n, n];  point to point, three rows, r = q - m, J6 = [-skew(u) | I], all weighted by w(|q - m|).  u stands here instead of
 *   the world point s of the rigid estimators, because the STEP below adds to the translations and does not left-multiply the pose.  The
 *   12-column row is J12 = [(1 - alpha) J6, alpha J6], and the outputs are H = sum w J12^T J12 (12x12, the full symmetric matrix),
 *   g = sum w J12^T r (12), rows, sum_d2, sum_r2.  A point's terms are the 27 rigid values (upper w J6^T J6, w J6^T r) times (1 - alpha)^2,
 *   alpha (1 - alpha), alpha^2 resp. (1 - alpha), alpha.
 *   LIMITATION.  The rotation columns are FIRST ORDER in the rotation between the two poses: they are exact when phi = 0, and otherwise the usual
 *   linear interpolation of the two increments (the exact slerp Jacobian is not built).  A zero-residual fixed point stays where it is.
 *   SUMS.  The SUMS rule of the point map: no floating-point atomics; source points in caller order in tiles of 512; a fixed tree inside a tile
 *   (the pairs (l, l ^ 1), ^ 2, ^ 4, ^ 8 inside 16 consecutive points, then the 32 groups of 16 in ascending order); tiles added in ascending
 *   order.  The same bits on every run.
 *   STEP (host, float64; the Python layer).  delta = -(H + P)^-1 (g + p) by a Cholesky solve; a failed factorisation or a non-finite delta is no
 *   error: the identity update, which ends the loop.  R_b <- E(delta[0:3]) R_b, t_b <- t_b + delta[3:6], R_e <- E(delta[6:9]) R_e,
 *   t_e <- t_e + delta[9:12].  begin = "fixed" solves the lower-right 6x6 block alone and leaves T_b bit for bit; begin = "free" solves all
 *   twelve, with an optional prior (w_rot, w_trans) around the T_begin the call was given: rows w_rot I3 and rows w_trans I3 on the begin
 *   block's diagonal, rows w_rot Log(R_b R_p^T) and rows w_trans (t_b - t_p) on g.
 *   LOOP.  RegistrationICP's loop on the host: sums at the start poses, then step / sums until |d fitness| < relative_fitness and |d RMSE| <
 *   relative_rmse, or max_iteration; fitness = rows / n_src, inlier_rmse = sqrt(sum_d2 / rows).  One iteration is one launch and one read-back
 *   of 160 doubles.
 * Every refusal is PCR_EINVAL with a message naming the argument: NULL or non-finite times, t1 <= t0 or a non-finite t0 / t1 / alpha_ref, a pose
 * that is NULL, holds a non-finite value or whose last row is not 0 0 0 1, and every refusal of pcr_point_map_linearize. */
/* DESKEW: xyz, normals (optional), times, out_xyz and out_normals (exactly when normals is given) are device buffers of n rows; motion16 = D
 * (host).  out_xyz may be xyz.  Asynchronous on the context's stream. */
int pcr_deskew(pcr_context *ctx, const float *xyz, const float *normals, const float *times, int64_t n, const double *motion16, double t0, double t1, double alpha_ref,
               float *out_xyz, float *out_normals);
/* UPDATE's sums at the poses (T_begin16, T_end16) in ONE launch, all outputs on the host and each optional: H144 (the full symmetric 12x12 matrix,
 * begin columns first), g12, *rows, *sum_d2, *sum_r2; matches: optional DEVICE int32, one map row or -1 per source point. */
int pcr_point_map_linearize_continuous(pcr_context *ctx, const pcr_point_map *map, const float *src_xyz, const float *src_times, int64_t n_src, const double *T_begin16,
                                       const double *T_end16, double t0, double t1, double max_correspondence_distance, int neighborhood, const pcr_estimation *estimation,
                                       double *H144, double *g12, int64_t *rows, double *sum_d2, double *sum_r2, int32_t *matches);

/* ---- measurement hooks (bench.py): no reference counterpart -------------------------- */
/* While enabled, pcr_multiscale_gicp / pcr_registration_generalized_icp bracket every chunk of GICP-iteration
 * launches with HIP events on the context stream and the kernel stamps itself with s_memrealtime.
 * out16 = { [0] ms of HIP-event time over chunks whose launches were all live, [1] launches in those chunks,
 *           [2] us of in-kernel time summed over live launches, [3] live launches,
 *           [4] algorithmic bytes of the live launches (48 B x source points), [5] launches issued, [6], [7] diagnostics,
 *           [8] ms of HIP-event time over the feature-matching kernels of registro_FGR, [9] their algorithmic flops
 *           (2 * 33 * Ns * Nt per direction), [10] launches, [11] GICP queries whose skip certificate did not hold (searched again),
 *           summed over the launches after the first of every scale, rest 0 } */
int pcr_profile_enable(pcr_context *ctx, int on);
int pcr_profile_read(pcr_context *ctx, double *out16, int reset);

/* ---- test hooks (exercised by tests/ only) ----------------------------------------- */
/* exact k nearest neighbours of every point of a cloud (self included), through the same index the
 * pipeline uses. idx: n x k int32, d2: n x k float32 (device), rows sorted ascending.              */
int pcr_debug_knn(pcr_context *ctx, const float *xyz, int64_t n, int k, double radius, int32_t *idx, float *d2,
                  int32_t *counts);
/* the Hybrid(radius, k) neighbour lists of FPFH (k in 1..200, radius > 0) of `count` clouds (xyz[c]: n[c] x 3 float32, device).  count = 1
 * takes the path of pcr_compute_fpfh_feature, count > 1 (at most 64) the one of the lockstep registro_FGR groups.  idx[c]: n[c] x k int32
 * (device), row i = caller point i, entries caller indices, -1 = none; cnt[c]: n[c] int32 (device), the entries of the row, or -1 for a row
 * in the k-best kernel's slot layout (scan all k slots).  A ball of more than k points lists its k nearest by (float64 d^2, caller index). */
int pcr_debug_radius_lists(pcr_context *ctx, int count, const float *const *xyz, const int64_t *n, int k, double radius,
                           int32_t *const *idx, int32_t *const *cnt);
/* the voxel grids of `count` clouds (xyz[c], optional attr[c]: n[c] x 3 float32, device; n[c] > 0) at n_scales voxel sizes (1..8), through the
 * form of the voxel pass that `form` names: 0 the one-scale pass, cloud by cloud and scale by scale (pcr_voxel_down_sample); 1 all scales of a
 * cloud in one key / sort / scan / mean pass, cloud by cloud (pcr_multiscale_gicp); 2 all clouds and scales in one pass (the lockstep groups of
 * pcr_register_pairs_plan; count <= 64).  Bounds are taken as those paths take them.  out_xyz[c * n_scales + s] (and out_attr[...] when attr is
 * given): n[c] x 3 float32 (device), the packed rows of cloud c at scale s in the pass's own (Morton) order; out_n[c * n_scales + s] (host): the
 * rows.  *taken (host) = 0 when a merged form declines (fewer than two scales, or the scale index does not fit above the Morton bits of some
 * cloud): nothing is written then.                                                                                                          */
int pcr_debug_voxel_grids(pcr_context *ctx, int count, const float *const *xyz, const float *const *attr, const int64_t *n, const double *voxels,
                          int n_scales, int form, float *const *out_xyz, float *const *out_attr, int32_t *out_n, int *taken);
/* the scale clouds the GICP loops of pcr_multiscale_gicp / pcr_register_pairs_plan consume -- voxel grid, outlier filter (sor_k, sor_std), normals of
 * the CLEANED cloud (normal_k nearest kept points) oriented by the voxel means of `normals` -- of `count` clouds (xyz[c], optional normals[c]:
 * n[c] x 3 float32, device; normals itself or single entries may be null; n[c] > 0; count <= 64) at n_scales voxel sizes (1..8).  Cloud c is
 * prepared as a GICP source for even c and as a target (with its search tree) for odd c, as the lockstep groups number their clouds.  The code
 * that runs is the product's own preparation, picked by `form`:
 *   0  scale by scale after the merged voxel pass (the path pcr_multiscale_gicp takes when the batched one declines; any sor_k, normal_k);
 *   1  all scales of a cloud in one set of batched launches, cloud by cloud (pcr_multiscale_gicp's first choice);
 *   2  all clouds and scales as one batch (the lockstep groups of pcr_register_pairs_plan; count x n_scales <= 256).
 * Outputs, problem k = c * n_scales + s: out_xyz[k], out_normals[k] (device, caller buffers of n[c] x 3 float32): the cleaned points and their
 * normals, row for row in the order the GICP loop receives them (the Morton order of the voxel grid, outliers removed); out_n_voxel[k],
 * out_n_clean[k] (host): the rows of the voxel cloud and of the cleaned cloud (the rows written).  Finished when it returns.
 * Returns PCR_DECLINED (1), having written nothing, when forms 1 / 2 do not serve the inputs -- exactly where the product falls back to the next
 * path: sor_k > 32, normal_k > 32, fewer than 2 scales, or the merged voxel pass declining (pcr_debug_voxel_grids).  Form 0 never declines. */
int pcr_debug_scale_clouds(pcr_context *ctx, int count, const float *const *xyz, const float *const *normals, const int64_t *n, const double *voxels,
                           int n_scales, int sor_k, double sor_std, int normal_k, int form, float *const *out_xyz, float *const *out_normals,
                           int32_t *out_n_voxel, int32_t *out_n_clean);
/* one GICP linearisation at pose T: search + A.6 sums. JTJ36, JTr6, stats3 = {count, sum d^2, sum r^2} (host) */
int pcr_debug_gicp_linearize(pcr_context *ctx, const float *src_xyz, const float *src_normals, int64_t n_src,
                             const float *tgt_xyz, const float *tgt_normals, int64_t n_tgt, double max_dist,
                             const double *T, const pcr_gicp_params *params, double *JTJ36, double *JTr6,
                             double *stats3, int32_t *match /* device n_src, optional */);

/* the mutual nearest-feature search of registro_FGR alone (33-D float32 rows, device): out_1to0[j] = row of f0 nearest to row j of f1,
 * out_0to1 likewise.  mode 0: f16-split MFMA screen + exact float64 re-check (production; with tile pruning from ~70k rows per side),
 * 1: all-pairs float64 MFMA, 2: float32 brute force, 3 / 4: the screen with tile pruning forced on / off */
int pcr_debug_feature_nn(pcr_context *ctx, const float *f0, int64_t n0, const float *f1, int64_t n1, int32_t *out_1to0, int32_t *out_0to1, int mode);

/* what the RANSAC kernels compute for iterations [first, first + count) of pcr_registration_ransac_correspondence with these arguments, no early
 * stop (max_iteration and confidence are not read).  All four outputs are device arrays: valid_out count bytes, T_out count x 16 float64 (zeros above
 * the last row when the sample failed the edge-length check: no fit was made), inliers_out count int32 (-1: invalid), err2_out count float64. */
int pcr_debug_ransac_hypotheses(pcr_context *ctx, const float *src_xyz, const float *src_normals, int64_t n_src, const float *tgt_xyz, const float *tgt_normals,
                                int64_t n_tgt, const int32_t *corres, int64_t n_corres, double max_distance, const pcr_ransac_params *params, int64_t first,
                                int64_t count, uint8_t *valid_out, double *T_out, int32_t *inliers_out, double *err2_out);

/* what the SC2 kernels compute for the seeds of pcr_registration_sc2_correspondence with these arguments, in the order of the seeds (refine_iterations
 * is checked, not used).  *n_seeds (host) = the number of seeds; the other outputs are device arrays with room for min(max(1, (int64)(seed_ratio *
 * n_corres)), max_seeds) seeds: seed_rows int32 (the seed's row), k1_rows and k2_rows int32 x 64 per seed (the rows of K1 and of K2 in their order,
 * the seed first, -1 beyond the members), T_out 16 float64 per seed (zeros above the last row for an invalid seed), valid_out bytes, inliers_out
 * int32 (-1: invalid), err2_out float64.  Fewer than 3 rows: PCR_EINVAL. */
int pcr_debug_sc2_seeds(pcr_context *ctx, const float *src_xyz, int64_t n_src, const float *tgt_xyz, int64_t n_tgt, const int32_t *corres, int64_t n_corres,
                        const pcr_sc2_option *option, int64_t *n_seeds, int32_t *seed_rows, int32_t *k1_rows, int32_t *k2_rows, double *T_out, uint8_t *valid_out,
                        int32_t *inliers_out, double *err2_out);

/* what the plane kernels compute for iterations [first, first + count) of pcr_segment_plane with these arguments, no early stop (num_iterations and
 * probability are checked, not used).  All four outputs are device arrays: valid_out count bytes, plane_out count x 4 float64 (zeros for an
 * invalid hypothesis), inliers_out count int32 (-1: invalid), err_out count float64 (the sum of the inlier distances). */
int pcr_debug_plane_hypotheses(pcr_context *ctx, const float *xyz, int64_t n, double distance_threshold, const pcr_plane_params *params, int64_t first,
                               int64_t count, uint8_t *valid_out, double *plane_out, int32_t *inliers_out, double *err_out);

/* test / diagnostic switches of the process (no reference equivalent).  Each one is latched from the environment variable of the same
 * name in upper case with the PCR_ prefix when the library first needs it; this call overrides it afterwards without touching the
 * environment (worker threads read an atomic, never getenv).  "knn_wave": -1 by size and call form (default), 0 the octet k-NN kernel,
 * 1 the one-query-per-lane kernel for every search that fits it; "knnw_budget": candidate batches a wavefront of that kernel takes before
 * it hands its queries over; "fence_prep": measurement only -- with profiling on, every scale's GICP loop of the pipelined multiscale path
 * (clouds the batched preprocessing declines: config 5) starts after ALL preprocessing enqueued so far has finished, so that HIP-event times
 * per launch are the iteration kernels' own; "icp_verify": diagnostics of the GICP loop (re-search of certified queries).
 * Switches between two forms of the FGR half that give the same bits (tests compare them): "spfh_float64" (0: pair features of FPFH decided in
 * float where float can and in float64 otherwise, for clouds from 60 000 points; 1: all in float64; 2: both, a disagreement is an error; 4: the
 * float pass whatever the size; 3: as 4 with a 16-entry queue, the overflow path), "radius_list_select" (1: overfull Hybrid(r, max_nn) balls finished by threshold selection; 0: by the k-best kernel),
 * "featnn_mutual" (1: the second direction of the feature search inside FGR runs only for the rows the first direction points at, under the
 * bound it found; 0: both directions in full), "icp_scales" (1: in lockstep groups of small clouds every pair goes through its scales by itself;
 * 0: one lockstep loop per scale), "search_sort_queries" (-1: a k-nearest or hybrid search of an index takes a large batch of queries -- 131072 or more with k in
 * 9..64, 32768 or more with k above 64 -- in the Morton order of the queries, every other search in the caller's order; 0: always in the caller's
 * order; 1: always in Morton order), "fps_form" (-1: pcr_farthest_point_sample picks its form by size; 0: one launch per step; 1: the persistent launch), "fps_wgs"
 * (0: the persistent workgroups by size; else that many, at most one per compute unit and 256), "fps_timeout" (ticks of the 100 MHz wall clock
 * a persistent workgroup waits at its barrier before the call falls back to the step form; -1: the default, that of PCR_FGR_MULTI_TIMEOUT;
 * 0 forces the fall-back), "nfl_form" (the kernel that turns the outlier filter's lists into the normals of the cleaned cloud -- 1, the default:
 * one point per lane; 0: eight lanes per point in eight rounds, the reference form).  "arena_poison": the scratch arena is filled with this byte before every call (a read of
 * scratch nobody wrote then follows the pattern).  Returns PCR_EINVAL for an unknown name. */
int pcr_set_option(const char *name, long long value);
/* Process-wide event counters (value, or -1 for an unknown name; reset != 0 clears it): how often a lockstep registro_FGR group fell back to
 * the one-pair path for one of its pairs -- "fgr_group_barrier_timeouts" (the co-resident optimiser workgroups of the group did not all get a
 * slot in time), "fgr_group_pool_overflows" (record pool of the feature screen), "fgr_group_pairs_redone_alone" (all causes).  The results are
 * the same bits either way; the throughput is not (bench.py prints them next to the NCLT stages). */
long long pcr_counter(const char *name, int reset);

#ifdef __cplusplus
}
#endif
#endif
