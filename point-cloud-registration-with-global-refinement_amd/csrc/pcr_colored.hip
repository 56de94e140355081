// pcr_colored.hip -- what colored ICP (registration_colored_icp with TransformationEstimationForColoredICP; Park, Zhou, Koltun, ICCV 2017) adds
// to the library besides its iteration kernel (k_icp_iter_colored, pcr_gicp.hip, next to the loop it shares): the specification is the
// statement in include/pcr_hip.h.
//   k_color_intensity  I = (r + g + b) / 3 in float64 of every point, gathered into the cloud's Morton order
//   k_color_gradient   one lane per point over its exact k-best / hybrid neighbour list (pcr_dev_knn_debug: the search of estimate_normals and
//                      FPFH): the list is put into the k-d tree's order (float64 d^2, caller index) in LDS, the 6 + 3 moments of A^T A, A^T b are
//                      summed in that order in float64 centred on the point, and the 3x3 system is solved by a pivoted LDLT in registers
// and the three entry points: pcr_color_gradient, pcr_registration_colored_icp, pcr_voxel_down_sample_ex.
// Floating-point contraction per source expression only, as in pcr_gicp.hip.
#pragma clang fp contract(on)
#include <cmath>
#include <cstring>
#include "pcr_internal.h"

#define CG_BS 64              // one wavefront per workgroup: the sorted lists of its 64 points take CG_KMAX x 64 x 12 B = 24 KB of LDS
#define CG_KMAX 32

__global__ void __launch_bounds__(256) k_color_intensity(const float *__restrict__ colors, const uint32_t *__restrict__ perm, int n, double *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t v = perm ? perm[i] : (uint32_t)i;
    out[i] = ((double)colors[v * 3] + (double)colors[v * 3 + 1] + (double)colors[v * 3 + 2]) / 3.0;
}

struct ColorGradArgs {
    const float4 *pts, *nrm;         // Morton order
    const double *inten;
    const uint32_t *perm;            // sorted -> caller index (the tie order of the list)
    const int *n_ptr;
    const int32_t *lidx; int k;      // rows of k sorted-cloud indices, in any order, -1 = empty slot
    double r2;                       // float64 radius test of the hybrid search (1e300: none)
    float4 *grad;
};

// x = A^-1 b for the symmetric 3x3 A = (a00 a01 a02; . a11 a12; . . a22) by LDL^T with diagonal pivoting (the largest remaining diagonal entry,
// the earlier one on a tie); a zero pivot leaves its component 0
__device__ static inline void cg_ldlt3(double a00, double a01, double a02, double a11, double a12, double a22, double b0, double b1, double b2, double *x) {
    const int p0 = (fabs(a11) > fabs(a00) && fabs(a11) >= fabs(a22)) ? 1 : (fabs(a22) > fabs(a00) ? 2 : 0);
    double t;
    if (p0 == 1) { t = a00; a00 = a11; a11 = t; t = a02; a02 = a12; a12 = t; t = b0; b0 = b1; b1 = t; }
    if (p0 == 2) { t = a00; a00 = a22; a22 = t; t = a01; a01 = a12; a12 = t; t = b0; b0 = b2; b2 = t; }
    const double i0 = a00 != 0.0 ? 1.0 / a00 : 0.0;
    double l1 = a01 * i0, l2 = a02 * i0;
    double s11 = a11 - l1 * a01, s12 = a12 - l1 * a02, s22 = a22 - l2 * a02;
    const bool p1 = fabs(s22) > fabs(s11);
    if (p1) { t = s11; s11 = s22; s22 = t; t = l1; l1 = l2; l2 = t; t = b1; b1 = b2; b2 = t; }
    const double i1 = s11 != 0.0 ? 1.0 / s11 : 0.0;
    const double l21 = s12 * i1;
    const double d2 = s22 - l21 * s12;
    const double i2 = d2 != 0.0 ? 1.0 / d2 : 0.0;
    const double y0 = b0, y1 = b1 - l1 * y0, y2 = b2 - l2 * y0 - l21 * y1;
    double x2 = y2 * i2;
    double x1 = y1 * i1 - l21 * x2;
    double x0 = y0 * i0 - l1 * x1 - l2 * x2;
    if (p1) { t = x1; x1 = x2; x2 = t; }
    if (p0 == 1) { t = x0; x0 = x1; x1 = t; }
    if (p0 == 2) { t = x0; x0 = x2; x2 = t; }
    x[0] = x0; x[1] = x1; x[2] = x2;
}

__global__ void __launch_bounds__(CG_BS) k_color_gradient(ColorGradArgs a) {
    __shared__ double sd[CG_KMAX][CG_BS];          // entry j of lane t at [j][t]: consecutive lanes, consecutive banks
    __shared__ int si[CG_KMAX][CG_BS];
    const int n = *a.n_ptr;
    const int i = blockIdx.x * CG_BS + threadIdx.x, t = threadIdx.x;
    if (i >= n) return;
    const float4 pf = a.pts[i], nf = a.nrm[i];
    const double px = pf.x, py = pf.y, pz = pf.z, nx = nf.x, ny = nf.y, nz = nf.z;
    // ---- the list in the k-d tree's order: insertion by (float64 d^2, caller index)
    int nn = 0;
    for (int s = 0; s < a.k; s++) {
        const int id = a.lidx[(size_t)i * a.k + s];
        if (id < 0 || id >= n) continue;
        const float4 q = a.pts[id];
        const double dx = (double)q.x - px, dy = (double)q.y - py, dz = (double)q.z - pz;
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (!(d2 < a.r2)) continue;
        int j = nn;
        while (j > 0) {
            const double dj = sd[j - 1][t];
            if (dj < d2 || (dj == d2 && a.perm[si[j - 1][t]] < a.perm[id])) break;
            sd[j][t] = dj; si[j][t] = si[j - 1][t];
            j--;
        }
        sd[j][t] = d2; si[j][t] = id;
        nn++;
    }
    double g[3] = {0.0, 0.0, 0.0};
    if (nn >= 4) {
        const double ip = a.inten[i];
        double m00 = 0, m01 = 0, m02 = 0, m11 = 0, m12 = 0, m22 = 0, b0 = 0, b1 = 0, b2 = 0;
        for (int j = 1; j < nn; j++) {                  // (the first entry is the point itself)
            const int id = si[j][t];
            const float4 q = a.pts[id];
            const double vx = (double)q.x - px, vy = (double)q.y - py, vz = (double)q.z - pz;
            const double vn = vx * nx + vy * ny + vz * nz;
            const double ax = vx - vn * nx, ay = vy - vn * ny, az = vz - vn * nz;      // q' - p, q' = q - ((q - p).n) n
            const double db = a.inten[id] - ip;
            m00 += ax * ax; m01 += ax * ay; m02 += ax * az; m11 += ay * ay; m12 += ay * az; m22 += az * az;
            b0 += ax * db; b1 += ay * db; b2 += az * db;
        }
        const double w = (double)(nn - 1), w2 = w * w;     // the last row, (nn - 1) n with b = 0
        m00 += w2 * (nx * nx); m01 += w2 * (nx * ny); m02 += w2 * (nx * nz); m11 += w2 * (ny * ny); m12 += w2 * (ny * nz); m22 += w2 * (nz * nz);
        cg_ldlt3(m00, m01, m02, m11, m12, m22, b0, b1, b2, g);
    }
    a.grad[i] = make_float4((float)g[0], (float)g[1], (float)g[2], 0.0f);
}

// colours of a caller cloud -> float64 intensities in the Morton order of its imported copy
static int color_intensities(pcr_context *ctx, const float *colors, const uint32_t *perm, int64_t n, double *out) {
    if (n <= 0) return PCR_OK;
    PCR_LAUNCH(ctx, k_color_intensity, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, colors, perm, (int)n, out);
    return PCR_OK;
}

// gradients of an imported cloud (normals and tree in place), Morton order; the neighbour lists live in the arena for the call
static int color_gradient(pcr_context *ctx, const DevCloud *c, const uint32_t *perm, const double *inten, int search_kind, int knn, double radius, float4 *grad) {
    if (search_kind != PCR_SEARCH_KNN && search_kind != PCR_SEARCH_HYBRID) { ctx->err = "colour gradient: KNN or Hybrid search"; return PCR_EINVAL; }
    if (knn < 1 || knn > CG_KMAX) { ctx->err = "colour gradient: knn outside 1..32"; return PCR_EINVAL; }
    const bool hybrid = search_kind == PCR_SEARCH_HYBRID;
    if (hybrid && !(radius > 0.0)) { ctx->err = "radius <= 0"; return PCR_EINVAL; }
    if (c->cap <= 0) return PCR_OK;
    ArenaMark mark(ctx);
    int32_t *idx = arena<int32_t>(ctx, (size_t)c->cap * knn);
    float *d2 = arena<float>(ctx, (size_t)c->cap * knn);
    int32_t *cnt = arena<int32_t>(ctx, c->cap);
    if (!idx || !d2 || !cnt) return PCR_ENOMEM;
    PCR_TRY(pcr_dev_knn_debug(ctx, c, knn, hybrid ? radius : 0.0, idx, d2, cnt));
    ColorGradArgs a;
    a.pts = c->pts; a.nrm = c->nrm; a.inten = inten; a.perm = perm; a.n_ptr = c->n; a.lidx = idx; a.k = knn;
    a.r2 = hybrid ? radius * radius : 1e300; a.grad = grad;
    PCR_LAUNCH(ctx, k_color_gradient, dim3((unsigned)((c->cap + CG_BS - 1) / CG_BS)), dim3(CG_BS), 0, ctx->stream, a);
    return PCR_OK;
}

static size_t color_list_bytes(int64_t n, int knn) { return (size_t)(n > 0 ? n : 1) * ((size_t)knn * 8 + 64) + (1u << 20); }

extern "C" int pcr_color_gradient(pcr_context *ctx, const float *xyz, const float *normals, const float *colors, int64_t n, int search_kind, int knn,
                                  double radius, float *gradient3) {
    return pcr_api_call(ctx, [&]() -> int {
    if (n < 0 || (n > 0 && (!xyz || !gradient3))) return PCR_EINVAL;
    if (n > 0 && !normals) { ctx->err = "colour gradient: the cloud has no normals"; return PCR_EINVAL; }
    if (n > 0 && !colors) { ctx->err = "colour gradient: the cloud has no colours"; return PCR_EINVAL; }
    if (n == 0) return PCR_OK;
    PCR_TRY(pcr_arena_reserve(ctx, pcr_scratch_bytes_for(n) + color_list_bytes(n, knn > 0 ? knn : 1) + (size_t)n * 24));
    DevCloud c; uint32_t *perm = nullptr;
    PCR_TRY(pcr_import_cloud(ctx, xyz, normals, n, &c, &perm, true));
    double *inten = arena<double>(ctx, n);
    float4 *grad = arena<float4>(ctx, n);
    if (!inten || !grad) return PCR_ENOMEM;
    PCR_TRY(color_intensities(ctx, colors, perm, n, inten));
    PCR_TRY(color_gradient(ctx, &c, perm, inten, search_kind, knn, radius, grad));
    return pcr_dev_scatter_rows_f4_to_f3(ctx, grad, perm, c.n, c.cap, gradient3);      // no scalar output: asynchronous on the context's stream
    });
}

extern "C" int pcr_registration_colored_icp(pcr_context *ctx, const float *src_xyz, const float *src_colors, int64_t n_src, const float *tgt_xyz,
                                            const float *tgt_normals, const float *tgt_colors, int64_t n_tgt, double max_dist, const double *init_T,
                                            const pcr_colored_icp_params *params, pcr_result *result, int32_t *correspondences) {
    return pcr_api_call(ctx, [&]() -> int {
    if (!params || !result || !init_T || n_src < 0 || n_tgt < 0) return PCR_EINVAL;
    if (!(max_dist > 0.0)) { ctx->err = "max_correspondence_distance <= 0"; return PCR_EINVAL; }
    if (n_tgt > 0 && !tgt_normals) { ctx->err = "colored ICP requires normals on the target"; return PCR_EINVAL; }
    if (n_src > 0 && !src_colors) { ctx->err = "colored ICP requires colours on the source"; return PCR_EINVAL; }
    if (n_tgt > 0 && !tgt_colors) { ctx->err = "colored ICP requires colours on the target"; return PCR_EINVAL; }
    if ((n_src > 0 && !src_xyz) || (n_tgt > 0 && !tgt_xyz)) { ctx->err = "missing cloud"; return PCR_EINVAL; }
    for (int k = 0; k < 16; k++) if (!std::isfinite(init_T[k])) { ctx->err = "non-finite init pose"; return PCR_EINVAL; }
    const int grad_nn = 30;                                   // KDTreeSearchParamHybrid(2 * max_correspondence_distance, 30)
    PCR_TRY(pcr_arena_reserve(ctx, pcr_scratch_bytes_for(n_src) + pcr_scratch_bytes_for(n_tgt) + color_list_bytes(n_tgt, grad_nn) + (size_t)(n_src + n_tgt) * 24));
    DevCloud s, t; uint32_t *sperm = nullptr, *tperm = nullptr;
    PCR_TRY(pcr_import_cloud(ctx, src_xyz, nullptr, n_src, &s, &sperm, false));
    PCR_TRY(pcr_import_cloud(ctx, tgt_xyz, tgt_normals, n_tgt, &t, &tperm, true));
    double *si = arena<double>(ctx, n_src > 0 ? n_src : 1), *ti = arena<double>(ctx, n_tgt > 0 ? n_tgt : 1);
    float4 *grad = arena<float4>(ctx, n_tgt > 0 ? n_tgt : 1);
    int32_t *match = arena<int32_t>(ctx, n_src > 0 ? n_src : 1);
    if (!si || !ti || !grad || !match) return PCR_ENOMEM;
    PCR_TRY(color_intensities(ctx, src_colors, sperm, n_src, si));
    PCR_TRY(color_intensities(ctx, tgt_colors, tperm, n_tgt, ti));
    PCR_TRY(color_gradient(ctx, &t, tperm, ti, PCR_SEARCH_HYBRID, grad_nn, 2.0 * max_dist, grad));
    PCR_TRY(pcr_dev_colored_icp(ctx, &s, &t, max_dist, init_T, params, si, ti, grad, result, match));
    if (correspondences) {
        int64_t nc = 0;
        PCR_TRY(pcr_dev_compact_matches(ctx, match, s.n, s.cap, sperm, tperm, correspondences, &nc));
    }
    return PCR_OK;
    });
}

// Colours through the voxel pass: k_voxel_mean averages whatever 3-vector rides in its attribute slot in float64 in input order, so the colours
// take that slot: in the one pass there is when the cloud has no normals, in a second pass of their own when it has.  Points and normals come from exactly the calls
// pcr_voxel_down_sample makes: the same bits in the same Morton order, and the colour rows line up with them because both passes sort the same keys.
extern "C" int pcr_voxel_down_sample_ex(pcr_context *ctx, const float *xyz, const float *normals_in, const float *colors_in, int64_t n, double voxel,
                                        float *out_xyz, float *out_normals, float *out_colors, int64_t *out_n) {
    return pcr_api_call(ctx, [&]() -> int {
    if (n < 0 || !out_n || (n > 0 && (!xyz || !out_xyz))) return PCR_EINVAL;
    if (!(voxel > 0.0)) { ctx->err = "voxel_size <= 0"; return PCR_EINVAL; }
    *out_n = 0;
    if (n == 0) return PCR_OK;
    const bool colors = colors_in && out_colors;
    const bool two = colors && normals_in;                    // colours need a pass of their own only when the normals hold the attribute slot
    PCR_TRY(pcr_arena_reserve(ctx, pcr_scratch_bytes_for(n) * (two ? 2 : 1)));
    double b6[6];
    PCR_TRY(pcr_dev_bounds(ctx, xyz, n, b6));
    const float *attr = normals_in ? normals_in : (colors ? colors_in : nullptr);
    DevCloud v;
    PCR_TRY(pcr_alloc_cloud(ctx, &v, (int)n, attr != nullptr, false));
    PCR_TRY(pcr_dev_voxel(ctx, xyz, attr, n, b6, voxel, &v));
    PCR_TRY(pcr_dev_pack_f4_to_f3(ctx, v.pts, v.n, v.cap, out_xyz));
    if (normals_in && out_normals) PCR_TRY(pcr_dev_pack_f4_to_f3(ctx, v.nrm, v.n, v.cap, out_normals));
    if (colors && !two) PCR_TRY(pcr_dev_pack_f4_to_f3(ctx, v.nrm, v.n, v.cap, out_colors));
    if (two) {
        DevCloud w;
        PCR_TRY(pcr_alloc_cloud(ctx, &w, (int)n, true, false));
        PCR_TRY(pcr_dev_voxel(ctx, xyz, colors_in, n, b6, voxel, &w));
        PCR_TRY(pcr_dev_pack_f4_to_f3(ctx, w.nrm, w.n, w.cap, out_colors));
    }
    return pcr_read_count(ctx, v.n, out_n);
    });
}
