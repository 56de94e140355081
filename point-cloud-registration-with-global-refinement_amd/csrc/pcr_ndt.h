// pcr_ndt.h -- what pcr_ndt.hip (the map of a cloud, the NDT iteration) and pcr_nmap.hip (the map that grows) share: the map as the kernels see it,
// the map behind the C handle, its row policy for the frame of the maps that grow (NmapRow; pcr_mapgrow.h), the one device function that turns
// (N_v, C_v) into validity and A_v, and the builder of a map on a given grid.
// The rule is the statement in include/pcr_hip.h.
#pragma once
#include "pcr_vgicp.h"

// One map row per occupied cell, in Morton order of the cell: mean4[v] = (mean, w = bit pattern of +N_v for a valid cell and of -N_v for an invalid
// one), info6[6 v ...] = A_v (xx,xy,xz,yy,yz,zz; zero for an invalid cell), cov8[2 v], cov8[2 v + 1] = C_v as in VgicpMapView; `tab`: cell -> (row, 1)
struct NdtMapView {
    const GridEntry *tab; const unsigned *dmask;
    const float4 *mean4, *cov8;
    const double *info6;
    double org[3], voxel;
};
// The map behind the C handle (pcr_ndt.hip builds, reads and destroys it; pcr_nmap.hip grows and trims it by swapping in a new block).
struct pcr_ndt_map {
    int device = 0;
    int64_t cells = 0;
    char *block = nullptr;       // the one allocation: rows, keys, count word, cell hash
    size_t bytes = 0;
    NdtMapView view;
    uint64_t *keys = nullptr;    // Morton keys of the rows (ascending)
    int *n_dev = nullptr;
    double grid_min[3] = {0, 0, 0};     // g of the RULE OF A MAP: view.org = g - voxel / 2
    int min_points = 0;                 // the rule by which every row's validity and A_v follow from (N_v, C_v)
    double ratio = 0;
};
static inline size_t ndt_block_bytes(int64_t cells) {
    return (size_t)cells * (sizeof(float4) * 3 + sizeof(double) * 6 + sizeof(uint64_t)) + (size_t)pcr_grid_slots((unsigned)cells) * sizeof(GridEntry) + 16 * 256;
}
// The map's row policy for the frame of the maps that grow (pcr_mapgrow.h states what each member is); combine is pcr_nmap.hip's.
struct NmapRow {
    typedef pcr_ndt_map Map;
    struct Rows { const float4 *mean4, *cov8; const double *info6; const uint64_t *keys; int n; };
    struct Out { float4 *mean4, *cov8; double *info6; uint64_t *keys; };
    struct Merged { int cap, min_points; double ratio; Out out; };
    static constexpr int EXTRA = 6;
    __device__ static inline const double *extra(const Rows &r) { return r.info6; }
    __device__ static inline double *extra(const Out &o) { return o.info6; }
    static size_t block_bytes(int64_t cells) { return ndt_block_bytes(cells); }
    static bool carve(pcr_context *ctx, int64_t cells, Out *o) {
        o->mean4 = arena<float4>(ctx, (size_t)cells); o->cov8 = arena<float4>(ctx, 2 * (size_t)cells); o->info6 = arena<double>(ctx, 6 * (size_t)cells);
        o->keys = arena<uint64_t>(ctx, (size_t)cells);
        return o->mean4 && o->cov8 && o->info6 && o->keys;
    }
    static Rows rows_of(const Map *m) { return Rows{m->view.mean4, m->view.cov8, m->view.info6, m->keys, (int)m->cells}; }
    static void set_view(Map *m, const Out &o) { m->view.mean4 = o.mean4; m->view.cov8 = o.cov8; m->view.info6 = o.info6; }
    static Merged merged(const Map *m, int cap, const Out &o) { return Merged{cap, m->min_points, m->ratio, o}; }
    __device__ static inline int count(const float4 m) { const int w = __float_as_int(m.w); return w < 0 ? -w : w; }      // the sign carries the validity
    __device__ static inline void combine(const Merged &g, float4 &m, float4 &c0, float4 &c1, double *x, const float4 mb, const float4 d0, const float4 d1);
};
__device__ static inline VgicpMapView ndt_hash(const NdtMapView &m) {      // what vg_row reads of a map
    VgicpMapView g;
    g.tab = m.tab; g.dmask = m.dmask; g.mean4 = m.mean4; g.cov8 = m.cov8;
    return g;
}

// Validity and A_v of a cell from its count and its float32 C_v (c0 = xx,xy,xz,yy; c1 = yz,zz): A_v = V diag(1 / max(lambda_k, ratio lambda_max)) V^T
// of S_v = C_v N_v / (N_v - 1) by cyclic Jacobi sweeps in float64 (the sweeps of vg_sym3_inv_sqrt, pcr_vgicp.hip).  The clamp bounds the condition
// number of A_v by 1 / ratio, so the rounding of the eigenvectors of clamped (nearly equal after the clamp) eigenvalues does not show in A_v.
// A6 is zero for an invalid cell.  A pure function of its arguments: the map of a cloud and a merged cell go through the same instructions.
__device__ static inline bool ndt_cell_information(int nv, const float4 c0, const float4 c1, int min_points, double ratio, double *A6) {
#pragma clang fp contract(off)
#pragma unroll
    for (int t = 0; t < 6; t++) A6[t] = 0.0;
    bool valid = false;
    if (nv >= min_points && nv >= 2) {
        const double N = (double)nv, N1 = N - 1.0;
        const double sxx = (double)c0.x * N / N1, sxy = (double)c0.y * N / N1, sxz = (double)c0.z * N / N1, syy = (double)c0.w * N / N1, syz = (double)c1.x * N / N1,
                     szz = (double)c1.y * N / N1;
        double a[9] = {sxx, sxy, sxz, sxy, syy, syz, sxz, syz, szz}, V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        for (int sweep = 0; sweep < 64; sweep++) {
            double off = a[1] * a[1]; off = off + a[2] * a[2]; off = off + a[5] * a[5];
            double diag = a[0] * a[0]; diag = diag + a[4] * a[4]; diag = diag + a[8] * a[8];
            if (off <= 1e-300 || off <= 1e-34 * diag) break;
#pragma unroll
            for (int pq = 0; pq < 3; pq++) {
                const int p_ = pq == 2 ? 1 : 0, q_ = pq == 0 ? 1 : 2;
                const double apq = a[p_ * 3 + q_];
                if (apq != 0.0) {
                    const double theta = (a[q_ * 3 + q_] - a[p_ * 3 + p_]) / (2.0 * apq);
                    const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
                    for (int k = 0; k < 3; k++) { const double akp = a[k * 3 + p_], akq = a[k * 3 + q_]; a[k * 3 + p_] = c * akp - sn * akq; a[k * 3 + q_] = sn * akp + c * akq; }
#pragma unroll
                    for (int k = 0; k < 3; k++) { const double apk = a[p_ * 3 + k], aqk = a[q_ * 3 + k]; a[p_ * 3 + k] = c * apk - sn * aqk; a[q_ * 3 + k] = sn * apk + c * aqk; }
#pragma unroll
                    for (int k = 0; k < 3; k++) { const double vkp = V[k * 3 + p_], vkq = V[k * 3 + q_]; V[k * 3 + p_] = c * vkp - sn * vkq; V[k * 3 + q_] = sn * vkp + c * vkq; }
                }
            }
        }
        const double lmax = fmax(a[0], fmax(a[4], a[8]));
        if (lmax > 0.0 && isfinite(lmax)) {
            valid = true;
            const double fl = ratio * lmax;
            const double i0 = 1.0 / fmax(a[0], fl), i1 = 1.0 / fmax(a[4], fl), i2 = 1.0 / fmax(a[8], fl);
            int t = 0;
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = r; c < 3; c++) {
                    double s = V[r * 3] * V[c * 3] * i0; s = s + V[r * 3 + 1] * V[c * 3 + 1] * i1; s = s + V[r * 3 + 2] * V[c * 3 + 2] * i2;
                    A6[t++] = s;
                }
        }
    }
    return valid;
}

// host helpers of pcr_ndt.hip that pcr_nmap.hip calls too
int ndt_check_map(pcr_context *ctx, const pcr_ndt_map *map, const char *call);
// A new map of the n points of xyz (MAP of the NDT section), finished when it returns.  grid_min3 == NULL: the grid of the cloud's own minimum;
// otherwise the given grid, and a member outside its 2^21 cells per axis is PCR_EINVAL.  T (16 doubles) == NULL: the points as they lie, not even
// the identity is applied; otherwise the members are p' = float32(T p).  Reserves the context's arena for itself.
int ndt_map_build(pcr_context *ctx, const char *call, const float *xyz, int64_t n, double voxel_size, int min_points_per_voxel, double eigenvalue_ratio,
                  const double *grid_min3, const double *T, pcr_ndt_map **out);
