// pcr_pmap.h -- the voxel point map (pcr_pmap.hip): the map as its kernels see it, the struct behind the C handle, and its block policy for the
// block builder of the maps that grow (map_build_block / map_adopt, pcr_mapgrow.h).  The rule is the statement in include/pcr_hip.h (voxel point map).
// This map has many rows per cell, so of the frame it takes the builder and the adoption only; merge and remove_far are its own (pcr_pmap.hip).
#pragma once
#include "pcr_icp_loop.h"
#include "pcr_mapgrow.h"

// Rows are the kept points, ordered by (Morton key of the cell, arrival): xyz[3 r .. 3 r + 2] and, in a map with normals, nrm[3 r .. 3 r + 2], packed
// float32.  `tab` is the cell hash of level 0 over the rows' keys (pcr_dev_build_grid_batch): cell -> (first row, member count).
struct PmapView {
    const GridEntry *tab; const unsigned *dmask;
    const float *xyz, *nrm;                // nrm == nullptr: a map without normals
    double org[3], voxel;                  // origin = grid_min - voxel / 2 in float64 (the GRID rule of the voxel covariance map)
};

struct pcr_point_map {
    int device = 0;
    int64_t cells = 0;           // the ROWS of the map (the frame's name for the row count: map_adopt sets it)
    int64_t n_cells = 0;         // occupied cells
    char *block = nullptr;       // the one allocation: rows, keys, cell table, count word, cell hash
    size_t bytes = 0;
    PmapView view;
    uint64_t *keys = nullptr;    // Morton key of every row's cell (ascending, equal inside a cell)
    int *n_dev = nullptr;        // the row count on the device (what the hash build reads)
    int *cell_first = nullptr;   // n_cells + 1 entries: first row of every cell in Morton order, then the row count
    double grid_min[3] = {0, 0, 0};
    int max_points = 0;          // M of the rule
    bool normals = false;        // the rows have normals: the caller's, or (estimated) the map's own
    // ESTIMATE: the map computes its normals from its own rows and keeps them current (include/pcr_hip.h)
    bool estimated = false;
    double est_radius = 0.0;     // rho
    int est_min = 0;             // k_min
    int32_t *ncount = nullptr;   // neighbours of every row within rho, the row itself included (in the block)
    int64_t valid_rows = 0;      // rows with ncount >= k_min
};

// The block policy: what map_build_block and map_adopt ask of a Row (block_bytes, carve, Out with keys, Map, set_view).  NRM: the map has normals;
// EST (with NRM): they are the map's own, and the block holds the neighbour count of every row and the word the valid rows are counted in.
template <bool NRM, bool EST = false> struct PmapRow {
    typedef pcr_point_map Map;
    struct Out { float *xyz, *nrm; uint64_t *keys; int *cell_first; int32_t *ncount; int *nvalid; };
    static size_t block_bytes(int64_t rows) {
        return (size_t)rows * (sizeof(float) * (NRM ? 6 : 3) + sizeof(uint64_t) + sizeof(int) + (EST ? sizeof(int32_t) : 0)) + (size_t)pcr_grid_slots((unsigned)rows) * sizeof(GridEntry) +
               (EST ? 18 : 16) * 256;
    }
    static bool carve(pcr_context *ctx, int64_t rows, Out *o) {
        o->xyz = arena<float>(ctx, 3 * (size_t)rows); o->nrm = NRM ? arena<float>(ctx, 3 * (size_t)rows) : nullptr;
        o->keys = arena<uint64_t>(ctx, (size_t)rows); o->cell_first = arena<int>(ctx, (size_t)rows + 1);
        o->ncount = EST ? arena<int32_t>(ctx, (size_t)rows) : nullptr; o->nvalid = EST ? arena<int>(ctx, 1) : nullptr;
        return o->xyz && (!NRM || o->nrm) && o->keys && o->cell_first && (!EST || (o->ncount && o->nvalid));
    }
    static void set_view(Map *m, const Out &o) { m->view.xyz = o.xyz; m->view.nrm = o.nrm; m->cell_first = o.cell_first; m->ncount = o.ncount; }
};

// ================================================================ the search (pcr_pmap.hip, pcr_ctime.hip)
__device__ static inline void pm_search(const PmapView &m, unsigned mask, int nbh, bool live, double qx, double qy, double qz, int ol, double &best_d2, int &best_row) {
    GridView g;
    g.tab = m.tab; g.dmask = m.dmask; g.L = 0;
    const int cx = vg_cell(qx, m.org[0], m.voxel), cy = vg_cell(qy, m.org[1], m.voxel), cz = vg_cell(qz, m.org[2], m.voxel);
    double bd = INFINITY; int br = 0x7fffffff;
    const int rounds = nbh == 27 ? 4 : 1;
    for (int r = 0; r < rounds; r++) {                                   // (wave-uniform)
        const int k = r * 8 + ol;
        int first = 0, cnt = 0;
        if (live && k < nbh) {
            int dx, dy, dz;
            vg_offset(nbh, k, dx, dy, dz);
            const int2 e = pcr_grid_lookup(g, mask, cx + dx, cy + dy, cz + dz);
            if (e.y > 0) { first = e.x; cnt = e.y; }
        }
        if (__ballot(cnt > 0) == 0ull) continue;                         // (wave-uniform)
        for (int l = 0; l < 8; l++) {                                    // (wave-uniform: the exchanges below are reached by all 64 lanes together)
            const int f = __shfl(first, l, 8), c = __shfl(cnt, l, 8);
            for (int j = ol; j < c; j += 8) {
                const int row = f + j;
                const float *p = m.xyz + (size_t)row * 3;
                const double dx = qx - (double)p[0], dy = qy - (double)p[1], dz = qz - (double)p[2];
                const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
                double d2 = xx + yy;
                d2 = d2 + zz;
                if (d2 < bd || (d2 == bd && row < br)) { bd = d2; br = row; }
            }
        }
    }
#pragma unroll
    for (int s = 1; s < 8; s <<= 1) {
        const double od = __shfl_xor(bd, s, 8); const int orow = __shfl_xor(br, s, 8);
        if (od < bd || (od == bd && orow < br)) { bd = od; br = orow; }
    }
    best_d2 = bd; best_row = br == 0x7fffffff ? -1 : br;
}
// the match of every lane's own point: lane t of an octet holds point t of the octet's eight; round r searches for the point of lane r
__device__ static inline void pm_match_own(const PmapView &m, int nbh, bool live, double qx, double qy, double qz, double max_d2, double &my_d2, int &my_row) {
    const unsigned mask = *m.dmask;
    const int ol = threadIdx.x & 7;
    my_d2 = 0.0; my_row = -1;
    for (int r = 0; r < 8; r++) {                                        // (wave-uniform)
        const double bx = __shfl(qx, r, 8), by = __shfl(qy, r, 8), bz = __shfl(qz, r, 8);
        const bool bl = __shfl(live ? 1 : 0, r, 8) != 0;
        if (__ballot(bl) == 0ull) continue;                              // (wave-uniform)
        double d2; int row;
        pm_search(m, mask, nbh, bl, bx, by, bz, ol, d2, row);
        if (ol == r && row >= 0 && d2 < max_d2) { my_d2 = d2; my_row = row; }
    }
}

// the robust kernels of the UPDATE rule
__device__ static inline double pm_weight(int loss, double k, double r) {
    if (loss == PCR_LOSS_L1) return 1.0 / fmax(fabs(r), 1e-300);
    if (loss == PCR_LOSS_GM) { const double rr = r * r; const double d = k + rr; return k / (d * d); }
    return 1.0;
}

// The rows of one correspondence -- the point q at its pose against map row `row` -- into the 27 sums of A: [0, 21) upper w J^T J, [21, 27) w J^T r;
// returns the squared residual (point to plane: r^2; point to point: |e|^2).  (lx, ly, lz) is the lever of the rotation columns: q itself for the
// rigid pose of pcr_pmap.hip, u = R p (q without its translation) for the pose pair of pcr_ctime.hip.  Called from units that contract nothing.
__device__ static inline double pm_row27(const PmapView &m, int plane, int loss, double loss_k, int row, double qx, double qy, double qz, double lx, double ly, double lz, double *A) {
    const float *p = m.xyz + (size_t)row * 3;
    const double ex = qx - (double)p[0], ey = qy - (double)p[1], ez = qz - (double)p[2];
    if (plane) {
        const float *nf = m.nrm + (size_t)row * 3;
        const double nx = nf[0], ny = nf[1], nz = nf[2];
        double r = ex * nx + ey * ny;
        r = r + ez * nz;
        const double J[6] = {ly * nz - lz * ny, lz * nx - lx * nz, lx * ny - ly * nx, nx, ny, nz};
        icp_row6(pm_weight(loss, loss_k, r), J, r, A);
        return r * r;
    }
    double nn = ex * ex + ey * ey;
    nn = nn + ez * ez;
    const double w = pm_weight(loss, loss_k, sqrt(nn));
    const double J0[6] = {0.0, lz, -ly, 1.0, 0.0, 0.0}, J1[6] = {-lz, 0.0, lx, 0.0, 1.0, 0.0}, J2[6] = {ly, -lx, 0.0, 0.0, 0.0, 1.0};
    icp_row6(w, J0, ex, A); icp_row6(w, J1, ey, A); icp_row6(w, J2, ez, A);
    return nn;
}

// what the calls that search the map check alike, and their scratch (pcr_pmap.hip): the map, the neighbourhood, the source, the distance and one pose
// (named T_name); the estimator against the map; the source's coordinates (one read-back)
int pm_check_search(pcr_context *ctx, const char *call, const pcr_point_map *map, const float *src_xyz, int64_t n_src, const double *T, const char *T_name, int nbh,
                    double max_distance);
int pm_check_estimation(pcr_context *ctx, const char *call, const pcr_point_map *map, const pcr_estimation *est);
int pm_check_src_finite(pcr_context *ctx, const char *call, const float *src_xyz, int64_t n_src);
size_t pm_search_scratch(int64_t n_src);
// point to plane on a map that estimates its normals: a match whose row is not valid is no row
static inline bool pm_reads_validity(const pcr_point_map *map, const pcr_estimation *est) { return map->estimated && est->kind == PCR_EST_POINT_TO_PLANE; }
