// pcr_pmap.h -- the voxel point map (pcr_pmap.hip): the map as its kernels see it, the struct behind the C handle, and its block policy for the
// block builder of the maps that grow (map_build_block / map_adopt, pcr_mapgrow.h).  The rule is the statement in include/pcr_hip.h (voxel point map).
// This map has many rows per cell, so of the frame it takes the builder and the adoption only; merge and remove_far are its own (pcr_pmap.hip).
#pragma once
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
