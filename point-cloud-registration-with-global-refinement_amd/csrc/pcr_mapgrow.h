// pcr_mapgrow.h -- the frame of the maps that grow: what the voxel covariance map (pcr_vmap.hip) and the normal-distributions map
// (pcr_nmap.hip) do alike when they build, merge and trim, written once over a compile-time row policy.  pcr_vgicp.hip and pcr_ndt.hip take the
// block builder from here for the maps they create.  Nothing here branches on the kind of map at run time: a unit instantiates the kernels and
// hosts with its own policy, under its own floating-point contraction setting.
//
// A row policy `Row` (VmapRow in pcr_vgicp.h, NmapRow in pcr_ndt.h) names
//   Map                      the struct behind the C handle: cells, block, bytes, keys, n_dev, view.{tab, dmask, mean4, cov8, ...}
//   Rows                     the rows as a kernel reads them, in ascending Morton order of the cell: mean4, cov8, keys, n (NDT: info6 too)
//   Out                      the rows of a new block as a kernel writes them: mean4, cov8, keys (NDT: info6 too)
//   Merged                   MERGE's target: cap, the union's row count, and out (NDT: the map's rule too, for the cell that is computed anew)
//   EXTRA, extra(rows/out)   the payload of a row beside mean4 / cov8: none (0, nullptr), or the six doubles of A_v
//   block_bytes(cells)       device bytes of the one block
//   carve(ctx, cells, &out)  the row arrays out of the block, which is the context's arena while the builder carves
//   rows_of(map), set_view(map, out), merged(map, cap, out)
//   count(mean4 row)         N_v from mean4.w: the plain word, or the absolute value of the signed word
//   combine(g, m, c0, c1, x, mb, d0, d1)   a cell held by both maps: (m, c0, c1) is A's row on entry and the union's on return, x its payload
#pragma once
#include <cmath>
#include <string>
#include "pcr_vgicp.h"

#define MG_BS 256
static inline unsigned mg_blocks(size_t n) { return (unsigned)((n + MG_BS - 1) / MG_BS); }

// ================================================================ kernels
// row o of a new block
template <class Row>
__device__ static inline void map_store_row(const typename Row::Out &out, int o, const float4 m, const float4 c0, const float4 c1, uint64_t key, const double *x) {
    out.mean4[o] = m; out.cov8[2 * (size_t)o] = c0; out.cov8[2 * (size_t)o + 1] = c1; out.keys[o] = key;
#pragma unroll
    for (int k = 0; k < Row::EXTRA; k++) Row::extra(out)[Row::EXTRA * (size_t)o + k] = x[k];
}
// lane t < a.n: row t of A finds where its key stands in B (where[t] = lower bound); lane a.n + j: row j of B finds where it stands in A and is
// flagged when A does not hold its cell.  A shared cell whose counts add up past 2^31 - 1 sets *overflow.
template <class Row>
__global__ void __launch_bounds__(MG_BS) k_map_merge_mark(typename Row::Rows a, typename Row::Rows b, int *__restrict__ where, uint8_t *__restrict__ only_b,
                                                          int *__restrict__ overflow) {
    const int t = blockIdx.x * MG_BS + threadIdx.x;
    if (t >= a.n + b.n) return;
    if (t < a.n) { where[t] = vg_lower_bound(b.keys, b.n, a.keys[t]); return; }
    const int j = t - a.n;
    const uint64_t key = b.keys[j];
    const int i = vg_lower_bound(a.keys, a.n, key);
    const bool shared = i < a.n && a.keys[i] == key;
    where[t] = i;
    only_b[j] = shared ? 0 : 1;
    if (shared && (int64_t)Row::count(a.mean4[i]) + (int64_t)Row::count(b.mean4[j]) > 0x7fffffffll) atomicOr(overflow, 1);
}
// the union's rows: row t of A lands at t + (rows of B alone below it), combined with its partner where B holds the cell too; a row of B alone
// lands at (rows of B alone before it) + (rows of A below it)
template <class Row>
__global__ void __launch_bounds__(MG_BS) k_map_merge_write(typename Row::Rows a, typename Row::Rows b, const int *__restrict__ where, const uint8_t *__restrict__ only_b,
                                                           const int *__restrict__ pos_b, const int *__restrict__ total_b, typename Row::Merged g) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * MG_BS + threadIdx.x;
    if (t >= a.n + b.n) return;
    float4 m, c0, c1; uint64_t key; int o;
    double x[Row::EXTRA + 1];
    if (t < a.n) {
        const int j = where[t];
        key = a.keys[t]; m = a.mean4[t]; c0 = a.cov8[2 * (size_t)t]; c1 = a.cov8[2 * (size_t)t + 1];
        o = t + (j < b.n ? pos_b[j] : *total_b);
        if (j < b.n && b.keys[j] == key) {
            Row::combine(g, m, c0, c1, x, b.mean4[j], b.cov8[2 * (size_t)j], b.cov8[2 * (size_t)j + 1]);
        } else {
#pragma unroll
            for (int k = 0; k < Row::EXTRA; k++) x[k] = Row::extra(a)[Row::EXTRA * (size_t)t + k];
        }
    } else {
        const int j = t - a.n;
        if (!only_b[j]) return;
        key = b.keys[j]; m = b.mean4[j]; c0 = b.cov8[2 * (size_t)j]; c1 = b.cov8[2 * (size_t)j + 1];
#pragma unroll
        for (int k = 0; k < Row::EXTRA; k++) x[k] = Row::extra(b)[Row::EXTRA * (size_t)j + k];
        o = pos_b[j] + where[t];
    }
    if (o < 0 || o >= g.cap) return;
    map_store_row<Row>(g.out, o, m, c0, c1, key, x);
}
// keep[v] = d^2 < r^2 (vg_within, pcr_vgicp.h; the count word in mean4.w plays no part)
template <class Row>
__global__ void __launch_bounds__(MG_BS) k_map_far_flags(const float4 *__restrict__ mean4, int n, double cx, double cy, double cz, double r2, uint8_t *__restrict__ keep) {
    const int v = blockIdx.x * MG_BS + threadIdx.x;
    if (v >= n) return;
    keep[v] = vg_within(mean4[v], cx, cy, cz, r2) ? 1 : 0;
}
template <class Row>
__global__ void __launch_bounds__(MG_BS) k_map_gather(typename Row::Rows a, const uint8_t *__restrict__ keep, const int *__restrict__ pos, int cap, typename Row::Out out) {
    const int v = blockIdx.x * MG_BS + threadIdx.x;
    if (v >= a.n || !keep[v]) return;
    const int o = pos[v];
    if (o < 0 || o >= cap) return;
    const float4 m = a.mean4[v], c0 = a.cov8[2 * (size_t)v], c1 = a.cov8[2 * (size_t)v + 1];      // every load before the first store: they overlap
    const uint64_t key = a.keys[v];
    double x[Row::EXTRA + 1];
#pragma unroll
    for (int k = 0; k < Row::EXTRA; k++) x[k] = Row::extra(a)[Row::EXTRA * (size_t)v + k];
    map_store_row<Row>(out, o, m, c0, c1, key, x);
}

// ================================================================ host
// A new block of `cells` rows.  Inside the block (the context's arena while a SideLane holds it): the row arrays, then `fill(out)`, which enqueues
// what writes the keys -- the hash build reads them -- and, for a map that grows, the rows; then the count word and the cell hash.  Back on the
// context's own arena: `after(block)`, which enqueues what needs the hash (the count and pack kernels of the two create paths).  Then the one
// wait.  Finished (the stream is idle) when it returns PCR_OK; on an error nothing of it is left.
template <class Row> struct MapBlock { char *block = nullptr; size_t bytes = 0; typename Row::Out out; int *n_dev = nullptr; GridView gv; };
template <class Row, class Fill, class After>
static int map_build_block(pcr_context *ctx, const char *call, int64_t cells, MapBlock<Row> *b, Fill &&fill, After &&after) {
    b->bytes = Row::block_bytes(cells);
    if (hipMalloc((void **)&b->block, b->bytes) != hipSuccess) { b->block = nullptr; ctx->err = std::string("hipMalloc(") + call + ")"; return PCR_ENOMEM; }
    auto body = [&]() -> int {
        {
            SideLane own(ctx, b->block, b->bytes, ctx->stream);      // the rows and the hash table come out of the block, on the call's own stream
            b->n_dev = Row::carve(ctx, cells, &b->out) ? arena<int>(ctx, 1) : nullptr;
            if (!b->n_dev) return PCR_ENOMEM;
            PCR_TRY(fill(b->out));
            PCR_HIP_CHECK(ctx, hipMemsetD32Async((hipDeviceptr_t)b->n_dev, (int)cells, 1, ctx->stream));
            DevCloud mc;                                             // the cells as a voxel-lattice cloud: what the hash build reads (keys, count, capacity)
            mc.keys = b->out.keys; mc.n = b->n_dev; mc.cap = (int)cells; mc.voxel_lattice = true;
            const DevCloud *pmc = &mc; const int level = 0;
            PCR_TRY(pcr_dev_build_grid_batch(ctx, &pmc, &level, 1, &b->gv));
        }
        if (!b->gv.tab) { ctx->err = std::string(call) + ": no cell hash"; return PCR_EHIP; }
        PCR_TRY(after(*b));
        // finished before the call returns: the caller may overwrite its buffers, and any context may use the map
        PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->launch_err != hipSuccess) return PCR_EHIP;          // (pcr_leave names the launch)
        return PCR_OK;
    };
    const int rc = body();
    if (rc != PCR_OK) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(b->block); b->block = nullptr; }
    return rc;
}
// the new block in, the old one (if any) out: hipFree waits for the device, so no call is still reading the old block
template <class Row> static void map_adopt(typename Row::Map *m, const MapBlock<Row> &b, int64_t cells) {
    char *old = m->block;
    m->cells = cells; m->block = b.block; m->bytes = b.bytes; m->keys = b.out.keys; m->n_dev = b.n_dev;
    m->view.tab = b.gv.tab; m->view.dmask = b.gv.dmask;
    Row::set_view(m, b.out);
    if (old) (void)hipFree(old);
}

// map <- MERGE(map, b); b's rows live in another map or in the context's arena.  Never reserves the arena: pcr_voxel_map_insert keeps the scan's
// rows (b) in it and a reserve may move or recycle them, so every caller reserves once, for this scratch and for what it keeps in the arena itself.
template <class Row> static int map_merge_into(pcr_context *ctx, const char *call, typename Row::Map *map, const typename Row::Rows &b) {
    const typename Row::Rows a = Row::rows_of(map);
    const size_t total = (size_t)a.n + (size_t)b.n;
    if (total > (size_t)(0x7fffffff / 8)) { ctx->err = std::string(call) + ": the merged map would hold 2^28 rows or more"; return PCR_EINVAL; }
    int *where = arena<int>(ctx, total), *pos_b = arena<int>(ctx, (size_t)b.n), *word = arena<int>(ctx, 2);
    uint8_t *only_b = arena<uint8_t>(ctx, (size_t)b.n);
    if (!where || !pos_b || !word || !only_b) return PCR_ENOMEM;
    int *total_b = word, *overflow = word + 1;
    PCR_HIP_CHECK(ctx, hipMemsetAsync(word, 0, 2 * sizeof(int), ctx->stream));
    PCR_LAUNCH(ctx, k_map_merge_mark<Row>, dim3(mg_blocks(total)), dim3(MG_BS), 0, ctx->stream, a, b, where, only_b, overflow);
    PCR_TRY(pcr_dev_flag_scan(ctx, only_b, nullptr, b.n, pos_b, total_b));
    int h[2] = {0, 0};
    PCR_HIP_CHECK(ctx, hipMemcpyAsync(h, word, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (h[1]) { ctx->err = std::string(call) + ": the member count of a cell would pass 2^31 - 1"; return PCR_EINVAL; }
    if (h[0] < 0 || h[0] > b.n) { ctx->err = std::string(call) + ": the scan of the new cells is out of range"; return PCR_EHIP; }
    const int64_t cells = (int64_t)a.n + h[0];
    MapBlock<Row> nb;
    PCR_TRY(map_build_block<Row>(ctx, call, cells, &nb, [&](const typename Row::Out &o) -> int {
        PCR_LAUNCH(ctx, k_map_merge_write<Row>, dim3(mg_blocks(total)), dim3(MG_BS), 0, ctx->stream, a, b, where, only_b, pos_b, total_b, Row::merged(map, (int)cells, o));
        return PCR_OK;
    }, [](const MapBlock<Row> &) -> int { return PCR_OK; }));
    map_adopt<Row>(map, nb, cells);
    return PCR_OK;
}

// map <- REMOVE_FAR(map, center, max_distance), with the argument checks; the caller has checked the map.  Nothing of the call lives in the arena
// before this, so it reserves `scratch` bytes of it itself, after the checks.
template <class Row>
static int map_remove_far(pcr_context *ctx, const char *call, typename Row::Map *map, const double *center3, double max_distance, int64_t *removed, size_t scratch) {
    const std::string who(call);
    if (!center3) { ctx->err = who + ": center3 is null"; return PCR_EINVAL; }
    for (int d = 0; d < 3; d++) if (!std::isfinite(center3[d])) { ctx->err = who + ": center3 holds a non-finite value"; return PCR_EINVAL; }
    if (!std::isfinite(max_distance) || !(max_distance > 0.0)) { ctx->err = who + ": max_distance must be finite and greater than 0"; return PCR_EINVAL; }
    PCR_TRY(pcr_arena_reserve(ctx, scratch));
    const typename Row::Rows a = Row::rows_of(map);
    uint8_t *keep = arena<uint8_t>(ctx, (size_t)a.n);
    int *pos = arena<int>(ctx, (size_t)a.n), *total = arena<int>(ctx, 1);
    if (!keep || !pos || !total) return PCR_ENOMEM;
    const double r2 = max_distance * max_distance;
    PCR_LAUNCH(ctx, k_map_far_flags<Row>, dim3(mg_blocks((size_t)a.n)), dim3(MG_BS), 0, ctx->stream, a.mean4, a.n, center3[0], center3[1], center3[2], r2, keep);
    PCR_TRY(pcr_dev_flag_scan(ctx, keep, nullptr, a.n, pos, total));
    int64_t kept = 0;
    PCR_TRY(pcr_read_count(ctx, total, &kept));
    if (kept < 0 || kept > a.n) { ctx->err = who + ": the scan of the kept rows is out of range"; return PCR_EHIP; }
    if (kept == 0) { ctx->err = who + ": would leave the map empty"; return PCR_EINVAL; }
    if (kept == a.n) return PCR_OK;                           // every row stays, with its bits and its place
    MapBlock<Row> nb;
    PCR_TRY(map_build_block<Row>(ctx, call, kept, &nb, [&](const typename Row::Out &o) -> int {
        PCR_LAUNCH(ctx, k_map_gather<Row>, dim3(mg_blocks((size_t)a.n)), dim3(MG_BS), 0, ctx->stream, a, keep, pos, (int)kept, o);
        return PCR_OK;
    }, [](const MapBlock<Row> &) -> int { return PCR_OK; }));
    if (removed) *removed = (int64_t)a.n - kept;
    map_adopt<Row>(map, nb, kept);
    return PCR_OK;
}
