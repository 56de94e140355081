// pcr_icp_loop.h -- what the iteration kernels of the ICP loops share, and the host side of a loop: the problem state and the argument block, the
// end of an iteration (icp_finish: workgroup reduction, last-workgroup gather, convergence test, 6x6 solve, pose update), the graph cache and the
// chunk pump; and the frame of the map loops, whose iteration is ONE kernel over the source points in caller order (icp_iter_frame on the device,
// icp_map_loop on the host).  Included by pcr_gicp.hip (GICP, the three ICP estimators, colored ICP, the lockstep groups), by
// pcr_vgicp.hip (voxelized GICP), pcr_ndt.hip (NDT) and pcr_pmap.hip (the voxel point map), which run a map loop, and by pcr_ctime.hip (continuous
// time, for icp_row6 and the tile size); each is a unit of its own so that the search kernels of pcr_gicp.hip compile to what they compiled to
// before the others existed.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "pcr_octree.h"
#include "pcr_umeyama.h"
#include "pcr_solve6.h"

#define ICP_BS 256
#define NV 30            // 21 (upper JTJ) + 6 (JTr) + sum r^2 + sum d^2 + count
#define NVP 32           // padded row of a partial
#define LIN_BS 512           // linearise kernel: few fat workgroups => few partial rows for the last one to gather
#define LIN_MAX_BLOCKS 128

// _COV: per-point covariances given (GICP_robusto path); P2PL / P2P / P2P_SCALED: registration_icp with TransformationEstimationPointToPlane /
// PointToPoint(with_scaling = false / true) -- k_icp_nn + k_icp_iter<MODE> only, never the fused or group forms
// COLORED: registration_colored_icp -- k_icp_nn + k_icp_iter_colored, a sibling of k_icp_iter with its own argument block (IcpColorArgs)
// VGICP: registration_voxelized_gicp -- k_icp_iter_vgicp alone (no search kernel), a sibling with its own argument block (IcpVoxelArgs); to
//   icp_finish the mode means one thing: sums[27] counts the source points with a row (the fitness), sums[29] the rows
// NDT: registration_ndt -- k_icp_iter_ndt alone (pcr_ndt.hip), a sibling with its own argument block (IcpNdtArgs); to icp_finish it is VGICP
enum { ICP_MODE_GICP = 0, ICP_MODE_EVAL = 1, ICP_MODE_GICP_COV = 2, ICP_MODE_P2PL = 3, ICP_MODE_P2P = 4, ICP_MODE_P2P_SCALED = 5, ICP_MODE_COLORED = 6, ICP_MODE_VGICP = 7,
       ICP_MODE_NDT = 8 };

struct IcpState {
    double T[16];
    double fitness, rmse;       // of the most recent search
    double sums[NVP];           // reduced sums of the most recent launch
    long long count;
    int iter;                   // pose updates applied
    int launches;               // searches done
    int done, converged;
    unsigned int ticket;
    int ns;                     // source points of this problem (for the byte model)
    unsigned long long t_start; // s_memrealtime (100 MHz) stamp of workgroup 0 at kernel entry
    unsigned long long t_live;  // sum over live launches of (last workgroup's exit stamp - t_start)
    unsigned long long t_dbg[4]; // diagnostic stamps (sum): wg0 after search, wg0 after reduce, last wg entering tail, last wg after partial sums
    unsigned long long searched; // queries whose certificate did not hold, summed over the launches after the cold one (bench: fraction searched)
    double dfit, drmse;         // |change| of fitness / rmse at the most recent launch (what the criteria test): the host sizes the next chunk of launches by them
};

struct IcpArgs {
    const float4 *src_pts, *src_nrm; const int *ns_ptr;
    const float *src_cov6, *tgt_cov6;            // optional raw covariances (xx,xy,xz,yy,yz,zz), Morton order
    const float4 *tgt_pts, *tgt_nrm; OctView tgt; const int *nt_ptr;
    GridView grid;                               // cell hash of the target (grid.tab == nullptr: search the octree)
    int32_t *match; int src_cap;
    int tile_rt;                                 // fused kernel: source points per workgroup of THIS problem when smaller than the kernel's tile (0: the kernel's): a launch of a lockstep
                                                 //   group has one kernel form, its pairs their own tile by their own size (same bits however the batch is cut)
    float4 *ref; int32_t *rbest;                 // per source point: position and margin / nearest point of its last search (skip certificate, tree-walk form)
    int4 *clist;                                 // cell-hash form: the PCR_NN_K nearest target points of the last search (list certificate); ref.w = distance of the next one
    float r2s, rs_minus_r;                       // search cap (r + g)^2 of the certificate mode and g = the unmatched margin
    int verify;                                  // diagnostics (PCR_ICP_VERIFY): search certified queries too and report disagreements
    IcpState *state;
    double *partials;
    double max_dist2; float r2f;
    int loss; double loss_k; double a;          // a = 1 - epsilon
    double rel_fit, rel_rmse; int max_it;
    int single;                                  // 1: linearise once, never update (debug / evaluate)
    // all scales of a pair behind ONE argument slot (pcr_dev_gicp_group_scales; ms_scales == 0: a single scale): when the criteria of scale ms_index
    // hold, the last workgroup stores the state in ms_hist[ms_index] and -- unless it was the last scale -- starts the next one itself: launches,
    // iterations and flags back to their start values, the pose kept, and ms_args[ms_index + 1] copied over *ms_self, the slot the next launch reads.
    // A launch that finds launches == 0 is the scale's first: no certificate is valid, every query is searched (what k_icp_nn + k_icp_lin do).
    const IcpArgs *ms_args; IcpArgs *ms_self; IcpState *ms_hist; int ms_scales, ms_index;
};

struct IcpInit { double T[16]; };
__device__ static inline void d_icp_init(IcpState *st, const IcpInit &in) {
    if (threadIdx.x == 0) {
        for (int k = 0; k < 16; k++) st->T[k] = in.T[k];
        st->fitness = 0; st->rmse = 0; st->count = 0; st->iter = 0; st->launches = 0; st->done = 0; st->converged = 0; st->ticket = 0; st->ns = 0; st->t_start = 0; st->t_live = 0; st->searched = 0; st->dfit = 1e300; st->drmse = 1e300; for (int k = 0; k < 4; k++) st->t_dbg[k] = 0;
        for (int k = 0; k < NVP; k++) st->sums[k] = 0;
    }
}
// the one init kernel of every loop that starts from one pose (internal linkage: every unit that includes this header gets its own)
__global__ static void k_icp_init(IcpState *st, IcpInit in) { d_icp_init(st, in); }

// ---- workgroup reduction of acc[], write-through partial row + ticket, and -- in the last-arriving workgroup -- the end of
// the iteration: gather the rows, fixed-order sums, convergence test, 6x6 solve, pose update.  BS = workgroup size.
template <int MODE, int BS>
__device__ static inline void icp_finish(const IcpArgs &a, IcpState *st, const double *T, double *acc, int nb, int ns, int launches, unsigned long long t_entry, int row) {
    __shared__ double red[BS / 16][NVP];           // one row per 16-lane DPP row
    __shared__ double fin[16][NVP];
    __shared__ int is_last;
    __shared__ double ldl_w[96];
    __shared__ int ldl_perm[6];
    const unsigned long long t_search = wall_clock64() - t_entry;
    // ---- workgroup reduction: DPP butterfly inside every 16-lane row (no LDS crossbar), then the 64 rows in order
    const int lane = threadIdx.x & 63;
#ifdef ICP_ROWSUM_FULL
#pragma unroll
    for (int k = 0; k < NV; k++) { const double s = pcr_row16_sum(acc[k]); if ((lane & 15) == 0) red[threadIdx.x >> 4][k] = s; }
#else
    {   // halving butterfly (pcr_device.h): lane r of a row ends with the sums of values r and 16 + r -- the same bits as pcr_row16_sum, 218 instead of 384 instructions
        double lo, hi;
        pcr_row16_sum_halving<NV>(acc, lane, &lo, &hi);
        const int r = lane & 15;
        red[threadIdx.x >> 4][r] = lo;
        if (16 + r < NV) red[threadIdx.x >> 4][16 + r] = hi;
    }
#endif
    __syncthreads();
    if (threadIdx.x < NV) {
        double s = red[0][threadIdx.x];
#pragma unroll 8
        for (int w = 1; w < BS / 16; w++) s += red[w][threadIdx.x];
        // publish write-through (sc1): no per-workgroup release fence (a release = whole-L2 write-back; ~700 of
        // them per launch serialised to >100 us).  cdna_hip_programming.md Guideline 16, recipe R1.
        __hip_atomic_store(&a.partials[(size_t)row * NVP + threadIdx.x], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 63) {   // diagnostics in the two padding columns: ticks to end-of-search / end-of-reduction (gathered as the maximum over the workgroups)
        __hip_atomic_store(&a.partials[(size_t)row * NVP + 30], (double)t_search, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&a.partials[(size_t)row * NVP + 31], (double)(wall_clock64() - t_entry), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing wave drains its stores ...
    __syncthreads();                                       // ... before ONE lane signals for the workgroup
    if (threadIdx.x == 0) {
        const unsigned int t = __hip_atomic_fetch_add(&st->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = (t == (unsigned int)(nb - 1));
        is_last = last;
    }
    __syncthreads();
    if (!is_last) return;

    // ---- last workgroup: gather the partial rows with sc0 sc1 loads (coherent at agent scope without invalidating this XCD's
    // L2: the acquire fence that plain loads would need took ~10 us here).  Buffer loads through a raw descriptor are visible to the
    // compiler, which keeps all 20 of a lane in flight behind counted waits: 320 rows (160k source points) in ONE round trip where
    // hand-written 8-load groups took three.
    {
        typedef unsigned int icp_u2 __attribute__((ext_vector_type(2)));
        constexpr int NCH = BS / 32;                                       // chunks of 32 columns; chunk c <- rows c, c + NCH, ...
        const int vcol = threadIdx.x & 31, chunk = threadIdx.x >> 5;
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)a.partials, 0, nb * NVP * 8, 0x00020000);
        double s = 0.0;
        for (int b0 = 0; b0 < nb; b0 += NCH * 20) {
            double v[20];
#pragma unroll
            for (int r = 0; r < 20; r++) {
                const int row = b0 + chunk + NCH * r;
                union { icp_u2 u; double d; } x;
                x.u = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (row < nb ? row : 0) * (NVP * 8) + vcol * 8, 0, 17 /* sc0 | sc1 */);
                v[r] = x.d;
            }
#pragma unroll
            for (int r = 0; r < 20; r++) { const double x = b0 + chunk + NCH * r < nb ? v[r] : 0.0; s = vcol < NV ? s + x : fmax(s, x); }
        }
        fin[chunk][vcol] = s;
    }
    __syncthreads();
    if (threadIdx.x < NVP) {
        double s = 0;
#pragma unroll
        for (int c = 0; c < BS / 32; c++) s = threadIdx.x < NV ? s + fin[c][threadIdx.x] : fmax(s, fin[c][threadIdx.x]);
        fin[0][threadIdx.x] = s;
        st->sums[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        // The end of the iteration on the first WAVEFRONT: every lane runs the same scalar work on the same sums (no extra time), so that the
        // three sine / cosine pairs of the pose update -- two thirds of this tail's dependent instructions when one lane computed them one
        // after the other -- are taken by three lanes at once; lane 0 alone writes the state.
        const bool lead = threadIdx.x == 0;
        const unsigned long long t0k = st->t_start;    // stamped by k_icp_nn (previous kernel)
        if (lead) {
            st->t_dbg[3] += wall_clock64() - t0k;
            st->t_dbg[0] += (unsigned long long)fin[0][30]; st->t_dbg[1] += (unsigned long long)fin[0][31];
        }
        const double *S = fin[0];
        const long long count = (long long)(S[29] + 0.5);
        const long long hits = (MODE == ICP_MODE_VGICP || MODE == ICP_MODE_NDT) ? (long long)(S[27] + 0.5) : count;      // (a constant copy of count for every other mode)
        const double fit = ns > 0 ? (double)hits / (double)ns : 0.0;
        const double rmse = count > 0 ? sqrt(S[28] / (double)count) : 0.0;
        const double fit_prev = st->fitness, rmse_prev = st->rmse; const int iter_prev = st->iter;
        bool stop = false, conv = false;
        if (a.single) stop = true;
        else if (launches > 0 && fabs(fit_prev - fit) < a.rel_fit && fabs(rmse_prev - rmse) < a.rel_rmse) { stop = true; conv = true; }
        else if (iter_prev >= a.max_it) stop = true;
        if (lead) {
            st->dfit = launches > 0 ? fabs(fit_prev - fit) : 1e300; st->drmse = launches > 0 ? fabs(rmse_prev - rmse) : 1e300;
            st->fitness = fit; st->rmse = rmse; st->count = count;
        }
        if (!stop && MODE != ICP_MODE_EVAL) {
            double U[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
            if (count > 0 && (MODE == ICP_MODE_P2P || MODE == ICP_MODE_P2P_SCALED)) {
                const float4 o = a.tgt_pts[0];                 // the origin of the moments (icp_point)
                const double org[3] = {o.x, o.y, o.z};
                icp_umeyama(S, S[29], org, MODE == ICP_MODE_P2P_SCALED, U);
            } else if (count > 0) {
                double nb6[6], x[6];
#pragma unroll
                for (int p = 0; p < 6; p++) nb6[p] = -S[21 + p];
                bool solved = icp_ldlt6_fast(S, nb6, x);
                if (!solved) {                         // rare: indefinite / semi-definite system (wave-uniform: every lane saw the same sums)
                    double *rhs = &fin[1][0];          // LDS copies (dynamic indexing must not touch scratch)
                    double *sol = &fin[2][0];
                    if (lead) {
                        for (int p = 0; p < 6; p++) rhs[p] = -S[21 + p];
                        sol[6] = icp_ldlt6_pivoted(S, rhs, sol, ldl_w, ldl_perm) ? 1.0 : 0.0;
                    }
                    __builtin_amdgcn_wave_barrier();
                    solved = sol[6] != 0.0;
                    for (int p = 0; p < 6; p++) x[p] = sol[p];
                }
                if (solved) {
                    // lane j < 3 takes angle j; the six values come back by readlane
                    const int lj = threadIdx.x;
                    const double ang = lj == 0 ? x[0] : (lj == 1 ? x[1] : x[2]);
                    union { double d; int i[2]; } sv, cv, t;
                    sv.d = sin(ang); cv.d = cos(ang);
                    auto from = [&](const decltype(sv) &v, int l) { t.i[0] = __builtin_amdgcn_readlane(v.i[0], l); t.i[1] = __builtin_amdgcn_readlane(v.i[1], l); return t.d; };
                    const double sa = from(sv, 0), ca = from(cv, 0), sb = from(sv, 1), cb = from(cv, 1), sg = from(sv, 2), cg = from(cv, 2);
                    U[0] = cg * cb; U[1] = cg * sb * sa - sg * ca; U[2] = cg * sb * ca + sg * sa; U[3] = x[3];
                    U[4] = sg * cb; U[5] = sg * sb * sa + cg * ca; U[6] = sg * sb * ca - cg * sa; U[7] = x[4];
                    U[8] = -sb;     U[9] = cb * sa;                U[10] = cb * ca;               U[11] = x[5];
                }
            }
            if (lead) {
                double Tn[16];
                for (int r = 0; r < 4; r++)
                    for (int c = 0; c < 4; c++) {
                        double s = 0;
                        for (int k = 0; k < 4; k++) s += U[r * 4 + k] * (k < 3 ? T[k * 4 + c] : (c == 3 ? 1.0 : 0.0));
                        Tn[r * 4 + c] = s;
                    }
                for (int k = 0; k < 16; k++) st->T[k] = Tn[k];
                st->iter = iter_prev + 1;
            }
        }
        if (lead) {
            st->launches = launches + 1;
            st->converged = conv ? 1 : 0;
            __hip_atomic_store(&st->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            st->ns = ns;
            st->t_live += wall_clock64() - t0k;
            st->done = stop ? 1 : 0;          // visible to the next launch through the kernel boundary
        }
        if (a.ms_scales > 0 && stop) {        // (wave-uniform) the scale is over: keep its result; not the last one: the pair goes on by itself
            __builtin_amdgcn_wave_barrier();
            const bool more = a.ms_index + 1 < a.ms_scales;
            const IcpArgs *next = a.ms_args + (a.ms_index + 1); IcpArgs *self = a.ms_self; IcpState *hist = a.ms_hist + a.ms_index;
            if (lead) {
                __threadfence();
                *hist = *st;
                if (more) {
                    st->launches = 0; st->iter = 0; st->converged = 0; st->done = 0; st->fitness = 0; st->rmse = 0; st->count = 0;
                    st->dfit = 1e300; st->drmse = 1e300;
                }
            }
            if (more) {                        // the argument slot, a dword per lane and round (nobody reads it any more in this launch: the other workgroups have left)
                const unsigned *srcw = reinterpret_cast<const unsigned *>(next); unsigned *dstw = reinterpret_cast<unsigned *>(self);
                for (int w = threadIdx.x; w < (int)(sizeof(IcpArgs) / 4); w += 64) dstw[w] = srcw[w];
            }
        }
    }
}

// ---- the frame of an iteration kernel that is the whole iteration (the map loops: no search kernel in front of it).  Workgroup b owns the source
// points [BS b, BS b + BS) in caller order.  The frame owns the exit of a finished loop and of surplus workgroups, the entry stamp, the pose, the
// zeroed sums and icp_finish; point(i, live, T, acc) adds the rows of source point i at the pose T into the lane's sums.  EVERY lane makes the call
// (live = i < ns), so that a body may exchange values across lanes.
template <int MODE, int BS, class Point>
__device__ static inline void icp_iter_frame(const IcpArgs &a, int ns, Point &&point) {
    IcpState *st = a.state;
    if (st->done) return;
    int nb = (ns + BS - 1) / BS;
    if (nb < 1) nb = 1;
    if ((int)blockIdx.x >= nb) return;
    const unsigned long long t_entry = wall_clock64();
    const int launches = st->launches;
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = st->T[k];
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) acc[k] = 0.0;
    const int i = blockIdx.x * BS + threadIdx.x;
    point(i, i < ns, T, acc);
    icp_finish<MODE, BS>(a, st, T, acc, nb, ns, launches, t_entry, (int)blockIdx.x);
}

__device__ static inline void icp_row6(double w, const double *J, double r, double *acc) {
    int t = 0;
#pragma unroll
    for (int p = 0; p < 6; p++) {
        const double wj = w * J[p];
#pragma unroll
        for (int q = p; q < 6; q++) acc[t++] += wj * J[q];
        acc[21 + p] += wj * r;
    }
}

static void state_to_result(const IcpState &s, pcr_result *out) {
    for (int k = 0; k < 16; k++) out->transformation[k] = s.T[k];
    out->fitness = s.fitness; out->inlier_rmse = s.rmse; out->n_correspondences = s.count;
    out->iterations = s.iter; out->converged = s.converged;
}

// ---- the graph cache.  One chunk of launches is replayed as ONE hipGraph launch: the loops are launch-bound (a 3000-point pair still takes
// 5 ms), and a graph costs one runtime call instead of 16.  The instantiated graphs are kept in the context under a key made by the loop.
static IcpGraph *icp_graph_find(pcr_context *ctx, const std::string &key) {
    for (auto &g : ctx->icp_graphs) if (g.key == key) return &g;
    return nullptr;
}
// the kernel nodes of a captured chunk in launch order (for hipGraphExecKernelNodeSetParams): the chunk is a chain, walked from its root
static int icp_graph_collect_nodes(pcr_context *ctx, IcpGraph &e, size_t expect) {
    size_t nr = 1; hipGraphNode_t node = nullptr;
    PCR_HIP_CHECK(ctx, hipGraphGetRootNodes(e.graph, &node, &nr));
    if (nr != 1) { ctx->err = "GICP group: captured chunk has more than one root"; return PCR_EHIP; }
    while (node) {
        hipGraphNodeType nt;
        PCR_HIP_CHECK(ctx, hipGraphNodeGetType(node, &nt));
        if (nt != hipGraphNodeTypeKernel) { ctx->err = "GICP group: captured chunk holds a node that is not a kernel"; return PCR_EHIP; }
        e.nodes.push_back(node);
        size_t nd = 0;
        PCR_HIP_CHECK(ctx, hipGraphNodeGetDependentNodes(node, nullptr, &nd));
        if (nd == 0) break;
        if (nd != 1) { ctx->err = "GICP group: captured chunk is not a chain"; return PCR_EHIP; }
        hipGraphNode_t next = nullptr;
        PCR_HIP_CHECK(ctx, hipGraphNodeGetDependentNodes(node, &next, &nd));
        node = next;
    }
    if (e.nodes.size() != expect) { ctx->err = "GICP group: captured chunk does not match its launch list"; return PCR_EHIP; }
    return PCR_OK;
}
// Captures enqueue(0) ... enqueue(len - 1) on the context's stream, instantiates the graph and stores it under `key`; expect_nodes > 0: its node
// list is collected too and must have that many kernels.  *out is valid until the cache is next changed.
template <class Enqueue>
static int icp_graph_capture(pcr_context *ctx, const std::string &key, int len, size_t expect_nodes, Enqueue &&enqueue, IcpGraph **out) {
    IcpGraph e; e.key = key;
    // (the graph objects belong to `e` until it is stored: an early error return below must not leak them)
    struct Owner { IcpGraph *g; ~Owner() { if (g) { if (g->exec) (void)hipGraphExecDestroy(g->exec); if (g->graph) (void)hipGraphDestroy(g->graph); } } } owner{&e};
    PCR_HIP_CHECK(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    for (int k = 0; k < len; k++) enqueue(k);
    PCR_HIP_CHECK(ctx, hipStreamEndCapture(ctx->stream, &e.graph));
    PCR_HIP_CHECK(ctx, hipGraphInstantiate(&e.exec, e.graph, nullptr, nullptr, 0));
    if (expect_nodes) PCR_TRY(icp_graph_collect_nodes(ctx, e, expect_nodes));
    if (ctx->icp_graphs.size() >= 48) {           // evict the oldest entry (the stream is drained first: a replay of it may still be queued)
        PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        (void)hipGraphExecDestroy(ctx->icp_graphs[0].exec);
        if (ctx->icp_graphs[0].graph) (void)hipGraphDestroy(ctx->icp_graphs[0].graph);
        ctx->icp_graphs.erase(ctx->icp_graphs.begin());
    }
    owner.g = nullptr;                            // stored: the context owns the graph from here on
    ctx->icp_graphs.push_back(std::move(e));
    *out = &ctx->icp_graphs.back();
    return PCR_OK;
}

// ---- the chunk pump.  Launches are queued in chunks; the states after chunk c are copied back while chunk c + 1 is already queued, so the GPU
// never idles on the host.  Launches after 'done' return at their first instruction.
struct IcpPump {
    pcr_context *ctx = nullptr;
    const IcpState *st_dev = nullptr; size_t slot_bytes = 0;
    IcpState *slots[2] = {nullptr, nullptr};          // two read-back slots of G states each in the pinned window
    int cur = 0, prev = -1;
    int launched = 0;                                 // launches queued so far
    bool done = false;                                // the judge ended the loop (else: `total` launches were queued and read back)
    std::vector<int> chunk_first, chunk_last;         // launches [first, last) of every chunk; chunk c lies between prof_events 2c and 2c + 1

    int init(pcr_context *c, const IcpState *states_dev, int G) {
        ctx = c; st_dev = states_dev; slot_bytes = sizeof(IcpState) * (size_t)G;
        if (2 * slot_bytes > ctx->pinned_cap) { ctx->err = "ICP loop: pinned window too small"; return PCR_ENOMEM; }
        slots[0] = (IcpState *)ctx->pinned; slots[1] = (IcpState *)(ctx->pinned + slot_bytes);
        return PCR_OK;
    }
    // issue(k, c, ragged) queues launches k ... k + c - 1; ragged: `total` cut the chunk short of the length asked for.
    // judge(states, upto, &next) sees the states after launch upto - 1, the end of the chunk before the one just queued, and sets the length
    // of the next chunk: 0 ends the loop.  The first two chunks have first_len launches.  No more than `total` launches are queued in all.
    template <class Issue, class Judge>
    int run(int first_len, int total, Issue &&issue, Judge &&judge) {
        int want = first_len;
        for (;;) {
            const int room = total - launched, c = room < want ? (room > 0 ? room : 0) : want;
            if (c > 0) {
                const size_t n = chunk_first.size();
                if (ctx->profiling) {
                    while (ctx->prof_events.size() < 2 * (n + 1)) { hipEvent_t e; PCR_HIP_CHECK(ctx, hipEventCreate(&e)); ctx->prof_events.push_back(e); }
                    PCR_HIP_CHECK(ctx, hipEventRecord(ctx->prof_events[2 * n], ctx->stream));
                }
                PCR_TRY(issue(launched, c, c != want));
                if (ctx->profiling) PCR_HIP_CHECK(ctx, hipEventRecord(ctx->prof_events[2 * n + 1], ctx->stream));
                chunk_first.push_back(launched); chunk_last.push_back(launched + c);
                launched += c;
                PCR_HIP_CHECK(ctx, hipMemcpyAsync(slots[cur], st_dev, slot_bytes, hipMemcpyDeviceToHost, ctx->stream));
                PCR_HIP_CHECK(ctx, hipEventRecord(ctx->ev[cur], ctx->stream));
            }
            if (prev >= 0) {
                PCR_HIP_CHECK(ctx, hipEventSynchronize(ctx->ev[prev]));
                PCR_TRY(judge((const IcpState *)slots[prev], launched - c, &want));
                if (want == 0) { done = true; return PCR_OK; }
            }
            if (c == 0) return PCR_OK;
            prev = cur; cur ^= 1;
        }
    }
    // bench instrumentation: chunks whose launches were all live (before 'done'): HIP-event time / launches = launch-to-launch period;
    // issued / live launches of the loop: the rest returned at once
    int add_profile(int live) {
        for (size_t c = 0; c < chunk_first.size(); c++) {
            if (chunk_last[c] > live) continue;
            float ms = 0;
            PCR_HIP_CHECK(ctx, hipEventElapsedTime(&ms, ctx->prof_events[2 * c], ctx->prof_events[2 * c + 1]));
            ctx->prof[0] += ms; ctx->prof[1] += chunk_last[c] - chunk_first[c];
        }
        ctx->prof[5] += launched; ctx->prof[13] += live;
        return PCR_OK;
    }
};

// ---- the host side of a map loop: RegistrationICP's loop with ONE kernel per iteration (an icp_iter_frame kernel of LIN_BS lanes) and nothing to
// prepare -- no imported source, no tree, no certificates -- pumped in chunks that replay as cached graphs.  The caller checks what is its own,
// zeroes both argument blocks with memset and fills them (loss, criteria and max_it in `a`; the rest is set here); launch(nb) enqueues one
// iteration of nb workgroups on the context's stream.  Every launch of a chunk is the same launch: one graph per chunk length, under the key
// (bytes of a, bytes of the second block, {nb, chunk length, tag}) -- `tag` names the KERNEL, so two kernel forms never share a cached graph.
// single: linearise once at T0 and stop, no graph; *sums then receives the NV sums (out is not written).
template <class Launch>
static int icp_map_loop(pcr_context *ctx, const char *call, IcpArgs &a, const void *block, size_t block_bytes, int ns, int tag, Launch &&launch, const double *T0, bool single,
                        pcr_result *out, double *sums) {
    const std::string who(call);
    ArenaMark mark(ctx);
    int chunk = 8; bool graph = true;
    pcr_icp_loop_switches(&chunk, &graph);
    const int nb = ns > 0 ? (ns + LIN_BS - 1) / LIN_BS : 1;
    IcpState *st = arena<IcpState>(ctx, 1);
    double *partials = arena<double>(ctx, (size_t)nb * NVP);
    if (!st || !partials) return PCR_ENOMEM;
    a.state = st; a.partials = partials; a.src_cap = ns > 0 ? ns : 1; a.grid.L = -1; a.single = single ? 1 : 0;
    IcpInit in; memcpy(in.T, T0, sizeof in.T);
    PCR_LAUNCH(ctx, k_icp_init, dim3(1), dim3(64), 0, ctx->stream, st, in);
    auto enqueue = [&](int) { launch(nb); };
    IcpState fin;
    if (single) {
        enqueue(0);
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(&fin, st, sizeof fin, hipMemcpyDeviceToHost, ctx->stream));
        PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        if (!fin.done) { ctx->err = who + ": the launch left no sums"; return PCR_EHIP; }
        if (sums) memcpy(sums, fin.sums, sizeof(double) * NV);
        return PCR_OK;
    }
    auto issue = [&](int k, int c, bool ragged) -> int {
        hipGraphExec_t ge = nullptr;
        if (graph && !ragged) {
            std::string key((const char *)&a, sizeof a);
            key.append((const char *)block, block_bytes);
            const int extra[3] = {nb, c, tag};
            key.append((const char *)extra, sizeof extra);
            IcpGraph *hit = icp_graph_find(ctx, key);
            if (!hit) {
                PCR_TRY(icp_graph_capture(ctx, key, c, 0, enqueue, &hit));
                (void)hipGraphDestroy(hit->graph); hit->graph = nullptr;      // no node of it is patched later: the instantiated graph is all that is kept
            }
            ge = hit->exec;
        }
        if (ge) PCR_HIP_CHECK(ctx, hipGraphLaunch(ge, ctx->stream));
        else for (int i = 0; i < c; i++) enqueue(k + i);
        return PCR_OK;
    };
    auto judge = [&](const IcpState *s, int, int *next) -> int {
        if (s->done) { fin = *s; *next = 0; }
        else *next = chunk;
        return PCR_OK;
    };
    IcpPump pump;
    PCR_TRY(pump.init(ctx, st, 1));
    PCR_TRY(pump.run(chunk, a.max_it + 1, issue, judge));
    if (!pump.done) { ctx->err = who + ": the loop ended without a final state"; return PCR_EHIP; }
    PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));          // the launches after 'done' return at once; the arena and the pinned slots are free again
    state_to_result(fin, out);
    for (int k = 0; k < 16; k++) if (!std::isfinite(fin.T[k])) { ctx->err = who + ": non-finite pose"; return PCR_ENUMERIC; }
    return PCR_OK;
}
