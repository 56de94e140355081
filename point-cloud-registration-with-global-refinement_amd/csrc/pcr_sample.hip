// pcr_sample.hip -- farthest point sampling on gfx950: PointCloud.farthest_point_down_sample of Open3D as ONE sequential loop of num_samples
// dependent steps (include/pcr_hip.h states the rules DIST, INIT, STEP and RESULT).  A step is a distance update over all rows followed by a
// global arg-max with ties to the smaller index; both forms below run exactly that and give the same bits:
//   step form        k_fps_init, then ONE launch of k_fps_step per sample: every workgroup updates its rows' running distance in global memory,
//                    reduces them to one (distance, index) record and takes a ticket; the workgroup whose ticket is last reduces the records and
//                    writes the next sample and the loop state.  Nobody waits for anybody; the launches are enqueued back to back.
//   persistent form  k_fps_persist: ONE launch of G co-resident workgroups runs all steps.  A workgroup keeps its slice of the cloud in LDS
//                    (x, y, z float and the running distance double, 20 B per point; rows that do not fit stay in global memory and only this
//                    workgroup touches them).  Per step: update the slice, wavefront and workgroup arg-max, publish the record into a slot
//                    chosen by step parity, arrive at a monotonic counter, wait, gather the G records and reduce them in every workgroup.
//                    The hand-off is that of d_fgr_opt_multi (pcr_fgr.hip): agent-scope relaxed stores and loads, s_waitcnt vmcnt(0) before
//                    arriving, s_sleep in the poll, and a tick limit after which the waiter sets `failed` and every wave exits; the host then
//                    repeats the call in the step form.  G = 1 is the same kernel without the wait.
// max over (distance, smaller index first) is a total order, so the answer does not depend on how rows are dealt to lanes, wavefronts or
// workgroups.  Every loop is bounded by a count or by the tick limit; no float atomics.  Contraction is off: d^2 has the bits of a host
// recomputation (the rule of pcr_search.hip).
#pragma clang fp contract(off)
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include "pcr_device.h"

#define FPS_TB 512                     // threads of a persistent workgroup
#define FPS_SB 256                     // threads of a step-form workgroup
#define FPS_STEP_ROWS 4                // rows per thread of the step form: 1024 rows per workgroup
#define FPS_MAX_WGS 256                // persistent workgroups: at most one per CU
#define FPS_LDS_SCRATCH 256            // bytes of reduction scratch in front of the slice (two record sets of FPS_TB / 64 wavefronts + the bail word)
#define FPS_LDS_POINT 20               // bytes of LDS per resident point
#define FPS_LDS_MAX (160 * 1024)       // LDS a workgroup may take on gfx950
#define FPS_MAX_POINTS 0x7fffffffLL    // the clouds of this library are counted in int
static_assert(FPS_MAX_WGS <= FPS_TB, "one gathered record per thread");

struct FpsState {                      // zeroed by a memset before every run of either form; the host reads it once at the end
    unsigned long long arrive;         // persistent form: the monotonic barrier counter
    unsigned long long cover_bits;     // m after the last step (bits of a double >= 0)
    int failed;                        // persistent form: a workgroup gave up waiting (co-residency not granted): the host reruns in the step form
    unsigned int ticket;               // step form
    int bad_start;                     // start_index names a row with a non-finite coordinate
    int cur;
    int pad[4];
};
static_assert(sizeof(FpsState) % 16 == 0, "the memset covers whole 16-byte words");

struct FpsBest { double d; int i; };   // running maximum (starting from 0) and the smallest row that holds it (INT_MAX: none)
__device__ static inline FpsBest fps_better(const FpsBest a, const FpsBest b) { return (b.d > a.d || (b.d == a.d && b.i < a.i)) ? b : a; }

// d^2 of DIST: float64 on the float32 coordinates, differences, squares and sums in the order x, y, z, each rounded once
__device__ static inline double fps_d2(float x, float y, float z, double cx, double cy, double cz) {
#pragma clang fp contract(off)
    const double ex = (double)x - cx, ey = (double)y - cy, ez = (double)z - cz;
    double d2 = ex * ex;
    d2 += ey * ey;
    d2 += ez * ez;
    return d2;
}
__device__ static inline bool fps_finite(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }
// one row of STEP: the new running distance (a row at -1 stays there) folded into the thread's best; rows come in ascending order, the test is strict
__device__ static inline double fps_update(double old, double d2, int j, FpsBest &b) {
    const double nd = old < 0.0 ? old : (d2 < old ? d2 : old);
    if (nd > b.d) { b.d = nd; b.i = j; }
    return nd;
}

// ---- wavefront reductions inside the VALU (DPP within the 16-lane rows, permlane swaps across them); every lane gets the result
template <int CTRL> __device__ static inline double fps_dpp_d(double v) {
    union { double d; int i[2]; } a, b;
    a.d = v; b.i[0] = pcr_dpp_i<CTRL>(a.i[0]); b.i[1] = pcr_dpp_i<CTRL>(a.i[1]);
    return b.d;
}
__device__ static inline double fps_wave_max(double v) {            // values >= 0, never NaN
    v = fmax(v, fps_dpp_d<PCR_DPP_XOR1>(v)); v = fmax(v, fps_dpp_d<PCR_DPP_XOR2>(v));
    v = fmax(v, fps_dpp_d<PCR_DPP_HMIRROR>(v)); v = fmax(v, fps_dpp_d<PCR_DPP_MIRROR>(v));
    union { double d; unsigned u[2]; } a, o;
    a.d = v; a.u[0] = pcr_swap16(a.u[0], &o.u[0]); a.u[1] = pcr_swap16(a.u[1], &o.u[1]); v = fmax(a.d, o.d);
    a.d = v; a.u[0] = pcr_swap32(a.u[0], &o.u[0]); a.u[1] = pcr_swap32(a.u[1], &o.u[1]);
    return fmax(a.d, o.d);
}
__device__ static inline int fps_wave_min_i(int v) {
    v = min(v, pcr_dpp_i<PCR_DPP_XOR1>(v)); v = min(v, pcr_dpp_i<PCR_DPP_XOR2>(v));
    v = min(v, pcr_dpp_i<PCR_DPP_HMIRROR>(v)); v = min(v, pcr_dpp_i<PCR_DPP_MIRROR>(v));
    unsigned o; unsigned a = pcr_swap16((unsigned)v, &o);
    v = min((int)a, (int)o);
    a = pcr_swap32((unsigned)v, &o);
    return min((int)a, (int)o);
}
// arg-max over the workgroup, ties to the smaller index at both levels; all threads call it and all get the result.  sd / si: NW entries of LDS
// that nobody reads any more (the callers alternate between two sets, with a workgroup barrier between two uses of the same set).
template <int NW> __device__ static inline FpsBest fps_block_best(const FpsBest b, double *sd, int *si) {
    const double m = fps_wave_max(b.d);
    const int i = fps_wave_min_i(b.d == m ? b.i : INT_MAX);
    if ((threadIdx.x & (PCR_WAVE - 1)) == 0) { sd[threadIdx.x >> 6] = m; si[threadIdx.x >> 6] = i; }
    __syncthreads();
    FpsBest r = {sd[0], si[0]};
#pragma unroll
    for (int w = 1; w < NW; w++) { const FpsBest o = {sd[w], si[w]}; r = fps_better(r, o); }
    return r;
}
__device__ static inline void fps_store_record(unsigned long long *rec, const FpsBest b) {
    __hip_atomic_store(&rec[0], (unsigned long long)__double_as_longlong(b.d), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&rec[1], (unsigned long long)(unsigned int)b.i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ static inline FpsBest fps_load_record(unsigned long long *rec) {
    const unsigned long long k = __hip_atomic_load(&rec[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long i = __hip_atomic_load(&rec[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const FpsBest b = {__longlong_as_double((long long)k), (int)(unsigned int)i};
    return b;
}

// ------------------------------------------------------------------------------------------------------------ step form
__global__ void __launch_bounds__(FPS_SB) k_fps_init(const float *__restrict__ xyz, int n, int start, double *__restrict__ dist, FpsState *st, long long *__restrict__ sel) {
    const int j = blockIdx.x * FPS_SB + threadIdx.x;
    if (j < n) dist[j] = fps_finite(xyz[(size_t)j * 3], xyz[(size_t)j * 3 + 1], xyz[(size_t)j * 3 + 2]) ? (double)INFINITY : -1.0;
    if (j == 0) {
        const bool ok = fps_finite(xyz[(size_t)start * 3], xyz[(size_t)start * 3 + 1], xyz[(size_t)start * 3 + 2]);
        st->cur = start; st->bad_start = ok ? 0 : 1;
        if (ok) sel[0] = start;
    }
}

// step i: distances against row st->cur, the next sample into sel[i + 1] (if there is one) and into the state
__global__ void __launch_bounds__(FPS_SB) k_fps_step(const float *__restrict__ xyz, int n, double *__restrict__ dist, FpsState *st, unsigned long long *recs,
                                                     long long *__restrict__ sel, long long i, long long num_samples) {
    __shared__ double sd[2][FPS_SB / PCR_WAVE];
    __shared__ int si[2][FPS_SB / PCR_WAVE];
    __shared__ int is_last;
    if (st->bad_start) return;
    const int cur = st->cur;            // (written by the previous launch; the workgroup that rewrites it below is the last to have read it)
    const double cx = (double)xyz[(size_t)cur * 3], cy = (double)xyz[(size_t)cur * 3 + 1], cz = (double)xyz[(size_t)cur * 3 + 2];
    FpsBest b = {0.0, INT_MAX};
    const long long base = (long long)blockIdx.x * (FPS_SB * FPS_STEP_ROWS) + threadIdx.x;
#pragma unroll
    for (int r = 0; r < FPS_STEP_ROWS; r++) {
        const long long j = base + (long long)r * FPS_SB;
        if (j < n) dist[j] = fps_update(dist[j], fps_d2(xyz[j * 3], xyz[j * 3 + 1], xyz[j * 3 + 2], cx, cy, cz), (int)j, b);
    }
    b = fps_block_best<FPS_SB / PCR_WAVE>(b, sd[0], si[0]);
    if (threadIdx.x == 0) fps_store_record(recs + 2 * (size_t)blockIdx.x, b);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the record is out before the ticket is taken
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int t = __hip_atomic_fetch_add(&st->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        is_last = (t == gridDim.x - 1);
    }
    __syncthreads();
    if (!is_last) return;
    FpsBest g = {0.0, INT_MAX};
    for (unsigned int q = threadIdx.x; q < gridDim.x; q += FPS_SB) g = fps_better(g, fps_load_record(recs + 2 * (size_t)q));
    g = fps_block_best<FPS_SB / PCR_WAVE>(g, sd[1], si[1]);
    if (threadIdx.x == 0) {
        const int next = g.d > 0.0 ? g.i : cur;
        st->cur = next; st->cover_bits = (unsigned long long)__double_as_longlong(g.d);
        if (i + 1 < num_samples) sel[i + 1] = next;
        __hip_atomic_store(&st->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ------------------------------------------------------------------------------------------------------ persistent form
struct FpsPersistArgs {
    const float *xyz; int n;
    long long num_samples; int start;
    int slice;                          // rows per workgroup: workgroup b owns [b * slice, min(n, (b + 1) * slice))
    int lds_rows;                       // the first lds_rows rows of a slice live in LDS, the rest in `dist` (and are read from xyz)
    double *dist; long long *sel; FpsState *st;
    unsigned long long *recs;           // 2 (step parity) x FPS_MAX_WGS records of two words
    unsigned long long timeout_ticks;
};
__global__ void __launch_bounds__(FPS_TB) k_fps_persist(FpsPersistArgs a) {
    extern __shared__ __attribute__((aligned(16))) char fps_lds[];
    double *rd = (double *)fps_lds;                                   // [2][FPS_TB / 64]
    int *ri = (int *)(fps_lds + 2 * (FPS_TB / PCR_WAVE) * sizeof(double));      // [2][FPS_TB / 64]
    int *bail = ri + 2 * (FPS_TB / PCR_WAVE);
    double *sd = (double *)(fps_lds + FPS_LDS_SCRATCH);
    float *sx = (float *)(sd + a.lds_rows), *sy = sx + a.lds_rows, *sz = sy + a.lds_rows;
    constexpr int NW = FPS_TB / PCR_WAVE;
    const float *__restrict__ xyz = a.xyz;
    FpsState *st = a.st;
    const int G = gridDim.x;
    int cur = a.start;
    if (!fps_finite(xyz[(size_t)cur * 3], xyz[(size_t)cur * 3 + 1], xyz[(size_t)cur * 3 + 2])) {      // every workgroup sees it and leaves
        if (blockIdx.x == 0 && threadIdx.x == 0) st->bad_start = 1;
        return;
    }
    const long long lo_l = (long long)blockIdx.x * a.slice;
    const int lo = (int)min(lo_l, (long long)a.n), cnt = min(a.slice, a.n - lo), in_lds = min(cnt, a.lds_rows);
    // INIT.  Thread t owns rows t, t + FPS_TB, ... of the slice from here to the end, in LDS and in global memory alike: no barrier is needed
    // between its own writes and reads
    for (int l = threadIdx.x; l < cnt; l += FPS_TB) {
        const size_t j = (size_t)lo + l;
        const float x = xyz[j * 3], y = xyz[j * 3 + 1], z = xyz[j * 3 + 2];
        const double d0 = fps_finite(x, y, z) ? (double)INFINITY : -1.0;
        if (l < in_lds) { sx[l] = x; sy[l] = y; sz[l] = z; sd[l] = d0; }
        else a.dist[j] = d0;
    }
    if (threadIdx.x == 0) *bail = 0;
    __syncthreads();
    double cover = 0.0;
    for (long long it = 0; it < a.num_samples; it++) {
        if (blockIdx.x == 0 && threadIdx.x == 0) a.sel[it] = cur;
        const double cx = (double)xyz[(size_t)cur * 3], cy = (double)xyz[(size_t)cur * 3 + 1], cz = (double)xyz[(size_t)cur * 3 + 2];
        FpsBest b = {0.0, INT_MAX};
#pragma unroll 4
        for (int l = threadIdx.x; l < in_lds; l += FPS_TB) sd[l] = fps_update(sd[l], fps_d2(sx[l], sy[l], sz[l], cx, cy, cz), lo + l, b);
        for (int l = in_lds + threadIdx.x; l < cnt; l += FPS_TB) {
            const size_t j = (size_t)lo + l;
            a.dist[j] = fps_update(a.dist[j], fps_d2(xyz[j * 3], xyz[j * 3 + 1], xyz[j * 3 + 2], cx, cy, cz), (int)j, b);
        }
        const int set = G > 1 ? 0 : (int)(it & 1);      // (alone, one barrier per step: the record sets alternate by step instead)
        FpsBest g = fps_block_best<NW>(b, rd + set * NW, ri + set * NW);
        if (G > 1) {
            unsigned long long *slot = a.recs + (size_t)(it & 1) * 2 * FPS_MAX_WGS;
            if (threadIdx.x == 0) fps_store_record(slot + 2 * (size_t)blockIdx.x, g);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the record is out before the workgroup arrives
            __syncthreads();
            if (threadIdx.x == 0) {
                __hip_atomic_fetch_add(&st->arrive, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long want = (unsigned long long)(it + 1) * (unsigned long long)G;
                const unsigned long long t0 = wall_clock64();
                while (__hip_atomic_load(&st->arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
                    if (wall_clock64() - t0 > a.timeout_ticks || __hip_atomic_load(&st->failed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { *bail = 1; break; }
                    __builtin_amdgcn_s_sleep(2);
                }
            }
            __syncthreads();
            if (*bail) {
                if (threadIdx.x == 0) __hip_atomic_store(&st->failed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            // one coherent record per lane; a workgroup can be at most one barrier ahead, so the slot of this parity is not rewritten before
            // every workgroup has arrived at the next barrier, after this read
            FpsBest r = {0.0, INT_MAX};
            if ((int)threadIdx.x < G) r = fps_load_record(slot + 2 * (size_t)threadIdx.x);
            g = fps_block_best<NW>(r, rd + NW, ri + NW);
        }
        if (g.d > 0.0) cur = g.i;
        cover = g.d;
    }
    for (int l = threadIdx.x; l < in_lds; l += FPS_TB) a.dist[(size_t)lo + l] = sd[l];
    if (blockIdx.x == 0 && threadIdx.x == 0) { st->cur = cur; st->cover_bits = (unsigned long long)__double_as_longlong(cover); }
}

// ------------------------------------------------------------------------------------------------------------------ host
// Which form a cloud takes and with how many workgroups.  The option "fps_form" forces a form (0 step launches, 1 persistent), "fps_wgs" the
// number of persistent workgroups, "fps_timeout" the ticks of the 100 MHz wall clock a workgroup waits at the barrier (tests set 0 to force the
// fall-back; default: that of PCR_FGR_MULTI_TIMEOUT).  Measured on an MI355X: a step of the persistent form costs the barrier --
// 3.1 us up to 32 workgroups, 3.5 at 64, 4.4 at 128, 6.2 at 256 -- plus 0.2 us per 1000 LDS rows of a slice (0.4 us per 1000 rows left in global
// memory), a step of the step form 4.7 us at 2k..20k points, 6.7 at 200k and 17.4 at 1M.  So the persistent form at every size it was measured at
// (2k .. 1M points); a cloud that fits one workgroup's LDS runs alone (1.3 us + the rows, no barrier), larger ones take one workgroup per
// FPS_ROWS_PER_WG rows up to 128, and 256 only once 128 slices no longer fit in LDS.  Above FPS_PERSIST_MAX_POINTS (the LDS of 256 workgroups)
// nothing was measured: the step form, whose grid grows with the cloud.
#define FPS_PERSIST_MAX_POINTS 2000000
#define FPS_ROWS_PER_WG 3072
#define FPS_WGS_NARROW 128
static int fps_form_for(int64_t n) {
    const int forced = pcr_options().fps_form.load(std::memory_order_relaxed);
    if (forced == 0 || forced == 1) return forced;
    return n <= FPS_PERSIST_MAX_POINTS ? 1 : 0;
}
static int fps_wgs_for(int64_t n, int cus, int lds_rows_max) {
    const int forced = pcr_options().fps_wgs.load(std::memory_order_relaxed);
    int g = forced;
    if (g <= 0) {
        if (n <= lds_rows_max) g = 1;
        else if (n <= (int64_t)FPS_WGS_NARROW * lds_rows_max) g = std::min(FPS_WGS_NARROW, std::max(2, (int)((n + FPS_ROWS_PER_WG - 1) / FPS_ROWS_PER_WG)));
        else g = FPS_MAX_WGS;
    }
    g = std::min(g, std::min(FPS_MAX_WGS, cus));          // at most one per CU: they must be co-resident
    return std::max(g, 1);
}
static unsigned long long fps_timeout() {
    const int forced = pcr_options().fps_timeout.load(std::memory_order_relaxed);
    if (forced >= 0) return (unsigned long long)forced;
    static const unsigned long long def = getenv("PCR_FGR_MULTI_TIMEOUT") ? strtoull(getenv("PCR_FGR_MULTI_TIMEOUT"), nullptr, 10) : 5000000ull;
    return def;
}

static int fps_read_state(pcr_context *ctx, const FpsState *st, FpsState *h) {
    PCR_HIP_CHECK(ctx, hipMemcpyAsync(h, st, sizeof *h, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

extern "C" int pcr_farthest_point_sample(pcr_context *ctx, const float *xyz, int64_t n, int64_t num_samples, int64_t start_index, int64_t *out_index, double *out_dist2,
                                         pcr_fps_info *info) {
    return pcr_api_call(ctx, [&]() -> int {
        if (info) memset(info, 0, sizeof *info);
        if (n < 0 || n > FPS_MAX_POINTS) { ctx->err = "farthest_point_down_sample: bad point count"; return PCR_EINVAL; }
        if (num_samples < 0 || num_samples > n) { ctx->err = "farthest_point_down_sample: num_samples must be in 0..n"; return PCR_EINVAL; }
        if (!xyz && n > 0) { ctx->err = "farthest_point_down_sample: missing cloud"; return PCR_EINVAL; }
        if (num_samples == 0) return PCR_OK;
        if (start_index < 0 || start_index >= n) { ctx->err = "farthest_point_down_sample: start_index outside 0..n-1"; return PCR_EINVAL; }
        if (!out_index) { ctx->err = "farthest_point_down_sample: no index output"; return PCR_EINVAL; }
        int cus = 0, lds_max = 0;
        PCR_HIP_CHECK(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
        PCR_HIP_CHECK(ctx, hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
        lds_max = std::min(lds_max, FPS_LDS_MAX);
        const int nb = (int)((n + FPS_SB * FPS_STEP_ROWS - 1) / (FPS_SB * FPS_STEP_ROWS));
        PCR_TRY(pcr_arena_reserve(ctx, (out_dist2 ? 0 : (size_t)n * sizeof(double)) + (size_t)(nb + 2 * FPS_MAX_WGS) * 16 + sizeof(FpsState) + (1u << 12)));
        FpsState *st = arena<FpsState>(ctx, 1);
        unsigned long long *recs = arena<unsigned long long>(ctx, (size_t)std::max(nb, 2 * FPS_MAX_WGS) * 2);
        double *dist = out_dist2 ? out_dist2 : arena<double>(ctx, (size_t)n);
        if (!st || !recs || !dist) return PCR_ENOMEM;
        static_assert(sizeof(long long) == sizeof(int64_t), "sel is written as long long");
        long long *sel = (long long *)out_index;
        FpsState h;
        int form = fps_form_for(n), fell_back = 0, workgroups = nb;
        if (form == 1) {
            FpsPersistArgs a;
            const int lds_rows_max = (lds_max - FPS_LDS_SCRATCH) / FPS_LDS_POINT;
            const int G = fps_wgs_for(n, cus, lds_rows_max);
            a.xyz = xyz; a.n = (int)n; a.num_samples = num_samples; a.start = (int)start_index;
            a.slice = (int)((n + G - 1) / G);
            a.lds_rows = std::min(a.slice, lds_rows_max);
            a.dist = dist; a.sel = sel; a.st = st; a.recs = recs; a.timeout_ticks = fps_timeout();
            const size_t lds = ((size_t)FPS_LDS_SCRATCH + (size_t)a.lds_rows * FPS_LDS_POINT + 15) & ~(size_t)15;
            if (lds > 48 * 1024) PCR_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)k_fps_persist, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            PCR_HIP_CHECK(ctx, hipMemsetAsync(st, 0, sizeof *st, ctx->stream));
            PCR_LAUNCH(ctx, k_fps_persist, dim3(G), dim3(FPS_TB), lds, ctx->stream, a);
            PCR_TRY(fps_read_state(ctx, st, &h));
            workgroups = G;
            if (h.failed) { form = 0; fell_back = 1; workgroups = nb; }      // the workgroups were not co-resident in time: the same answer, one launch per sample
        }
        if (form == 0) {
            PCR_HIP_CHECK(ctx, hipMemsetAsync(st, 0, sizeof *st, ctx->stream));
            PCR_LAUNCH(ctx, k_fps_init, dim3((unsigned)((n + FPS_SB - 1) / FPS_SB)), dim3(FPS_SB), 0, ctx->stream, xyz, (int)n, (int)start_index, dist, st, sel);
            for (int64_t i = 0; i < num_samples; i++)
                PCR_LAUNCH(ctx, k_fps_step, dim3(nb), dim3(FPS_SB), 0, ctx->stream, xyz, (int)n, dist, st, recs, sel, (long long)i, (long long)num_samples);
            PCR_TRY(fps_read_state(ctx, st, &h));
        }
        if (info) { info->form = form; info->workgroups = workgroups; info->fell_back = fell_back; }
        if (h.bad_start) { ctx->err = "farthest_point_down_sample: start_index names a row with a non-finite coordinate"; return PCR_EINVAL; }
        if (info) memcpy(&info->cover_dist2, &h.cover_bits, sizeof(double));
        return PCR_OK;
    });
}
