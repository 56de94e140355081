// pcr_place.hip -- Scan Context place recognition on gfx950 (Kim and Kim, IROS 2018; include/pcr_hip.h states the rules DESCRIPTOR and DISTANCE).
//   pcr_scan_context            k_sc_cells: every workgroup keeps a private R x S tile of cell maxima in LDS (atomic maximum on the ordered-integer
//                               image of the float32 value, 0 = no row yet), takes its rows grid-strided and merges the occupied cells into the
//                               global tile with one atomic maximum per cell; the three row counts go the same way (integer adds).  k_sc_finish
//                               turns the ordered integers back into floats.  A maximum does not depend on the order of its operands and the
//                               counts are integers, so every run gives the same bits.  No transcendental decides a bin: rings by comparing
//                               rho^2 against the host's table of squared bounds, sectors by the quadrant and by comparing v cos_k against
//                               u sin_k with the host's tables.
//   pcr_scan_context_distance   k_sc_distance: one workgroup per (query row, tile of SCD_BROWS candidate rows).  Both descriptors sit in LDS as
//                               float32.  The S x S matrix of column cosines is formed once per pair, SCD_JC query columns at a time (2 x 4
//                               register tiles, the sum over the rings in ring order inside one thread), and thread n adds its circular diagonal
//                               of each chunk in ascending column order; the arg-min over the shifts takes the smaller shift on a tie.
// Contraction is off in the whole unit: every product and every sum is rounded once, as the numpy restatement (tests/scan_context_reference.py)
// rounds them.  sqrt and the division of float64 are correctly rounded on this target.
#pragma clang fp contract(off)
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include "pcr_device.h"

#define SC_MAX_RINGS 64
#define SC_MAX_SECTORS 128
#define SC_TB 256                      // threads of a k_sc_cells workgroup
#define SC_ROWS_PER_WG 2048            // rows a workgroup takes before another one is added ...
#define SC_MAX_WGS 256                 // ... up to one workgroup per compute unit
#define SC_MAX_POINTS 0x7fffffffLL
#define SCD_TB 256                     // threads of a k_sc_distance workgroup
#define SCD_JC 32                      // query columns of the cosine matrix held in LDS at a time (64 was tried at up to 64 sectors: the larger
                                       // tile costs occupancy, 15.5 against 11.7 ms for 1024 x 1024 pairs at the defaults)
#define SCD_BROWS 8                    // candidate rows per workgroup

struct ScArgs {                        // by value: the tables are read through scalar loads
    int R, S;
    float h;
    double L2;
    double ring_bound2[SC_MAX_RINGS - 1];
    double cos_k[SC_MAX_SECTORS / 4 - 1], sin_k[SC_MAX_SECTORS / 4 - 1];
};
struct ScCounts { unsigned long long used, nonfinite, range, pad; };

// the ordered-integer image of a float: a < b as floats <=> key(a) < key(b) as unsigned, -0.0 just below +0.0; no finite or infinite value maps to 0
__device__ static inline unsigned sc_key(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ static inline float sc_value(unsigned k) {
    if (k == 0u) return 0.0f;                                        // a cell without rows
    const float v = __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
    return v == 0.0f ? 0.0f : v;                                     // a maximum of -0.0 is stored as +0.0
}

__global__ void __launch_bounds__(SC_TB) k_sc_cells(const float *__restrict__ xyz, int n, ScArgs a, unsigned *cells, ScCounts *counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned sc_tile[];
    __shared__ unsigned cnt[3];
    const int RS = a.R * a.S, quarter = a.S >> 2;
    for (int c = threadIdx.x; c < RS; c += SC_TB) sc_tile[c] = 0u;
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0u;
    __syncthreads();
    unsigned used = 0, nonfinite = 0, range = 0;
    for (long long i = (long long)blockIdx.x * SC_TB + threadIdx.x; i < n; i += (long long)gridDim.x * SC_TB) {
        const float fx = xyz[i * 3], fy = xyz[i * 3 + 1], fz = xyz[i * 3 + 2];
        if (!(isfinite(fx) && isfinite(fy) && isfinite(fz))) { nonfinite++; continue; }
        const double x = (double)fx, y = (double)fy;
        const double rho2 = x * x + y * y;                          // the squares of float32 values are exact in float64
        if (rho2 >= a.L2 || rho2 == 0.0) { range++; continue; }
        int ring = 0;
        for (int k = 0; k < a.R - 1; k++) ring += rho2 >= a.ring_bound2[k] ? 1 : 0;
        int q; double u, v;
        if (x > 0.0 && y >= 0.0) { q = 0; u = x; v = y; }
        else if (x <= 0.0 && y > 0.0) { q = 1; u = y; v = -x; }
        else if (x < 0.0 && y <= 0.0) { q = 2; u = -x; v = -y; }
        else { q = 3; u = -y; v = x; }
        int within = 0;
        for (int k = 0; k < quarter - 1; k++) within += v * a.cos_k[k] >= u * a.sin_k[k] ? 1 : 0;
        const int cell = ring * a.S + q * quarter + within;         // ring <= R - 1, within <= S / 4 - 1: inside the tile
        atomicMax(&sc_tile[cell], sc_key(fz + a.h));
        used++;
    }
    if (used) atomicAdd(&cnt[0], used);
    if (nonfinite) atomicAdd(&cnt[1], nonfinite);
    if (range) atomicAdd(&cnt[2], range);
    __syncthreads();
    for (int c = threadIdx.x; c < RS; c += SC_TB) {
        const unsigned k = sc_tile[c];
        if (k) atomicMax(&cells[c], k);
    }
    if (threadIdx.x == 0) {
        if (cnt[0]) atomicAdd(&counts->used, (unsigned long long)cnt[0]);
        if (cnt[1]) atomicAdd(&counts->nonfinite, (unsigned long long)cnt[1]);
        if (cnt[2]) atomicAdd(&counts->range, (unsigned long long)cnt[2]);
    }
}

__global__ void __launch_bounds__(SC_TB) k_sc_finish(const unsigned *__restrict__ cells, int RS, float *__restrict__ desc) {
    const int c = blockIdx.x * SC_TB + threadIdx.x;
    if (c < RS) desc[c] = sc_value(cells[c]);
}

// ------------------------------------------------------------------------------------------------------------ distance
struct ScdBest { double d; int n; };
__device__ static inline ScdBest scd_better(const ScdBest a, const ScdBest b) { return (b.d < a.d || (b.d == a.d && b.n < a.n)) ? b : a; }

// sqrt of the squared norm of every column of a descriptor in LDS (0 for an empty column: the column is not valid)
__device__ static inline void scd_norms(const float *__restrict__ s, int R, int S, double *__restrict__ q) {
    if ((int)threadIdx.x < S) {
        double nn = 0.0;
        for (int r = 0; r < R; r++) { const double v = (double)s[r * S + threadIdx.x]; nn += v * v; }
        q[threadIdx.x] = nn > 0.0 ? sqrt(nn) : 0.0;
    }
}

__global__ void __launch_bounds__(SCD_TB) k_sc_distance(const float *__restrict__ descA, const float *__restrict__ descB, int nB, int R, int S, int tilesB,
                                                       double *__restrict__ out_dist, int *__restrict__ out_shift) {
    extern __shared__ __attribute__((aligned(16))) char scd_lds[];
    __shared__ double red_d[2];
    __shared__ int red_n[2];
    const int RS = R * S, quarter = S >> 2;
    double *Cc = (double *)scd_lds;                       // [SCD_JC][S]: the cosine of a valid column pair, NaN for a pair that is not valid
    double *qA = Cc + SCD_JC * S, *qB = qA + S;           // [S] each
    float *sA = (float *)(qB + S), *sB = sA + RS;         // [R][S] each; every offset is a multiple of 16 bytes (S is a multiple of 4)
    const int a = blockIdx.x / tilesB, tb = blockIdx.x - a * tilesB;
    const int b_lo = tb * SCD_BROWS, b_hi = min(nB, b_lo + SCD_BROWS);
    const int tid = threadIdx.x;
    for (int i = tid; i < RS; i += SCD_TB) sA[i] = descA[(size_t)a * RS + i];
    __syncthreads();
    scd_norms(sA, R, S, qA);
    for (int b = b_lo; b < b_hi; b++) {
        __syncthreads();                                  // the previous candidate's readers are done (and qA is written)
        for (int i = tid; i < RS; i += SCD_TB) sB[i] = descB[(size_t)b * RS + i];
        __syncthreads();
        scd_norms(sB, R, S, qB);
        __syncthreads();
        double sum = 0.0; int m = 0;                      // of shift n = tid
        for (int j0 = 0; j0 < S; j0 += SCD_JC) {
            const int jc = min(SCD_JC, S - j0);           // a multiple of 4
            const int tiles = (jc >> 1) * quarter;
            for (int t = tid; t < tiles; t += SCD_TB) {
                const int tj = t / quarter, jp = 4 * (t - tj * quarter), j = j0 + 2 * tj;
                double g[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
                for (int r = 0; r < R; r++) {             // r ascending: the order of the sums of the rule
                    const float2 av = *(const float2 *)&sA[r * S + j];
                    const float4 bv = *(const float4 *)&sB[r * S + jp];
                    const double ad[2] = {(double)av.x, (double)av.y};
                    const double bd[4] = {(double)bv.x, (double)bv.y, (double)bv.z, (double)bv.w};
#pragma unroll
                    for (int i = 0; i < 2; i++)
#pragma unroll
                        for (int k = 0; k < 4; k++) g[i][k] += ad[i] * bd[k];
                }
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const double qa = qA[j + i], qb = qB[jp + k];
                        Cc[(2 * tj + i) * S + jp + k] = (qa > 0.0 && qb > 0.0) ? g[i][k] / (qa * qb) : (double)NAN;
                    }
            }
            __syncthreads();
            if (tid < S) {
                int jp = j0 - tid;
                if (jp < 0) jp += S;
#pragma unroll 4
                for (int jl = 0; jl < jc; jl++) {         // j ascending; the loads do not wait for the sum
                    const double c = Cc[jl * S + jp];
                    const bool ok = c == c;               // (a valid cosine of finite descriptors is never NaN)
                    sum = ok ? sum + c : sum;
                    m += ok ? 1 : 0;
                    jp = jp + 1 == S ? 0 : jp + 1;
                }
            }
            __syncthreads();
        }
        ScdBest best = {(double)INFINITY, INT_MAX};
        if (tid < S) { best.d = m > 0 ? 1.0 - sum / (double)m : 1.0; best.n = tid; }
        if (tid < 2 * PCR_WAVE) {                         // S <= 128: the shifts live in the first two wavefronts
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const ScdBest other = {__shfl_down(best.d, o, PCR_WAVE), __shfl_down(best.n, o, PCR_WAVE)};
                best = scd_better(best, other);
            }
            if ((tid & (PCR_WAVE - 1)) == 0) { red_d[tid >> 6] = best.d; red_n[tid >> 6] = best.n; }
        }
        __syncthreads();
        if (tid == 0) {
            const ScdBest w0 = {red_d[0], red_n[0]}, w1 = {red_d[1], red_n[1]};
            const ScdBest r = scd_better(w0, w1);
            out_dist[(size_t)a * nB + b] = r.d;
            out_shift[(size_t)a * nB + b] = r.n;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
static const char *sc_check_shape(int R, int S) {
    if (R < 1 || R > SC_MAX_RINGS) return "num_rings outside 1..64";
    if (S < 4 || S > SC_MAX_SECTORS) return "num_sectors outside 4..128";
    if (S % 4) return "num_sectors is not a multiple of 4";
    return nullptr;
}

extern "C" int pcr_scan_context(pcr_context *ctx, const float *xyz, int64_t n, const pcr_scan_context_params *params, const pcr_scan_context_tables *tables,
                                float *out_desc, pcr_scan_context_info *out_info) {
    return pcr_api_call(ctx, [&]() -> int {
        if (out_info) memset(out_info, 0, sizeof *out_info);
        if (!params || !tables) { ctx->err = "scan_context: missing parameters or tables"; return PCR_EINVAL; }
        const int R = params->num_rings, S = params->num_sectors;
        if (const char *bad = sc_check_shape(R, S)) { ctx->err = std::string("scan_context: ") + bad; return PCR_EINVAL; }
        if (!std::isfinite(params->max_range) || !(params->max_range > 0.0)) { ctx->err = "scan_context: max_range must be finite and > 0"; return PCR_EINVAL; }
        if (!std::isfinite(params->height_offset) || !std::isfinite((float)params->height_offset)) { ctx->err = "scan_context: height_offset must be finite"; return PCR_EINVAL; }
        if (!std::isfinite(tables->range2) || !(tables->range2 > 0.0)) { ctx->err = "scan_context: the squared range of the tables must be finite and > 0"; return PCR_EINVAL; }
        if ((R > 1 && !tables->ring_bound2) || (S > 4 && (!tables->cos_k || !tables->sin_k))) { ctx->err = "scan_context: missing table"; return PCR_EINVAL; }
        if (n < 0 || n > SC_MAX_POINTS) { ctx->err = "scan_context: n is negative or over the int limit"; return PCR_EINVAL; }
        if (!out_desc) { ctx->err = "scan_context: no descriptor output"; return PCR_EINVAL; }
        if (n > 0 && !xyz) { ctx->err = "scan_context: null cloud pointer"; return PCR_EINVAL; }
        ScArgs a;
        memset(&a, 0, sizeof a);
        a.R = R; a.S = S; a.h = (float)params->height_offset; a.L2 = tables->range2;
        for (int k = 0; k < R - 1; k++) a.ring_bound2[k] = tables->ring_bound2[k];
        for (int k = 0; k < S / 4 - 1; k++) { a.cos_k[k] = tables->cos_k[k]; a.sin_k[k] = tables->sin_k[k]; }
        for (int k = 0; k < R - 1; k++)
            if (!(a.ring_bound2[k] > 0.0) || (k > 0 && !(a.ring_bound2[k] >= a.ring_bound2[k - 1]))) { ctx->err = "scan_context: ring_bound2 must be positive and ascending"; return PCR_EINVAL; }
        const int RS = R * S;
        PCR_TRY(pcr_arena_reserve(ctx, (size_t)RS * sizeof(unsigned) + sizeof(ScCounts) + (1u << 12)));
        unsigned *cells = arena<unsigned>(ctx, (size_t)RS);
        ScCounts *counts = arena<ScCounts>(ctx, 1);
        if (!cells || !counts) return PCR_ENOMEM;
        PCR_HIP_CHECK(ctx, hipMemsetAsync(cells, 0, (size_t)RS * sizeof(unsigned), ctx->stream));
        PCR_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, sizeof(ScCounts), ctx->stream));
        if (n > 0) {
            const int wgs = (int)std::min<int64_t>(SC_MAX_WGS, (n + SC_ROWS_PER_WG - 1) / SC_ROWS_PER_WG);
            PCR_LAUNCH(ctx, k_sc_cells, dim3(wgs), dim3(SC_TB), (size_t)RS * sizeof(unsigned), ctx->stream, xyz, (int)n, a, cells, counts);
        }
        PCR_LAUNCH(ctx, k_sc_finish, dim3((RS + SC_TB - 1) / SC_TB), dim3(SC_TB), 0, ctx->stream, (const unsigned *)cells, RS, out_desc);
        if (out_info) {
            ScCounts h;
            PCR_HIP_CHECK(ctx, hipMemcpyAsync(&h, counts, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
            PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            out_info->used = (int64_t)h.used; out_info->dropped_nonfinite = (int64_t)h.nonfinite; out_info->dropped_range = (int64_t)h.range;
        }
        return PCR_OK;
    });
}

extern "C" int pcr_scan_context_distance(pcr_context *ctx, const float *descA, int64_t nA, const float *descB, int64_t nB, int R, int S, double *out_dist,
                                         int32_t *out_shift) {
    return pcr_api_call(ctx, [&]() -> int {
        if (const char *bad = sc_check_shape(R, S)) { ctx->err = std::string("scan_context_distance: ") + bad; return PCR_EINVAL; }
        if (nA < 0 || nB < 0) { ctx->err = "scan_context_distance: negative row count"; return PCR_EINVAL; }
        if (nA == 0 || nB == 0) return PCR_OK;
        if (!descA || !descB || !out_dist || !out_shift) { ctx->err = "scan_context_distance: null pointer"; return PCR_EINVAL; }
        const int64_t tilesB = (nB + SCD_BROWS - 1) / SCD_BROWS;
        if (nB > INT_MAX || nA > INT_MAX || nA * tilesB > INT_MAX) { ctx->err = "scan_context_distance: the block is too large for one call (rows x row tiles over the int limit)"; return PCR_EINVAL; }
        const size_t lds = (size_t)(SCD_JC + 2) * S * sizeof(double) + 2 * (size_t)R * S * sizeof(float);
        if (lds > 48 * 1024) PCR_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)k_sc_distance, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        PCR_LAUNCH(ctx, k_sc_distance, dim3((unsigned)(nA * tilesB)), dim3(SCD_TB), lds, ctx->stream, descA, descB, (int)nB, R, S, (int)tilesB, out_dist, out_shift);
        return PCR_OK;
    });
}
