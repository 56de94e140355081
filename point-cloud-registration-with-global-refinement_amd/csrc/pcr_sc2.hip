// pcr_sc2.hip -- spatial-compatibility (second-order, "SC2") global registration on a correspondence list on gfx950: pcr_spatial_compatibility,
// pcr_registration_sc2_correspondence and the test hook pcr_debug_sc2_seeds.  include/pcr_hip.h states the rule; every count in it is an exact
// integer, every length the float64 expression of sc_len, so a numpy restatement gives the same bits, seeds and member rows.
//   k_sc_gather   the rows' points as float4 (the list has passed pcr_corres_check)
//   k_sc_bits     a wavefront holds 64 columns in registers and walks 64 rows (scalar loads): __ballot of the float64 test IS the word, lane 0 stores it
//   k_sc_scores   one workgroup per row i, the row in LDS: for every set bit j the lanes AND + popcount row i with row j, word by word, into per-lane
//                 sums that are reduced once -> deg_i, score_i.  The work is sum_i deg_i * W words: the lists are sparse (a fraction of a percent
//                 to a few percent of the pairs), and sparse uniformly, so that a 64 x 64 tile of C is almost never empty and a dense tiled product
//                 with tile skipping would do N * N * W of it.  Integer adds: exact in any order.
//   k_sc_keys / pcr_sort_pairs / k_sc_sorted   the order (score descending, row ascending): stable radix sort of (2^33 - 1 - score)
//   k_sc_nms      one wavefront per rank: a row is a candidate unless an earlier rank lies within nms_radius of it in the source (ballot, early exit)
//   k_sc_pick     the first candidates become the seeds
//   k_sc_seed     one workgroup per seed m, row m in LDS: SC2_mj for every set bit j, the k1 largest packed (value, ~row) keys kept sorted across the
//                 lanes of each wavefront and merged by the first; then ONE wavefront: lane a holds the mask of K1 members compatible with member a,
//                 L_ma, the k2 cut with the half-of-maximum rule, and the Umeyama fit over K2
//   ScPolicy      the seeds' hypotheses scored by the frame of pcr_hypo.h, as pcr_ransac.hip scores a round but over a dense array of seeds and
//                 with sc_d2, whose products and sums round one by one like the restatement's
//   k_sc_eval / k_sc_refit        refinement: inlier flags, count, err2 and the moments of the inlier rows under a pose in one pass, then the fit
// No floating-point atomics; no kernel waits on another workgroup; every loop is bounded by a count.
#pragma clang fp contract(off)      // x*x + y*y + z*z rounds every product and every sum once, as the restatement does
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "pcr_internal.h"
#include "pcr_umeyama.h"
#include "pcr_hypo.h"

#define SC_BS 256
#define SC_WAVES (SC_BS / 64)
#define SC_MAX_N 65536
#define SC_MAX_W (SC_MAX_N / 64)
#define SC_TILE 512                 // rows per LDS tile of the score: 6 doubles each
#define SC_SPLIT_ROWS 1024
#define SC_MAX_SPLITS 64
#define SC_NV 18                    // sums of k_sc_eval: count, err2, 16 moments
typedef unsigned long long sc_word;

__device__ static inline double sc_len(const float4 a, const float4 b) {
    const double dx = (double)a.x - (double)b.x, dy = (double)a.y - (double)b.y, dz = (double)a.z - (double)b.z;
    return sqrt(dx * dx + dy * dy + dz * dz);
}
// |T s - t|^2, float64, left to right
__device__ static inline double sc_d2(const double *T, double sx, double sy, double sz, double tx, double ty, double tz) {
    const double x = T[0] * sx + T[1] * sy + T[2] * sz + T[3] - tx;
    const double y = T[4] * sx + T[5] * sy + T[6] * sz + T[7] - ty;
    const double z = T[8] * sx + T[9] * sy + T[10] * sz + T[11] - tz;
    return x * x + y * y + z * z;
}
// a value every lane holds alike, moved to scalar registers: the loops over it are then uniform for the compiler too
__device__ static inline sc_word sc_uniform(sc_word v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((sc_word)hi << 32) | (sc_word)lo;
}
__device__ static inline int sc_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(SC_BS) k_sc_gather(const float *__restrict__ src, const float *__restrict__ tgt, const int32_t *__restrict__ corres, int N,
                                                     float4 *__restrict__ ps, float4 *__restrict__ pt) {
    const int i = blockIdx.x * SC_BS + threadIdx.x;
    if (i >= N) return;
    const int a = corres[2 * (size_t)i], b = corres[2 * (size_t)i + 1];
    ps[i] = make_float4(src[3 * (size_t)a], src[3 * (size_t)a + 1], src[3 * (size_t)a + 2], 0.f);
    pt[i] = make_float4(tgt[3 * (size_t)b], tgt[3 * (size_t)b + 1], tgt[3 * (size_t)b + 2], 0.f);
}

// grid (W, ceil(N / 256)): word blockIdx.x of 64 rows per wavefront
__global__ void __launch_bounds__(SC_BS) k_sc_bits(const float4 *__restrict__ ps, const float4 *__restrict__ pt, int N, int W, double tau, sc_word *__restrict__ bits) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int w = blockIdx.x, col = w * 64 + lane;
    const bool live = col < N;
    const float4 cs = ps[live ? col : N - 1], ct = pt[live ? col : N - 1];
    const int r0 = (blockIdx.y * SC_WAVES + wave) * 64, r1 = min(N, r0 + 64);
    for (int r = r0; r < r1; r++) {
        const double ls = sc_len(ps[r], cs), lt = sc_len(pt[r], ct);
        const bool c = live && col != r && fabs(ls - lt) < tau;
        const sc_word word = __ballot(c);
        if (lane == 0) bits[(size_t)r * W + w] = word;
    }
}

__global__ void __launch_bounds__(SC_BS) k_sc_scores(const sc_word *__restrict__ bits, int N, int W, int32_t *__restrict__ deg, long long *__restrict__ score) {
    __shared__ sc_word row[SC_MAX_W];
    __shared__ long long red[SC_WAVES];
    __shared__ int redd[SC_WAVES];
    const int i = blockIdx.x, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int k = threadIdx.x; k < W; k += SC_BS) row[k] = bits[(size_t)i * W + k];
    __syncthreads();
    long long acc = 0; int d = 0;
    for (int w = wave; w < W; w += SC_WAVES) {
        sc_word m = sc_uniform(row[w]);
        d += __popcll(m);
        while (m) {
            const int j = w * 64 + (__ffsll((long long)m) - 1);
            m &= m - 1;
            const sc_word *__restrict__ rj = bits + (size_t)j * W;
            for (int k = lane; k < W; k += 64) acc += __popcll(row[k] & rj[k]);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) { red[wave] = acc; redd[wave] = d; }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long s = 0; int dd = 0;
        for (int v = 0; v < SC_WAVES; v++) { s += red[v]; dd += redd[v]; }
        if (score) score[i] = s;
        if (deg) deg[i] = dd;
    }
}

__global__ void __launch_bounds__(SC_BS) k_sc_keys(const long long *__restrict__ score, int N, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int i = blockIdx.x * SC_BS + threadIdx.x;
    if (i >= N) return;
    keys[i] = ((1ull << 33) - 1ull) - (uint64_t)score[i];        // score <= N (N - 1) < 2^32
    vals[i] = (uint32_t)i;
}
__global__ void __launch_bounds__(SC_BS) k_sc_sorted(const float4 *__restrict__ ps, const uint32_t *__restrict__ order, int N, float4 *__restrict__ psort) {
    const int r = blockIdx.x * SC_BS + threadIdx.x;
    if (r < N) psort[r] = ps[order[r]];
}
__global__ void __launch_bounds__(SC_BS) k_sc_nms(const float4 *__restrict__ psort, const uint32_t *__restrict__ order, const long long *__restrict__ score, int N, double nms,
                                                  uint8_t *__restrict__ flag) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * SC_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= N) return;
    bool cand = score[order[r]] > 0;
    if (cand && nms > 0.0) {
        const float4 p = psort[r];
        for (int q0 = 0; q0 < r; q0 += 64) {
            const int q = q0 + lane;
            const bool hit = q < r && sc_len(psort[q], p) < nms;
            if (__ballot(hit)) { cand = false; break; }
        }
    }
    if (lane == 0) flag[r] = cand ? 1 : 0;
}
__global__ void __launch_bounds__(SC_BS) k_sc_pick(const uint32_t *__restrict__ order, const uint8_t *__restrict__ flag, const int *__restrict__ pos, int N, int S, int *__restrict__ seeds) {
    const int r = blockIdx.x * SC_BS + threadIdx.x;
    if (r < N && flag[r] && pos[r] < S) seeds[pos[r]] = (int)order[r];
}

struct ScSeedArgs {
    const sc_word *bits; const float4 *ps, *pt; int N, W, k1, k2;
    const int *seeds; int32_t *k1_rows, *k2_rows;      // [seed][64], -1 beyond the members
    double *T; uint8_t *valid;                         // [seed][12], [seed]
};
__global__ void __launch_bounds__(SC_BS) k_sc_seed(ScSeedArgs a) {
    __shared__ sc_word row[SC_MAX_W];
    __shared__ sc_word keys[SC_WAVES][64];
    const int s = blockIdx.x, m = a.seeds[s], W = a.W;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int k = threadIdx.x; k < W; k += SC_BS) row[k] = a.bits[(size_t)m * W + k];
    __syncthreads();
    // lane l holds the l-th largest key (SC2_mj << 32 | ~j) this wavefront has seen; 0 = empty (a key's low half is never 0: j < 2^32 - 1)
    sc_word key = 0;
    for (int w = wave; w < W; w += SC_WAVES) {
        sc_word mm = sc_uniform(row[w]);
        while (mm) {
            const int j = w * 64 + (__ffsll((long long)mm) - 1);
            mm &= mm - 1;
            const sc_word *__restrict__ rj = a.bits + (size_t)j * W;
            int c = 0;
            for (int k = lane; k < W; k += 64) c += __popcll(row[k] & rj[k]);
            c = sc_wave_sum(c);
            const sc_word nk = ((sc_word)(unsigned)c << 32) | (sc_word)(0xFFFFFFFFu - (unsigned)j);
            const int at = __popcll(__ballot(key > nk));           // the keys are distinct and sorted: a prefix of the lanes
            const sc_word up = __shfl_up(key, 1, 64);
            if (lane == at) key = nk; else if (lane > at) key = up;
        }
    }
    keys[wave][lane] = key;
    __syncthreads();
    if (wave != 0) return;                 // no barrier below
    for (int v = 1; v < SC_WAVES; v++)
        for (int l = 0; l < 64; l++) {
            const sc_word nk = sc_uniform(keys[v][l]);
            if (nk == 0) break;
            const int at = __popcll(__ballot(key > nk));
            const sc_word up = __shfl_up(key, 1, 64);
            if (lane == at) key = nk; else if (lane > at) key = up;
        }
    // K1: m, then the first k1 keys
    const int n1 = min(a.k1, (int)__popcll(__ballot(key != 0))), nK1 = 1 + n1;
    const sc_word prev = __shfl_up(key, 1, 64);
    const int idx = lane == 0 ? m : (lane < nK1 ? (int)(0xFFFFFFFFu - (unsigned)prev) : -1);
    if (a.k1_rows) a.k1_rows[(size_t)s * 64 + lane] = idx;
    sc_word mask = 0;                      // bit b: member b of K1 is compatible with member `lane`
    for (int b = 0; b < nK1; b++) {
        const int jb = __shfl(idx, b, 64);
        if (lane < nK1) mask |= ((a.bits[(size_t)idx * W + (jb >> 6)] >> (jb & 63)) & 1ull) << b;
    }
    const sc_word mask_m = __shfl(mask, 0, 64);
    const bool member = lane >= 1 && lane < nK1;
    const int L = member ? (((mask_m >> lane) & 1ull) ? (int)__popcll(mask_m & mask) : 0) : -1;
    int rank = 0, maxL = 0;
    for (int b = 1; b < nK1; b++) {
        const int Lb = __shfl(L, b, 64);
        if (Lb > L || (Lb == L && b < lane)) rank++;
        maxL = max(maxL, Lb);
    }
    const bool chosen = member && rank < a.k2 && 2 * L >= maxL;      // L is non-increasing in rank: the chosen are ranks 0 .. count - 1
    const int nK2 = 1 + (int)__popcll(__ballot(chosen));
    int mine = lane == 0 ? m : -1;         // K2 in order: m, then the chosen by rank
    for (int b = 1; b < nK1; b++) {
        const int rb = __shfl(rank, b, 64), ib = __shfl(idx, b, 64), cb = __shfl(chosen ? 1 : 0, b, 64);
        if (cb && rb == lane - 1) mine = ib;
    }
    if (a.k2_rows) a.k2_rows[(size_t)s * 64 + lane] = lane < nK2 ? mine : -1;
    const float4 sp = a.ps[mine >= 0 ? mine : m], tp = a.pt[mine >= 0 ? mine : m];
    double U[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool ok = nK2 >= 3;
    if (ok) {                              // every lane sums the same moments in K2 order, about the seed's own two points
        const double os[3] = {(double)__shfl(sp.x, 0, 64), (double)__shfl(sp.y, 0, 64), (double)__shfl(sp.z, 0, 64)};
        const double o[3] = {(double)__shfl(tp.x, 0, 64), (double)__shfl(tp.y, 0, 64), (double)__shfl(tp.z, 0, 64)};
        double M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = 0.0;
        for (int p = 0; p < nK2; p++) {
            const double u[3] = {(double)__shfl(sp.x, p, 64) - os[0], (double)__shfl(sp.y, p, 64) - os[1], (double)__shfl(sp.z, p, 64) - os[2]};
            const double v[3] = {(double)__shfl(tp.x, p, 64) - o[0], (double)__shfl(tp.y, p, 64) - o[1], (double)__shfl(tp.z, p, 64) - o[2]};
#pragma unroll
            for (int d = 0; d < 3; d++) {
                M[d] += u[d]; M[3 + d] += v[d];
#pragma unroll
                for (int e = 0; e < 3; e++) M[6 + 3 * d + e] += v[d] * u[e];
            }
            M[15] += u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
        }
        icp_umeyama(M, (double)nK2, o, false, U, os);
#pragma unroll
        for (int k = 0; k < 12; k++) if (!isfinite(U[k])) ok = false;
    }
    if (lane == 0) {
        a.valid[s] = ok ? 1 : 0;
#pragma unroll
        for (int k = 0; k < 12; k++) a.T[(size_t)s * 12 + k] = ok ? U[k] : 0.0;
    }
}

struct ScPolicy {                  // no sequential loop here: the host picks the best seed from one read-back.  UNROLL 2: what the compiler chose unasked
    typedef float4 Row;
    static constexpr int DIM = 12, ROWD = 6, TILE = SC_TILE, SPLIT_ROWS = SC_SPLIT_ROWS, MAX_SPLITS = SC_MAX_SPLITS, UNROLL = 2, SUM_UNROLL = 1;
    static constexpr bool LISTED = false, STOPS = false;
    __host__ __device__ static constexpr int stride(int S) { return S; }
    __device__ static inline double residual(const double *T, const double *p) { return sc_d2(T, p[0], p[1], p[2], p[3], p[4], p[5]); }
};

// refinement pass under the pose T12: inlier flags, and per workgroup (count, err2, the 16 moments of the inlier rows about o = (target, source) origin)
__global__ void __launch_bounds__(SC_BS) k_sc_eval(const float4 *__restrict__ ps, const float4 *__restrict__ pt, int N, const double *__restrict__ T12, double d2max,
                                                   const double *__restrict__ o6, uint8_t *__restrict__ flags, double *__restrict__ partials) {
    __shared__ double red[SC_WAVES][SC_NV];
    const int i = blockIdx.x * SC_BS + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double v[SC_NV];
#pragma unroll
    for (int k = 0; k < SC_NV; k++) v[k] = 0.0;
    if (i < N) {
        double Tm[12];
#pragma unroll
        for (int k = 0; k < 12; k++) Tm[k] = T12[k];
        const float4 s = ps[i], t = pt[i];
        const double d2 = sc_d2(Tm, s.x, s.y, s.z, t.x, t.y, t.z);
        const bool in = d2 < d2max;
        flags[i] = in ? 1 : 0;
        if (in) {
            const double ux = (double)s.x - o6[3], uy = (double)s.y - o6[4], uz = (double)s.z - o6[5];
            const double vx = (double)t.x - o6[0], vy = (double)t.y - o6[1], vz = (double)t.z - o6[2];
            v[0] = 1.0; v[1] = d2;
            v[2] = ux; v[3] = uy; v[4] = uz; v[5] = vx; v[6] = vy; v[7] = vz;
            v[8] = vx * ux; v[9] = vx * uy; v[10] = vx * uz; v[11] = vy * ux; v[12] = vy * uy; v[13] = vy * uz; v[14] = vz * ux; v[15] = vz * uy; v[16] = vz * uz;
            v[17] = ux * ux + uy * uy + uz * uz;
        }
    }
#pragma unroll
    for (int k = 0; k < SC_NV; k++) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < SC_NV; k++) red[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < SC_NV) {
        double s = red[0][threadIdx.x];
        for (int w = 1; w < SC_WAVES; w++) s += red[w][threadIdx.x];
        partials[(size_t)blockIdx.x * SC_NV + threadIdx.x] = s;
    }
}
// out: [0] count, [1] err2 of the pose evaluated, [2..13] the fit over its inlier rows, [14] 1 when that fit exists and is finite
__global__ void k_sc_refit(const double *__restrict__ partials, int nb, const double *__restrict__ o6, double *__restrict__ out) {
    double S[SC_NV];
    for (int k = 0; k < SC_NV; k++) S[k] = 0.0;
    for (int b = 0; b < nb; b++)
        for (int k = 0; k < SC_NV; k++) S[k] += partials[(size_t)b * SC_NV + k];
    double U[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    bool ok = S[0] >= 1.0;
    if (ok) {
        const double o[3] = {o6[0], o6[1], o6[2]}, os[3] = {o6[3], o6[4], o6[5]};
        icp_umeyama(S + 2, S[0], o, false, U, os);
        for (int k = 0; k < 12; k++) if (!isfinite(U[k])) ok = false;
    }
    out[0] = S[0]; out[1] = S[1];
    for (int k = 0; k < 12; k++) out[2 + k] = U[k];
    out[14] = ok ? 1.0 : 0.0;
}
__global__ void __launch_bounds__(SC_BS) k_sc_dump(const int *__restrict__ seeds, const double *__restrict__ T, int S, int32_t *__restrict__ seed_rows, double *__restrict__ T_out) {
    const int s = blockIdx.x * SC_BS + threadIdx.x;
    if (s >= S) return;
    seed_rows[s] = seeds[s];
    for (int k = 0; k < 12; k++) T_out[(size_t)s * 16 + k] = T[(size_t)s * 12 + k];
    T_out[(size_t)s * 16 + 12] = 0; T_out[(size_t)s * 16 + 13] = 0; T_out[(size_t)s * 16 + 14] = 0; T_out[(size_t)s * 16 + 15] = 1;
}

// ------------------------------------------------------------------------------------------------------------------ host
struct ScRun {
    int N = 0, W = 0, S = 0;             // rows, words per row, seeds
    float4 *ps = nullptr, *pt = nullptr; sc_word *bits = nullptr; int32_t *deg = nullptr; long long *score = nullptr;
    int *seeds = nullptr; int32_t *k1_rows = nullptr, *k2_rows = nullptr; double *T = nullptr; uint8_t *valid = nullptr; int32_t *cnt = nullptr; double *err2 = nullptr;
};
static inline int sc_grid(int64_t n) { return (int)((n + SC_BS - 1) / SC_BS); }
static int64_t sc_seed_cap(const pcr_sc2_option *o, int64_t N) {
    int64_t by_ratio = (int64_t)(o->seed_ratio * (double)N);
    if (by_ratio < 1) by_ratio = 1;
    return std::min<int64_t>(by_ratio, o->max_seeds);
}
static size_t sc_scratch_bytes(int64_t N, int64_t S, bool own_bits) {
    const size_t W = (size_t)(N + 63) / 64;
    return (own_bits ? (size_t)N * W * 8 : 0) + (size_t)N * (32 + 4 + 8 + 16 + 8 + 16 + 1 + 4 + 1 + 4) + pcr_sort_temp_bytes((size_t)N) +
           (size_t)S * (4 + 512 + 96 + 1 + 4 + 8 + (size_t)SC_MAX_SPLITS * 12) + (size_t)(N / SC_BS + 1) * SC_NV * 8 + (2u << 20);
}

static int sc_check_list(pcr_context *ctx, const float *src_xyz, int64_t n_src, const float *tgt_xyz, int64_t n_tgt, const int32_t *corres, int64_t N, double tau) {
    if (n_src < 0 || n_tgt < 0 || N < 0) { ctx->err = "negative count"; return PCR_EINVAL; }
    if (!(tau > 0.0) || !std::isfinite(tau)) { ctx->err = "spatial compatibility: inlier_threshold must be positive and finite"; return PCR_EINVAL; }
    if (N > SC_MAX_N) {
        ctx->err = "spatial compatibility: " + std::to_string((long long)N) + " correspondences, the limit is 65536 (the bit matrix would exceed 512 MB): "
                   "use the mutual filter of correspondences_from_features or a keypoint subset";
        return PCR_EINVAL;
    }
    if (n_src > 0x7fffffff / 8 || n_tgt > 0x7fffffff / 8) { ctx->err = "cloud too large"; return PCR_EINVAL; }
    if ((n_src > 0 && !src_xyz) || (n_tgt > 0 && !tgt_xyz)) { ctx->err = "missing cloud"; return PCR_EINVAL; }
    if (N > 0 && (!corres || n_src == 0 || n_tgt == 0)) { ctx->err = "correspondences without a list or without points"; return PCR_EINVAL; }
    return PCR_OK;
}
static int sc_check_option(pcr_context *ctx, const pcr_sc2_option *o) {
    if (!o) { ctx->err = "missing pcr_sc2_option"; return PCR_EINVAL; }
    if (!(o->inlier_threshold > 0.0) || !std::isfinite(o->inlier_threshold)) { ctx->err = "sc2: inlier_threshold must be positive and finite"; return PCR_EINVAL; }
    if (!(o->nms_radius >= 0.0)) { ctx->err = "sc2: nms_radius must be >= 0"; return PCR_EINVAL; }
    if (o->k1 < 2 || o->k1 > 63) { ctx->err = "sc2: k1 must be in 2..63 (K1 fits one wavefront)"; return PCR_EINVAL; }
    if (o->k2 < 1 || o->k2 > o->k1) { ctx->err = "sc2: k2 must be in 1..k1"; return PCR_EINVAL; }
    if (!(o->seed_ratio > 0.0 && o->seed_ratio <= 1.0)) { ctx->err = "sc2: seed_ratio must be in (0, 1]"; return PCR_EINVAL; }
    if (o->max_seeds < 1 || o->max_seeds > 65536) { ctx->err = "sc2: max_seeds must be in 1..65536"; return PCR_EINVAL; }
    if (o->refine_iterations < 0) { ctx->err = "sc2: refine_iterations must be >= 0"; return PCR_EINVAL; }
    return PCR_OK;
}

// the list checked, gathered, and its compatibility graph: bits (the caller's array, or scratch), deg and score (likewise; null + !need: not computed)
static int sc_graph(pcr_context *ctx, ScRun &R, const float *src_xyz, int64_t n_src, const float *tgt_xyz, int64_t n_tgt, const int32_t *corres, int64_t N, double tau,
                    sc_word *bits_out, int32_t *deg_out, long long *score_out, bool need_scores) {
    PCR_TRY(pcr_corres_check(ctx, corres, N, n_src, n_tgt));
    R.N = (int)N; R.W = (int)((N + 63) / 64);
    R.ps = arena<float4>(ctx, N); R.pt = arena<float4>(ctx, N);
    R.bits = bits_out ? bits_out : arena<sc_word>(ctx, (size_t)N * R.W);
    R.deg = deg_out; R.score = score_out ? score_out : (need_scores ? arena<long long>(ctx, N) : nullptr);
    if (!R.ps || !R.pt || !R.bits || (need_scores && !R.score)) return PCR_ENOMEM;
    PCR_LAUNCH(ctx, k_sc_gather, dim3(sc_grid(N)), dim3(SC_BS), 0, ctx->stream, src_xyz, tgt_xyz, corres, R.N, R.ps, R.pt);
    PCR_LAUNCH(ctx, k_sc_bits, dim3(R.W, sc_grid(N)), dim3(SC_BS), 0, ctx->stream, R.ps, R.pt, R.N, R.W, tau, R.bits);
    if (R.deg || R.score) PCR_LAUNCH(ctx, k_sc_scores, dim3(R.N), dim3(SC_BS), 0, ctx->stream, R.bits, R.N, R.W, R.deg, R.score);
    return PCR_OK;
}

// order, suppression, seeds, their hypotheses and scores; R.S is on the host when it returns
static int sc_seeds(pcr_context *ctx, ScRun &R, const pcr_sc2_option *o) {
    const int N = R.N;
    const size_t tb = pcr_sort_temp_bytes((size_t)N);
    uint64_t *keys = arena<uint64_t>(ctx, N), *keys2 = arena<uint64_t>(ctx, N);
    uint32_t *vals = arena<uint32_t>(ctx, N), *order = arena<uint32_t>(ctx, N);
    void *temp = pcr_arena_alloc(ctx, tb);
    float4 *psort = arena<float4>(ctx, N);
    uint8_t *flag = arena<uint8_t>(ctx, N); int *pos = arena<int>(ctx, N), *total = arena<int>(ctx, 1);
    const int cap = (int)sc_seed_cap(o, N);
    R.seeds = arena<int>(ctx, cap);
    if (!keys || !keys2 || !vals || !order || !temp || !psort || !flag || !pos || !total || !R.seeds) return PCR_ENOMEM;
    PCR_LAUNCH(ctx, k_sc_keys, dim3(sc_grid(N)), dim3(SC_BS), 0, ctx->stream, R.score, N, keys, vals);
    PCR_TRY(pcr_sort_pairs(ctx, temp, tb, keys, keys2, vals, order, (size_t)N, 33));
    PCR_LAUNCH(ctx, k_sc_sorted, dim3(sc_grid(N)), dim3(SC_BS), 0, ctx->stream, R.ps, order, N, psort);
    PCR_LAUNCH(ctx, k_sc_nms, dim3((N + SC_WAVES - 1) / SC_WAVES), dim3(SC_BS), 0, ctx->stream, psort, order, R.score, N, o->nms_radius, flag);
    PCR_TRY(pcr_dev_flag_scan(ctx, flag, nullptr, N, pos, total));
    PCR_LAUNCH(ctx, k_sc_pick, dim3(sc_grid(N)), dim3(SC_BS), 0, ctx->stream, order, flag, pos, N, cap, R.seeds);
    int64_t n_cand = 0;
    PCR_TRY(pcr_read_count(ctx, total, &n_cand));
    const int S = R.S = (int)std::min<int64_t>(n_cand, cap);
    if (S == 0) return PCR_OK;
    R.k1_rows = arena<int32_t>(ctx, (size_t)S * 64); R.k2_rows = arena<int32_t>(ctx, (size_t)S * 64);
    R.T = arena<double>(ctx, (size_t)S * 12); R.valid = arena<uint8_t>(ctx, S); R.cnt = arena<int32_t>(ctx, S); R.err2 = arena<double>(ctx, S);
    HypoScore<ScPolicy> sc = {};
    PCR_TRY(hypo_score_alloc(ctx, sc, N, S));
    if (!R.k1_rows || !R.k2_rows || !R.T || !R.valid || !R.cnt || !R.err2) return PCR_ENOMEM;
    ScSeedArgs a;
    a.bits = R.bits; a.ps = R.ps; a.pt = R.pt; a.N = N; a.W = R.W; a.k1 = o->k1; a.k2 = o->k2; a.seeds = R.seeds; a.k1_rows = R.k1_rows; a.k2_rows = R.k2_rows; a.T = R.T; a.valid = R.valid;
    PCR_LAUNCH(ctx, k_sc_seed, dim3(S), dim3(SC_BS), 0, ctx->stream, a);
    sc.ra = R.ps; sc.rb = R.pt; sc.rows = N; sc.thr = o->inlier_threshold * o->inlier_threshold; sc.model = R.T; sc.valid = R.valid; sc.cnt = R.cnt; sc.err = R.err2;
    hypo_score(ctx, sc, S, nullptr);
    return PCR_OK;
}

static void sc_empty_result(pcr_result *result, pcr_sc2_info *info, int64_t N) {
    memset(result, 0, sizeof *result);
    for (int k = 0; k < 4; k++) result->transformation[5 * k] = 1.0;
    if (info) { info->n_corres = N; info->n_seeds = 0; info->n_valid = 0; info->best_seed = -1; info->best_seed_count = 0; info->refine_iterations_run = 0; }
}

extern "C" int pcr_spatial_compatibility(pcr_context *ctx, const float *src_xyz, int64_t n_src, const float *tgt_xyz, int64_t n_tgt, const int32_t *corres, int64_t n_corres,
                                         double inlier_threshold, int64_t *bits, int32_t *degrees, int64_t *scores) {
    return pcr_api_call(ctx, [&]() -> int {
        PCR_TRY(sc_check_list(ctx, src_xyz, n_src, tgt_xyz, n_tgt, corres, n_corres, inlier_threshold));
        if (n_corres == 0) return PCR_OK;
        PCR_TRY(pcr_arena_reserve(ctx, sc_scratch_bytes(n_corres, 0, !bits)));
        ScRun R;
        return sc_graph(ctx, R, src_xyz, n_src, tgt_xyz, n_tgt, corres, n_corres, inlier_threshold, (sc_word *)bits, degrees, (long long *)scores, false);
    });
}

extern "C" int pcr_registration_sc2_correspondence(pcr_context *ctx, const float *src_xyz, int64_t n_src, const float *tgt_xyz, int64_t n_tgt, const int32_t *corres,
                                                   int64_t n_corres, const pcr_sc2_option *option, pcr_result *result, int32_t *correspondences, pcr_sc2_info *info) {
    return pcr_api_call(ctx, [&]() -> int {
        if (!result) return PCR_EINVAL;
        PCR_TRY(sc_check_option(ctx, option));
        PCR_TRY(sc_check_list(ctx, src_xyz, n_src, tgt_xyz, n_tgt, corres, n_corres, option->inlier_threshold));
        const int64_t N = n_corres;
        sc_empty_result(result, info, N);
        if (N == 0) return PCR_OK;
        PCR_TRY(pcr_arena_reserve(ctx, sc_scratch_bytes(N, sc_seed_cap(option, N), true)));
        if (N < 3) return pcr_corres_check(ctx, corres, N, n_src, n_tgt);       // the list is still checked
        ScRun R;
        PCR_TRY(sc_graph(ctx, R, src_xyz, n_src, tgt_xyz, n_tgt, corres, N, option->inlier_threshold, nullptr, nullptr, nullptr, true));
        PCR_TRY(sc_seeds(ctx, R, option));
        const int S = R.S;
        if (info) info->n_seeds = S;
        if (S == 0) return PCR_OK;
        std::vector<int32_t> cnt(S); std::vector<double> err2(S), T((size_t)S * 12); std::vector<int> seeds(S);
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(cnt.data(), R.cnt, sizeof(int32_t) * S, hipMemcpyDeviceToHost, ctx->stream));
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(err2.data(), R.err2, sizeof(double) * S, hipMemcpyDeviceToHost, ctx->stream));
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(T.data(), R.T, sizeof(double) * 12 * S, hipMemcpyDeviceToHost, ctx->stream));
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(seeds.data(), R.seeds, sizeof(int) * S, hipMemcpyDeviceToHost, ctx->stream));
        PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        int best = -1; int64_t n_valid = 0;
        for (int s = 0; s < S; s++) {
            if (cnt[s] >= 0) n_valid++;
            if (cnt[s] <= 0) continue;
            if (best < 0 || cnt[s] > cnt[best] || (cnt[s] == cnt[best] && err2[s] < err2[best])) best = s;
        }
        if (info) { info->n_valid = n_valid; info->best_seed = best; info->best_seed_count = best >= 0 ? cnt[best] : 0; }
        if (best < 0) return PCR_OK;
        // refinement: every pass evaluates a pose (flags, count, err2) and fits the next candidate over its inlier rows
        const int nb = sc_grid(N);
        double *Tdev = arena<double>(ctx, 12), *o6 = arena<double>(ctx, 6), *partials = arena<double>(ctx, (size_t)nb * SC_NV), *out = arena<double>(ctx, 16);
        uint8_t *flags = arena<uint8_t>(ctx, N); int *pos = arena<int>(ctx, N), *total = arena<int>(ctx, 1);
        if (!Tdev || !o6 || !partials || !out || !flags || !pos || !total) return PCR_ENOMEM;
        const double d2max = option->inlier_threshold * option->inlier_threshold;
        double h[16];
        {                                   // the moments' origins: the two points of the best seed's row
            float4 hp[2];
            PCR_HIP_CHECK(ctx, hipMemcpyAsync(&hp[0], R.pt + seeds[best], sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
            PCR_HIP_CHECK(ctx, hipMemcpyAsync(&hp[1], R.ps + seeds[best], sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
            PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            const double o[6] = {hp[0].x, hp[0].y, hp[0].z, hp[1].x, hp[1].y, hp[1].z};
            PCR_HIP_CHECK(ctx, hipMemcpyAsync(o6, o, sizeof o, hipMemcpyHostToDevice, ctx->stream));
            PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        }
        auto eval = [&](const double *T12) -> int {
            PCR_HIP_CHECK(ctx, hipMemcpyAsync(Tdev, T12, sizeof(double) * 12, hipMemcpyHostToDevice, ctx->stream));
            PCR_LAUNCH(ctx, k_sc_eval, dim3(nb), dim3(SC_BS), 0, ctx->stream, R.ps, R.pt, (int)N, Tdev, d2max, o6, flags, partials);
            PCR_LAUNCH(ctx, k_sc_refit, dim3(1), dim3(1), 0, ctx->stream, partials, nb, o6, out);
            PCR_HIP_CHECK(ctx, hipMemcpyAsync(h, out, sizeof(double) * 16, hipMemcpyDeviceToHost, ctx->stream));
            PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            return PCR_OK;
        };
        double cur[12], cand[12];
        memcpy(cur, &T[(size_t)best * 12], sizeof cur);
        PCR_TRY(eval(cur));
        double c0 = h[0], e0 = h[1]; bool have = h[14] != 0.0; bool flags_are_cur = true;
        memcpy(cand, h + 2, sizeof cand);
        int it = 0;
        while (it < option->refine_iterations && have) {
            PCR_TRY(eval(cand));
            it++; flags_are_cur = false;
            if (!(h[0] > c0 || (h[0] == c0 && h[1] < e0))) break;
            memcpy(cur, cand, sizeof cur); c0 = h[0]; e0 = h[1]; have = h[14] != 0.0; flags_are_cur = true;
            memcpy(cand, h + 2, sizeof cand);
        }
        if (!flags_are_cur) PCR_TRY(eval(cur));
        if (info) info->refine_iterations_run = it;
        const int64_t count = (int64_t)c0;
        if (count <= 0) { ctx->err = "sc2: the best seed lost its inliers"; return PCR_ENUMERIC; }
        for (int k = 0; k < 12; k++) result->transformation[k] = cur[k];
        result->fitness = (double)count / (double)N;
        result->inlier_rmse = sqrt(e0 / (double)count);
        result->n_correspondences = count;
        result->iterations = it;
        result->converged = 1;
        if (correspondences) {
            PCR_TRY(pcr_dev_flag_scan(ctx, flags, nullptr, (int)N, pos, total));
            PCR_LAUNCH(ctx, k_hypo_emit<>, dim3(hypo_blocks(N)), dim3(HYPO_BS), 0, ctx->stream, corres, flags, pos, (int)N, correspondences);
            int64_t n_in = 0;
            PCR_TRY(pcr_read_count(ctx, total, &n_in));
            if (n_in != count) { ctx->err = "sc2: the inlier pass disagrees with the count of the pose"; return PCR_ENUMERIC; }
        }
        return PCR_OK;
    });
}

extern "C" int pcr_debug_sc2_seeds(pcr_context *ctx, const float *src_xyz, int64_t n_src, const float *tgt_xyz, int64_t n_tgt, const int32_t *corres, int64_t n_corres,
                                   const pcr_sc2_option *option, int64_t *n_seeds, int32_t *seed_rows, int32_t *k1_rows, int32_t *k2_rows, double *T_out, uint8_t *valid_out,
                                   int32_t *inliers_out, double *err2_out) {
    return pcr_api_call(ctx, [&]() -> int {
        if (!n_seeds || !seed_rows || !k1_rows || !k2_rows || !T_out || !valid_out || !inliers_out || !err2_out) return PCR_EINVAL;
        *n_seeds = 0;
        PCR_TRY(sc_check_option(ctx, option));
        PCR_TRY(sc_check_list(ctx, src_xyz, n_src, tgt_xyz, n_tgt, corres, n_corres, option->inlier_threshold));
        const int64_t N = n_corres;
        if (N < 3) { ctx->err = "fewer than 3 correspondences"; return PCR_EINVAL; }
        PCR_TRY(pcr_arena_reserve(ctx, sc_scratch_bytes(N, sc_seed_cap(option, N), true)));
        ScRun R;
        PCR_TRY(sc_graph(ctx, R, src_xyz, n_src, tgt_xyz, n_tgt, corres, N, option->inlier_threshold, nullptr, nullptr, nullptr, true));
        PCR_TRY(sc_seeds(ctx, R, option));
        const int S = R.S;
        *n_seeds = S;
        if (S == 0) return PCR_OK;
        PCR_LAUNCH(ctx, k_sc_dump, dim3(sc_grid(S)), dim3(SC_BS), 0, ctx->stream, R.seeds, R.T, S, seed_rows, T_out);
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(k1_rows, R.k1_rows, sizeof(int32_t) * 64 * S, hipMemcpyDeviceToDevice, ctx->stream));
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(k2_rows, R.k2_rows, sizeof(int32_t) * 64 * S, hipMemcpyDeviceToDevice, ctx->stream));
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(valid_out, R.valid, S, hipMemcpyDeviceToDevice, ctx->stream));
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(inliers_out, R.cnt, sizeof(int32_t) * S, hipMemcpyDeviceToDevice, ctx->stream));
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(err2_out, R.err2, sizeof(double) * S, hipMemcpyDeviceToDevice, ctx->stream));
        PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        return PCR_OK;
    });
}
