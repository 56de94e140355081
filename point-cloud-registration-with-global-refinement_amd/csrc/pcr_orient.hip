// pcr_orient.hip -- normal orientation on gfx950: PointCloud.orient_normals_consistent_tangent_plane of Open3D (Hoppe et al. 1992) and its
// element-wise relatives, plus the Euclidean minimum spanning tree the propagation is built on.  include/pcr_hip.h states the rules (DIST, DOT,
// ORDER, EMST, KNN, GRAPH, TREE, ROOT, PROPAGATE, RESULT); under ORDER both spanning trees are unique, so the rows below are those of a Prim or
// Kruskal run on the host, whatever the schedule.
//
// Both trees come out of BORUVKA ROUNDS.  Component labels, candidates and edges live in the CALLER's row numbers; only the octree walk goes
// through the Morton-sorted copy of the cloud, whose points carry their caller row in w.  A round of the EMST:
//   k_ori_leaf_labels  per leaf of the octree the component all its rows belong to, or -1
//   k_emst_list        per row the first entry of its k-NN list in another component: exact, because for a fixed row the order (d^2, j) of the
//                      list and the order (d^2, lo, hi) of the edges agree; an atomic minimum of the d^2 bits per component
//   k_emst_walk        rows without such an entry walk the octree (oct_search) under the component's best d^2 so far, ties included, skipping
//                      leaves that lie in their own component; a row whose last list distance exceeds that bound strictly does not walk
//   k_emst_pick        among the rows that hold the component's d^2, an atomic minimum of (lo << 32 | hi)
//   k_emst_hook        every component hooks along its edge; the only cycles under a strict order are mutual picks of ONE edge, broken by
//                      hooking the larger root under the smaller; each edge is emitted once
//   k_ori_compress     every row follows the hooks to its new root (a second label array: nothing is read and written in one launch)
// The TREE rounds are the same over the explicit edge list (EMST edges + list entries) with weight 1 - |c|, and the labels carry a parity bit:
// hooking root A under root B along {a, b} stores par(a) ^ par(b) ^ s(a, b), so that after the last round flip_v = par(v) ^ par(r) ^ flip_r
// without a walk over a tree of unknown depth.
//
// TERMINATION.  Every kernel is an ordinary bounded launch: no lane waits for another lane, wavefront or workgroup; there is no lock, no
// barrier across workgroups and no spin on a value somebody else has to write.  The atomics are minima and counters whose result nobody
// waits for.  k_ori_compress follows hook[], which no launch writes while it is read, for at most n steps (the hooks of a round form a
// forest: a cycle would need two components that pick different edges towards each other, which a strict order excludes, and the mutual
// pick of one edge is broken by the root numbers); the host loop stops after ceil(log2 n) rounds, or when a round joined nothing, with an
// error.  Loads of values that other compute units change within a launch (the component minima) are relaxed agent-scope atomics, as in
// pcr_cluster.hip; whatever a lane reads there is a valid upper bound of its component's minimum.
// Contraction is off: d^2 and the dot products have the bits of a host recomputation.
#pragma clang fp contract(off)
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include "pcr_octree.h"

#define ORI_BS 256
#define ORI_MAX_POINTS 0x7fffffffLL            // the clouds of this library are counted in int
#define ORI_MAX_K 200                          // the search index's limit
#define ORI_LIST_MIN 8                         // entries of the lists the EMST rounds read
#define ORI_NONE 0xffffffffffffffffull
#define ORI_FAR 3.4e38f

struct OriState {                              // zeroed before a run; the host reads it after every round
    int n_edges;                               // edges emitted so far by the rounds of the current tree
    int bad;                                   // a non-finite coordinate or normal component
    int n_flipped;
    int root;
    unsigned int zmax;                         // ROOT: the largest z as an ordered key
    int flip_root;                             // ROOT: nz_r < 0, taken before any row is negated
    unsigned long long walked;                 // rows that walked the octree, over all rounds
};
static_assert(sizeof(OriState) == 32, "one small record");

__device__ static inline unsigned long long ori_load64(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the entry only decreases, so a value read earlier is an upper bound: a key that is not below it cannot be the minimum (pcr_cluster.hip)
__device__ static inline void ori_min64(unsigned long long *p, unsigned long long v) { if (ori_load64(p) > v) atomicMin(p, v); }
__device__ static inline bool ori_lt(unsigned long long ak, int ai, unsigned long long bk, int bi) { return ak < bk || (ak == bk && ai < bi); }
__device__ static inline unsigned long long ori_pack(int a, int b) {
    const unsigned lo = (unsigned)min(a, b), hi = (unsigned)max(a, b);
    return ((unsigned long long)lo << 32) | hi;
}
// a float64 as an unsigned key with the same order (weights 1 - |c| are negative when the normals are longer than 1)
__device__ static inline unsigned long long ori_key_f64(double w) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(w);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ static inline unsigned int ori_key_f32(float z) {          // -0 and +0 compare equal: one key for both
    const unsigned int b = __float_as_uint(z == 0.0f ? 0.0f : z);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
// DOT: c(i, j) = (nx_i nx_j + ny_i ny_j) + nz_i nz_j in float64 on the float32 normals, each operation rounded once
__device__ static inline double ori_dot(const float *__restrict__ nrm, int a, int b) {
#pragma clang fp contract(off)
    const double ax = (double)nrm[(size_t)a * 3], ay = (double)nrm[(size_t)a * 3 + 1], az = (double)nrm[(size_t)a * 3 + 2];
    const double bx = (double)nrm[(size_t)b * 3], by = (double)nrm[(size_t)b * 3 + 1], bz = (double)nrm[(size_t)b * 3 + 2];
    double c = ax * bx;
    c += ay * by;
    c += az * bz;
    return c;
}
template <int CTRL> __device__ static inline unsigned long long ori_dpp_u64(unsigned long long v) {
    const unsigned lo = (unsigned)pcr_dpp_i<CTRL>((int)(unsigned)v), hi = (unsigned)pcr_dpp_i<CTRL>((int)(unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
// smallest (key, caller row) of the octet, in all 8 lanes
__device__ static inline void ori_octet_min(unsigned long long &k, int &i) {
    { const unsigned long long o = ori_dpp_u64<PCR_DPP_XOR1>(k); const int oi = pcr_dpp_i<PCR_DPP_XOR1>(i); if (ori_lt(o, oi, k, i)) { k = o; i = oi; } }
    { const unsigned long long o = ori_dpp_u64<PCR_DPP_XOR2>(k); const int oi = pcr_dpp_i<PCR_DPP_XOR2>(i); if (ori_lt(o, oi, k, i)) { k = o; i = oi; } }
    { const unsigned long long o = ori_dpp_u64<PCR_DPP_HMIRROR>(k); const int oi = pcr_dpp_i<PCR_DPP_HMIRROR>(i); if (ori_lt(o, oi, k, i)) { k = o; i = oi; } }
}
// float32 bound of a walk under the float64 key bits bk (d^2 >= 0): slightly wide, never below the smallest normal float (a bound of 0 --
// duplicated points -- must still let the strict box and screen tests pass the copies)
__device__ static inline float ori_bound(unsigned long long bk) {
    if (bk == ORI_NONE) return ORI_FAR;
    return fminf(fmaxf((float)(__longlong_as_double((long long)bk) * (1.0 + 1e-6)), 1.17549435e-38f), ORI_FAR);
}

// ============================================================================================================ set-up
__global__ void __launch_bounds__(ORI_BS) k_ori_check(const float *__restrict__ xyz, const float *__restrict__ nrm, size_t count, OriState *st) {
    const size_t i = (size_t)blockIdx.x * ORI_BS + threadIdx.x;
    bool bad = false;
    if (i < count) bad = !isfinite(xyz[i]) || (nrm && !isfinite(nrm[i]));
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(&st->bad, 1);
}
__global__ void __launch_bounds__(ORI_BS) k_ori_tag(float4 *pts, const uint32_t *__restrict__ perm, int n) {
    const int i = blockIdx.x * ORI_BS + threadIdx.x;
    if (i < n) pts[i].w = __int_as_float((int)perm[i]);
}
__global__ void __launch_bounds__(ORI_BS) k_ori_init(int n, int *__restrict__ comp, int *__restrict__ hook, uint8_t *__restrict__ par) {
    const int i = blockIdx.x * ORI_BS + threadIdx.x;
    if (i >= n) return;
    comp[i] = i; hook[i] = i;
    if (par) par[i] = 0;
}
// the component every row of a leaf belongs to, or -1
__global__ void __launch_bounds__(ORI_BS) k_ori_leaf_labels(OctView t, int n, const int *__restrict__ comp, int *__restrict__ leaf_lab) {
    const int l = blockIdx.x * ORI_BS + threadIdx.x;
    const OctMeta *m = t.meta;
    if (l >= n || m->nl < 1 || l >= m->cnt[0]) return;
    const size_t j = (size_t)(m->off[0] + l);
    const int first = __float_as_int(t.nodes[2 * j].w), count = __float_as_int(t.nodes[2 * j + 1].w);
    int lab = -1;
    if (count > 0 && first >= 0 && first + count <= n) {
        lab = comp[__float_as_int(t.pts[first].w)];
        for (int p = first + 1; p < first + count; p++)
            if (comp[__float_as_int(t.pts[p].w)] != lab) { lab = -1; break; }
    }
    leaf_lab[l] = lab;
}

// ============================================================================================================ EMST rounds
struct EmstArgs {
    OctView t; int n, K;
    const int32_t *lidx; const double *ld2;      // n x K lists in caller rows, ordered by (d^2, caller row); -1 / +inf beyond the cloud's size
    const int *comp; const int *leaf_lab;
    unsigned long long *best_w, *best_e;         // per component (indexed by its root row): bits of the smallest d^2, then the smallest (lo, hi) at it
    unsigned long long *cand_k; int *cand_j;     // per row: its nearest row of another component, as far as the round needs it
    OriState *st;
};
__global__ void __launch_bounds__(ORI_BS) k_emst_list(EmstArgs a) {
    const int i = blockIdx.x * ORI_BS + threadIdx.x;
    if (i >= a.n) return;
    const int ci = a.comp[i];
    unsigned long long ck = ORI_NONE; int cj = -1;
    for (int s = 0; s < a.K; s++) {
        const int j = a.lidx[(size_t)i * a.K + s];
        if (j < 0) break;
        if (a.comp[j] != ci) { cj = j; ck = (unsigned long long)__double_as_longlong(a.ld2[(size_t)i * a.K + s]); break; }
    }
    a.cand_k[i] = ck; a.cand_j[i] = cj;
    if (cj >= 0) ori_min64(a.best_w + ci, ck);
}

// one sorted row per octet; only the rows k_emst_list left without a candidate walk
__global__ void __launch_bounds__(ORI_BS) k_emst_walk(EmstArgs a) {
    constexpr int OPB = ORI_BS / OCT;
    __shared__ OctMeta m;
    __shared__ OctStack<OPB> stk;
    if (threadIdx.x == 0) m = *a.t.meta;
    __syncthreads();
    const int lane = threadIdx.x & 63, oct = lane >> 3, ol = lane & 7, ob = threadIdx.x >> 3;
    const int s = blockIdx.x * OPB + ob;
    const bool inr = s < a.n;
    const float4 q = a.t.pts[inr ? s : 0];
    const int i = __float_as_int(q.w);
    int ci = -1, bj = INT_MAX;
    unsigned long long bk = ORI_NONE;                         // the bound: the component's best d^2 so far, then this row's own best (ties included)
    bool walk = false;
    if (inr && m.nl >= 1 && m.n >= 1 && (unsigned)i < (unsigned)a.n && a.cand_j[i] < 0) {
        ci = a.comp[i];
        bk = ori_load64(a.best_w + ci);
        const size_t last = (size_t)i * a.K + (a.K - 1);
        // every row of another component is at least as far as the last entry of a full list
        walk = !(a.lidx[last] >= 0 && (unsigned long long)__double_as_longlong(a.ld2[last]) > bk);
    }
    const unsigned long long wb = __ballot(walk && ol == 0);
    if (wb == 0ull) return;
    if (lane == 0) atomicAdd(&a.st->walked, (unsigned long long)__popcll(wb));
    int node = 0, s_first = 0, s_count = 0, s_parent = 0, s_sib = 0, s_nsib = 1;
    uint64_t s_key = 0;
    if (walk) {
        node = a.t.leaf_of[s];
        const size_t j = (size_t)(m.off[0] + node);
        s_first = __float_as_int(a.t.nodes[2 * j].w); s_count = __float_as_int(a.t.nodes[2 * j + 1].w);
        const int4 u = a.t.up[j]; s_key = a.t.keys[s_first];
        s_parent = u.x; s_sib = u.y; s_nsib = u.z;
    }
    float bnd = ori_bound(bk);
    auto visit = [&](int first, int count) {                  // wave-wide; count == 0: octet idle
        const int end = first + count;
        unsigned long long mk = ORI_NONE; int mj = INT_MAX;   // the best candidate this lane tested in the range
        for (int base = first; __ballot(base < end) != 0ull; base += OCT) {
            const int idx = base + ol;
            if (idx < end) {
                const float4 p = a.t.pts[idx];
                if (pcr_d2(p.x - q.x, p.y - q.y, p.z - q.z) < bnd) {
                    const int cj = __float_as_int(p.w);
                    if (a.comp[cj] != ci) {
                        const unsigned long long ck = (unsigned long long)__double_as_longlong(pcr_d2_f64_unfused(q, p));
                        if (ori_lt(ck, cj, mk, mj)) { mk = ck; mj = cj; }
                    }
                }
            }
        }
        ori_octet_min(mk, mj);
        if (ori_lt(mk, mj, bk, bj)) { bk = mk; bj = mj; bnd = ori_bound(bk); }
    };
    oct_search<OPB>(a.t, m, stk, walk, node, 0, s_first, s_count, s_key, s_parent, s_sib, s_nsib, q.x, q.y, q.z,
                    [&]() { return bnd; }, visit, [&](int nf, int) { return a.leaf_lab[a.t.leaf_of[nf]] == ci; }, ol, oct, ob);
    if (walk && ol == 0 && bj != INT_MAX) {
        a.cand_k[i] = bk; a.cand_j[i] = bj;
        ori_min64(a.best_w + ci, bk);
    }
}
__global__ void __launch_bounds__(ORI_BS) k_emst_pick(EmstArgs a) {
    const int i = blockIdx.x * ORI_BS + threadIdx.x;
    if (i >= a.n) return;
    const int j = a.cand_j[i];
    if (j < 0) return;
    const int ci = a.comp[i];
    if (a.cand_k[i] == a.best_w[ci]) ori_min64(a.best_e + ci, ori_pack(i, j));
}

// ============================================================================================================ hook and compress (both trees)
// nrm / par / hookpar: the TREE rounds (parity of a row relative to its root); null for the EMST.  out_w: the EMST's d^2 (null for TREE).
struct HookArgs {
    int n; const int *comp; const unsigned long long *best_w, *best_e; int *hook;
    const float *nrm; const uint8_t *par; uint8_t *hookpar;
    int32_t *out_e; double *out_w; OriState *st;
};
__global__ void __launch_bounds__(ORI_BS) k_ori_hook(HookArgs a) {
    const int c = blockIdx.x * ORI_BS + threadIdx.x;
    if (c >= a.n || a.comp[c] != c) return;
    const unsigned long long e = a.best_e[c];
    if (e == ORI_NONE) return;                                // no edge leaves the component (the last one)
    const int lo = (int)(unsigned)(e >> 32), hi = (int)(unsigned)e;
    if ((unsigned)lo >= (unsigned)a.n || (unsigned)hi >= (unsigned)a.n) return;
    const int cl = a.comp[lo], ch = a.comp[hi];
    const int other = cl == c ? ch : cl;
    if (other == c) return;
    if (a.best_e[other] == e && c < other) return;            // a mutual pick of this edge: the larger root hooks and emits
    a.hook[c] = other;
    if (a.hookpar) {
        const int in = cl == c ? lo : hi, out = cl == c ? hi : lo;
        a.hookpar[c] = (uint8_t)((a.par[in] ^ a.par[out] ^ (ori_dot(a.nrm, lo, hi) < 0.0 ? 1 : 0)) & 1);
    }
    const int slot = atomicAdd(&a.st->n_edges, 1);
    if (slot < a.n - 1) {
        a.out_e[2 * (size_t)slot] = lo; a.out_e[2 * (size_t)slot + 1] = hi;
        if (a.out_w) a.out_w[slot] = __longlong_as_double((long long)a.best_w[c]);
    }
}
__global__ void __launch_bounds__(ORI_BS) k_ori_compress(int n, const int *__restrict__ comp_in, const int *__restrict__ hook, const uint8_t *__restrict__ par_in,
                                                        const uint8_t *__restrict__ hookpar, int *__restrict__ comp_out, uint8_t *__restrict__ par_out) {
    const int i = blockIdx.x * ORI_BS + threadIdx.x;
    if (i >= n) return;
    int r = comp_in[i];
    uint8_t p = par_in ? par_in[i] : 0;
    for (int step = 0; step < n; step++) {
        const int h = hook[r];
        if (h == r || (unsigned)h >= (unsigned)n) break;
        if (hookpar) p ^= hookpar[r];
        r = h;
    }
    comp_out[i] = r;
    if (par_out) par_out[i] = p;
}

// ============================================================================================================ edges in (lo, hi) order
__global__ void __launch_bounds__(ORI_BS) k_ori_edge_keys(const int32_t *__restrict__ e, int count, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int t = blockIdx.x * ORI_BS + threadIdx.x;
    if (t >= count) return;
    keys[t] = ((uint64_t)(uint32_t)e[2 * (size_t)t] << 32) | (uint32_t)e[2 * (size_t)t + 1];
    vals[t] = (uint32_t)t;
}
__global__ void __launch_bounds__(ORI_BS) k_ori_edge_emit(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, const double *__restrict__ w_in, int count,
                                                         int32_t *__restrict__ e, double *__restrict__ w_out) {
    const int t = blockIdx.x * ORI_BS + threadIdx.x;
    if (t >= count) return;
    e[2 * (size_t)t] = (int32_t)(uint32_t)(keys[t] >> 32); e[2 * (size_t)t + 1] = (int32_t)(uint32_t)keys[t];
    if (w_out) w_out[t] = w_in[vals[t]];
}

// ============================================================================================================ TREE rounds
// GRAPH: slot e < n k is entry e % k of row e / k (the first k places of the list, the row itself skipped), the rest are the EMST's edges
struct TreeArgs {
    int n, k, K; size_t E;
    const int32_t *lidx; const int32_t *emst; const float *nrm;
    int *ea, *eb; unsigned long long *ew;
    const int *comp; unsigned long long *best_w, *best_e;
};
__global__ void __launch_bounds__(ORI_BS) k_tree_edges(TreeArgs a) {
    const size_t e = (size_t)blockIdx.x * ORI_BS + threadIdx.x;
    if (e >= a.E) return;
    const size_t nk = (size_t)a.n * (size_t)a.k;
    int u, v;
    if (e < nk) {
        u = (int)(e / (size_t)a.k);
        v = a.lidx[(size_t)u * a.K + (e % (size_t)a.k)];
        if (v < 0 || v == u) { a.ea[e] = -1; a.eb[e] = -1; a.ew[e] = ORI_NONE; return; }
    } else { u = a.emst[2 * (e - nk)]; v = a.emst[2 * (e - nk) + 1]; }
    a.ea[e] = u; a.eb[e] = v;
    a.ew[e] = ori_key_f64(1.0 - fabs(ori_dot(a.nrm, u, v)));
}
template <bool PICK>
__global__ void __launch_bounds__(ORI_BS) k_tree_cand(TreeArgs a) {
    const size_t e = (size_t)blockIdx.x * ORI_BS + threadIdx.x;
    if (e >= a.E) return;
    const int u = a.ea[e];
    if (u < 0) return;
    const int v = a.eb[e];
    const int cu = a.comp[u], cv = a.comp[v];
    if (cu == cv) return;
    const unsigned long long w = a.ew[e];
    if (!PICK) { ori_min64(a.best_w + cu, w); ori_min64(a.best_w + cv, w); return; }
    const unsigned long long p = ori_pack(u, v);
    if (w == a.best_w[cu]) ori_min64(a.best_e + cu, p);
    if (w == a.best_w[cv]) ori_min64(a.best_e + cv, p);
}

// ============================================================================================================ ROOT, PROPAGATE, RESULT
__global__ void __launch_bounds__(ORI_BS) k_ori_root_max(const float *__restrict__ xyz, int n, OriState *st) {
    const int i = blockIdx.x * ORI_BS + threadIdx.x;
    if (i >= n) return;
    const unsigned int key = ori_key_f32(xyz[(size_t)i * 3 + 2]);
    if (__hip_atomic_load(&st->zmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(&st->zmax, key);
}
__global__ void __launch_bounds__(ORI_BS) k_ori_root_min(const float *__restrict__ xyz, int n, OriState *st) {
    const int i = blockIdx.x * ORI_BS + threadIdx.x;
    if (i >= n) return;
    if (ori_key_f32(xyz[(size_t)i * 3 + 2]) == st->zmax) atomicMin(&st->root, i);
}
// flip_r is taken by one thread before any row is negated: k_ori_flip reads the record, never another row's normal
__global__ void k_ori_root_sign(const float *__restrict__ nrm, OriState *st) {
    if (blockIdx.x == 0 && threadIdx.x == 0) st->flip_root = nrm[(size_t)st->root * 3 + 2] < 0.0f ? 1 : 0;
}
__global__ void __launch_bounds__(ORI_BS) k_ori_flip(float *nrm, int n, const uint8_t *__restrict__ par, OriState *st, uint8_t *__restrict__ flipped) {
    const int i = blockIdx.x * ORI_BS + threadIdx.x;
    bool f = false;
    if (i < n) {
        f = (((par[i] ^ par[st->root]) & 1) ^ (st->flip_root & 1)) != 0;
        if (f) { nrm[(size_t)i * 3] = -nrm[(size_t)i * 3]; nrm[(size_t)i * 3 + 1] = -nrm[(size_t)i * 3 + 1]; nrm[(size_t)i * 3 + 2] = -nrm[(size_t)i * 3 + 2]; }
        if (flipped) flipped[i] = f ? 1 : 0;
    }
    const unsigned long long b = __ballot(f);
    if (b != 0ull && (threadIdx.x & 63) == 0) atomicAdd(&st->n_flipped, (int)__popcll(b));
}

// ============================================================================================================ element-wise
// mode 0 direction(ref), 1 camera(loc), 2 normalize; float64 on the float32 data, sums in the order x, y, z
__global__ void __launch_bounds__(ORI_BS) k_ori_elementwise(const float *__restrict__ xyz, float *nrm, int n, int mode, double rx, double ry, double rz) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * ORI_BS + threadIdx.x;
    if (i >= n) return;
    const float fx = nrm[(size_t)i * 3], fy = nrm[(size_t)i * 3 + 1], fz = nrm[(size_t)i * 3 + 2];
    const double x = (double)fx, y = (double)fy, z = (double)fz;
    const bool zero = fx == 0.0f && fy == 0.0f && fz == 0.0f;
    if (mode == 2) {
        if (zero) return;
        double s = x * x; s += y * y; s += z * z;
        const double len = __dsqrt_rn(s);
        nrm[(size_t)i * 3] = (float)__ddiv_rn(x, len); nrm[(size_t)i * 3 + 1] = (float)__ddiv_rn(y, len); nrm[(size_t)i * 3 + 2] = (float)__ddiv_rn(z, len);
        return;
    }
    double vx = rx, vy = ry, vz = rz;
    if (mode == 1) { vx = rx - (double)xyz[(size_t)i * 3]; vy = ry - (double)xyz[(size_t)i * 3 + 1]; vz = rz - (double)xyz[(size_t)i * 3 + 2]; }
    if (zero) {
        if (mode == 1) {
            double s = vx * vx; s += vy * vy; s += vz * vz;
            const double len = __dsqrt_rn(s);
            if (len == 0.0) { vx = 0.0; vy = 0.0; vz = 1.0; }
            else { vx = __ddiv_rn(vx, len); vy = __ddiv_rn(vy, len); vz = __ddiv_rn(vz, len); }
        }
        nrm[(size_t)i * 3] = (float)vx; nrm[(size_t)i * 3 + 1] = (float)vy; nrm[(size_t)i * 3 + 2] = (float)vz;
        return;
    }
    double d = x * vx; d += y * vy; d += z * vz;
    if (d < 0.0) { nrm[(size_t)i * 3] = -fx; nrm[(size_t)i * 3 + 1] = -fy; nrm[(size_t)i * 3 + 2] = -fz; }
}

// ============================================================================================================ host
static inline dim3 ori_grid(size_t work) { return dim3((unsigned)((work + ORI_BS - 1) / ORI_BS)); }
static int ori_ceil_log2(int64_t n) { int r = 0; while (((int64_t)1 << r) < n) r++; return r; }
static double ori_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static int ori_read_state(pcr_context *ctx, const OriState *st, OriState *h) {
    PCR_HIP_CHECK(ctx, hipMemcpyAsync(h, st, sizeof *h, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

struct OriWork {                               // what both trees share, from the arena
    int n = 0, K = 0;
    DevCloud c; uint32_t *perm = nullptr;
    int32_t *lidx = nullptr; double *ld2 = nullptr;
    int *comp[2] = {nullptr, nullptr}, *hook = nullptr, *leaf_lab = nullptr, *cand_j = nullptr;
    unsigned long long *best_w = nullptr, *best_e = nullptr, *cand_k = nullptr;
    int32_t *raw_e = nullptr, *emst = nullptr; double *raw_w = nullptr;     // edges in emission order; the EMST in (lo, hi) order
    uint64_t *k0 = nullptr, *k1 = nullptr; uint32_t *v0 = nullptr, *v1 = nullptr; void *sort_tmp = nullptr; size_t sort_bytes = 0;
    OriState *st = nullptr;
};
// arena bytes of a run on n rows with lists of K entries and (TREE) k graph entries per row
static size_t ori_bytes(int64_t n, int K, int k) {
    const size_t nn = (size_t)n;
    return pcr_scratch_bytes_for(n) + nn * 64 + nn * (size_t)K * 12 + nn * 128 + pcr_sort_temp_bytes(nn) + (nn * (size_t)k + nn) * 16 + (1u << 16);
}
// state record + non-finite check (before anything else touches the cloud); *bad on the host
static int ori_check(pcr_context *ctx, OriWork &w, const float *xyz, const float *nrm, int64_t n, bool *bad) {
    w.st = arena<OriState>(ctx, 1);
    if (!w.st) return PCR_ENOMEM;
    PCR_HIP_CHECK(ctx, hipMemsetAsync(w.st, 0, sizeof(OriState), ctx->stream));
    PCR_LAUNCH(ctx, k_ori_check, ori_grid((size_t)n * 3), dim3(ORI_BS), 0, ctx->stream, xyz, nrm, (size_t)n * 3, w.st);
    OriState h;
    PCR_TRY(ori_read_state(ctx, w.st, &h));
    *bad = h.bad != 0;
    return PCR_OK;
}
// sorted cloud with its octree, caller rows in w, the lists of K entries, and the per-row arrays (n >= 2)
static int ori_prepare(pcr_context *ctx, OriWork &w, const float *xyz, int64_t n, int K) {
    w.n = (int)n; w.K = K;
    PCR_TRY(pcr_import_cloud(ctx, xyz, nullptr, n, &w.c, &w.perm, false));
    PCR_LAUNCH(ctx, k_ori_tag, ori_grid(n), dim3(ORI_BS), 0, ctx->stream, w.c.pts, (const uint32_t *)w.perm, (int)n);
    w.lidx = arena<int32_t>(ctx, (size_t)n * K); w.ld2 = arena<double>(ctx, (size_t)n * K);
    w.comp[0] = arena<int>(ctx, n); w.comp[1] = arena<int>(ctx, n); w.hook = arena<int>(ctx, n); w.leaf_lab = arena<int>(ctx, n); w.cand_j = arena<int>(ctx, n);
    w.best_w = arena<unsigned long long>(ctx, n); w.best_e = arena<unsigned long long>(ctx, n); w.cand_k = arena<unsigned long long>(ctx, n);
    w.raw_e = arena<int32_t>(ctx, 2 * (size_t)n); w.emst = arena<int32_t>(ctx, 2 * (size_t)n); w.raw_w = arena<double>(ctx, n);
    w.k0 = arena<uint64_t>(ctx, n); w.k1 = arena<uint64_t>(ctx, n); w.v0 = arena<uint32_t>(ctx, n); w.v1 = arena<uint32_t>(ctx, n);
    w.sort_bytes = pcr_sort_temp_bytes((size_t)n); w.sort_tmp = pcr_arena_alloc(ctx, w.sort_bytes);
    if (!w.lidx || !w.ld2 || !w.comp[0] || !w.comp[1] || !w.hook || !w.leaf_lab || !w.cand_j || !w.best_w || !w.best_e || !w.cand_k || !w.raw_e || !w.emst || !w.raw_w ||
        !w.k0 || !w.k1 || !w.v0 || !w.v1 || !w.sort_tmp) return PCR_ENOMEM;
    // the lists in caller rows; the queries are taken in the cloud's Morton order (perm), every row written to its caller position
    if (ctx->profiling) PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    const double t0 = ori_now_ms();
    PCR_TRY(pcr_dev_tagged_knn(ctx, &w.c, xyz, n, w.perm, K, w.lidx, w.ld2));
    if (ctx->profiling) {
        PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        fprintf(stderr, "orient: lists of %d entries for %d rows: %.3f ms (after the sorted copy and its octree)\n", K, (int)n, ori_now_ms() - t0);
    }
    return PCR_OK;
}
// the n - 1 edges of raw_e (emission order) into `edges` in (lo, hi) order, their weights along
static int ori_sort_edges(pcr_context *ctx, OriWork &w, int32_t *edges, double *w_out) {
    const int m = w.n - 1;
    if (m < 1) return PCR_OK;
    PCR_LAUNCH(ctx, k_ori_edge_keys, ori_grid(m), dim3(ORI_BS), 0, ctx->stream, (const int32_t *)w.raw_e, m, w.k0, w.v0);
    PCR_TRY(pcr_sort_pairs(ctx, w.sort_tmp, w.sort_bytes, w.k0, w.k1, w.v0, w.v1, (size_t)m, 64));
    PCR_LAUNCH(ctx, k_ori_edge_emit, ori_grid(m), dim3(ORI_BS), 0, ctx->stream, (const uint64_t *)w.k1, (const uint32_t *)w.v1, (const double *)w.raw_w, m, edges, w_out);
    return PCR_OK;
}
// one tree by rounds: `round` enqueues the candidate kernels of a round over the labels comp[cur]; the hook, the compression and the read of
// the small record are shared.  *cur: the label array that is current afterwards.
template <class RoundFn>
static int ori_rounds(pcr_context *ctx, OriWork &w, const char *what, const float *nrm, uint8_t *const *par, uint8_t *hookpar, double *raw_w, int *cur, int *rounds_out,
                      RoundFn round) {
    const int n = w.n, max_rounds = ori_ceil_log2(n);
    PCR_LAUNCH(ctx, k_ori_init, ori_grid(n), dim3(ORI_BS), 0, ctx->stream, n, w.comp[0], w.hook, par ? par[0] : (uint8_t *)nullptr);
    PCR_HIP_CHECK(ctx, hipMemsetAsync(&w.st->n_edges, 0, sizeof(int), ctx->stream));
    int have = 0, rounds = 0, c = 0;
    unsigned long long walked = 0;                            // (profiling: the rows that had walked before this round; only the EMST rounds walk)
    while (have < n - 1) {
        const double t0 = ori_now_ms();
        if (rounds >= max_rounds) { ctx->err = std::string(what) + ": the rounds did not end at one component"; return PCR_ENUMERIC; }
        PCR_HIP_CHECK(ctx, hipMemsetAsync(w.best_w, 0xff, (size_t)n * sizeof(unsigned long long), ctx->stream));
        PCR_HIP_CHECK(ctx, hipMemsetAsync(w.best_e, 0xff, (size_t)n * sizeof(unsigned long long), ctx->stream));
        PCR_TRY(round(c));
        HookArgs h; h.n = n; h.comp = w.comp[c]; h.best_w = w.best_w; h.best_e = w.best_e; h.hook = w.hook; h.nrm = nrm; h.par = par ? par[c] : nullptr; h.hookpar = hookpar;
        h.out_e = w.raw_e; h.out_w = raw_w; h.st = w.st;
        PCR_LAUNCH(ctx, k_ori_hook, ori_grid(n), dim3(ORI_BS), 0, ctx->stream, h);
        PCR_LAUNCH(ctx, k_ori_compress, ori_grid(n), dim3(ORI_BS), 0, ctx->stream, n, (const int *)w.comp[c], (const int *)w.hook, (const uint8_t *)(par ? par[c] : nullptr),
                   (const uint8_t *)hookpar, w.comp[c ^ 1], par ? par[c ^ 1] : (uint8_t *)nullptr);
        c ^= 1;
        OriState s;
        PCR_TRY(ori_read_state(ctx, w.st, &s));
        if (s.n_edges <= have || s.n_edges > n - 1) { ctx->err = std::string(what) + ": a round joined no component"; return PCR_ENUMERIC; }
        // with profiling on (pcr_profile_enable), one line per round: every round ends in the read above, so the host clock brackets device work
        if (par) walked = s.walked;
        if (ctx->profiling) fprintf(stderr, "%s: %s round %d: %d edges, %llu rows walked, %.3f ms\n", what, par ? "TREE" : "EMST", rounds + 1, s.n_edges - have,
                                    s.walked - walked, ori_now_ms() - t0);
        walked = s.walked;
        have = s.n_edges;
        rounds++;
    }
    *cur = c; *rounds_out = rounds;
    return PCR_OK;
}
// EMST of the prepared cloud into w.emst ((lo, hi) order), d^2 into d2_out when asked for
static int ori_emst(pcr_context *ctx, OriWork &w, const char *what, double *d2_out, int *rounds) {
    int cur = 0;
    PCR_TRY(ori_rounds(ctx, w, what, nullptr, nullptr, nullptr, w.raw_w, &cur, rounds, [&](int c) -> int {
        EmstArgs a; a.t = oct_view(&w.c); a.n = w.n; a.K = w.K; a.lidx = w.lidx; a.ld2 = w.ld2; a.comp = w.comp[c]; a.leaf_lab = w.leaf_lab;
        a.best_w = w.best_w; a.best_e = w.best_e; a.cand_k = w.cand_k; a.cand_j = w.cand_j; a.st = w.st;
        PCR_LAUNCH(ctx, k_ori_leaf_labels, ori_grid(w.n), dim3(ORI_BS), 0, ctx->stream, a.t, w.n, (const int *)w.comp[c], w.leaf_lab);
        PCR_LAUNCH(ctx, k_emst_list, ori_grid(w.n), dim3(ORI_BS), 0, ctx->stream, a);
        PCR_LAUNCH(ctx, k_emst_walk, ori_grid((size_t)w.n * OCT), dim3(ORI_BS), 0, ctx->stream, a);
        PCR_LAUNCH(ctx, k_emst_pick, ori_grid(w.n), dim3(ORI_BS), 0, ctx->stream, a);
        return PCR_OK;
    }));
    return ori_sort_edges(ctx, w, w.emst, d2_out);
}
static void ori_info(pcr_orient_info *info, int emst_rounds, int tree_rounds, const OriState &s, int64_t root) {
    if (!info) return;
    info->emst_rounds = emst_rounds; info->tree_rounds = tree_rounds; info->walked_rows = (int64_t)s.walked; info->n_flipped = s.n_flipped; info->root = root;
}

extern "C" int pcr_euclidean_mst(pcr_context *ctx, const float *xyz, int64_t n, int32_t *edges, double *d2, pcr_orient_info *info) {
    return pcr_api_call(ctx, [&]() -> int {
        const char *what = "euclidean_minimum_spanning_tree";
        if (n < 0 || n > ORI_MAX_POINTS) { ctx->err = std::string(what) + ": n is negative or over the int limit"; return PCR_EINVAL; }
        if (n > 0 && !xyz) { ctx->err = std::string(what) + ": null cloud"; return PCR_EINVAL; }
        if (n > 1 && !edges) { ctx->err = std::string(what) + ": null edges pointer"; return PCR_EINVAL; }
        OriState s; memset(&s, 0, sizeof s);
        ori_info(info, 0, 0, s, -1);
        if (n == 0) return PCR_OK;
        PCR_TRY(pcr_arena_reserve(ctx, ori_bytes(n, ORI_LIST_MIN, 0)));
        OriWork w; bool bad = false;
        PCR_TRY(ori_check(ctx, w, xyz, nullptr, n, &bad));
        if (bad) { ctx->err = std::string(what) + ": non-finite coordinate"; return PCR_EINVAL; }
        if (n == 1) return PCR_OK;
        PCR_TRY(ori_prepare(ctx, w, xyz, n, ORI_LIST_MIN));
        int rounds = 0;
        PCR_TRY(ori_emst(ctx, w, what, d2, &rounds));
        PCR_HIP_CHECK(ctx, hipMemcpyAsync(edges, w.emst, 2 * (size_t)(n - 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
        PCR_TRY(ori_read_state(ctx, w.st, &s));
        ori_info(info, rounds, 0, s, -1);
        return PCR_OK;
    });
}

extern "C" int pcr_orient_normals_tangent_plane(pcr_context *ctx, const float *xyz, float *normals, int64_t n, int k, uint8_t *flipped, int32_t *tree_edges,
                                                pcr_orient_info *info) {
    return pcr_api_call(ctx, [&]() -> int {
        const char *what = "orient_normals_consistent_tangent_plane";
        if (n < 0 || n > ORI_MAX_POINTS) { ctx->err = std::string(what) + ": n is negative or over the int limit"; return PCR_EINVAL; }
        if (n > 0 && (!xyz || !normals)) { ctx->err = std::string(what) + ": null cloud or normals pointer"; return PCR_EINVAL; }
        if (k < 0 || k > ORI_MAX_K) { ctx->err = std::string(what) + ": k outside 0..200"; return PCR_EINVAL; }
        OriState s; memset(&s, 0, sizeof s);
        ori_info(info, 0, 0, s, -1);
        if (n == 0) return PCR_OK;
        const int K = k > ORI_LIST_MIN ? k : ORI_LIST_MIN;
        PCR_TRY(pcr_arena_reserve(ctx, ori_bytes(n, K, k)));
        OriWork w; bool bad = false;
        PCR_TRY(ori_check(ctx, w, xyz, normals, n, &bad));
        if (bad) { ctx->err = std::string(what) + ": non-finite coordinate or normal component"; return PCR_EINVAL; }
        uint8_t *par[2] = {arena<uint8_t>(ctx, n), arena<uint8_t>(ctx, n)}, *hookpar = arena<uint8_t>(ctx, n);
        if (!par[0] || !par[1] || !hookpar) return PCR_ENOMEM;
        int emst_rounds = 0, tree_rounds = 0, cur = 0;
        if (n == 1) PCR_HIP_CHECK(ctx, hipMemsetAsync(par[0], 0, 1, ctx->stream));
        else {
            PCR_TRY(ori_prepare(ctx, w, xyz, n, K));
            PCR_TRY(ori_emst(ctx, w, what, nullptr, &emst_rounds));
            TreeArgs t; t.n = (int)n; t.k = k; t.K = K; t.E = (size_t)n * (size_t)k + (size_t)(n - 1); t.lidx = w.lidx; t.emst = w.emst; t.nrm = normals;
            t.ea = arena<int>(ctx, t.E); t.eb = arena<int>(ctx, t.E); t.ew = arena<unsigned long long>(ctx, t.E);
            t.comp = nullptr; t.best_w = w.best_w; t.best_e = w.best_e;
            if (!t.ea || !t.eb || !t.ew) return PCR_ENOMEM;
            PCR_LAUNCH(ctx, k_tree_edges, ori_grid(t.E), dim3(ORI_BS), 0, ctx->stream, t);
            PCR_TRY(ori_rounds(ctx, w, what, normals, par, hookpar, nullptr, &cur, &tree_rounds, [&](int c) -> int {
                t.comp = w.comp[c];
                PCR_LAUNCH(ctx, k_tree_cand<false>, ori_grid(t.E), dim3(ORI_BS), 0, ctx->stream, t);
                PCR_LAUNCH(ctx, k_tree_cand<true>, ori_grid(t.E), dim3(ORI_BS), 0, ctx->stream, t);
                return PCR_OK;
            }));
            if (tree_edges) PCR_TRY(ori_sort_edges(ctx, w, tree_edges, nullptr));
        }
        PCR_HIP_CHECK(ctx, hipMemsetAsync(&w.st->root, 0x7f, sizeof(int), ctx->stream));
        PCR_LAUNCH(ctx, k_ori_root_max, ori_grid(n), dim3(ORI_BS), 0, ctx->stream, xyz, (int)n, w.st);
        PCR_LAUNCH(ctx, k_ori_root_min, ori_grid(n), dim3(ORI_BS), 0, ctx->stream, xyz, (int)n, w.st);
        PCR_LAUNCH(ctx, k_ori_root_sign, dim3(1), dim3(64), 0, ctx->stream, (const float *)normals, w.st);
        PCR_LAUNCH(ctx, k_ori_flip, ori_grid(n), dim3(ORI_BS), 0, ctx->stream, normals, (int)n, (const uint8_t *)par[cur], w.st, flipped);
        PCR_TRY(ori_read_state(ctx, w.st, &s));
        ori_info(info, emst_rounds, tree_rounds, s, s.root);
        return PCR_OK;
    });
}

static int ori_elementwise(pcr_context *ctx, const char *what, const float *xyz, float *normals, int64_t n, int mode, const double *ref) {
    if (n < 0 || n > ORI_MAX_POINTS) { ctx->err = std::string(what) + ": n is negative or over the int limit"; return PCR_EINVAL; }
    if (n > 0 && !normals) { ctx->err = std::string(what) + ": null normals pointer"; return PCR_EINVAL; }
    if (mode < 0 || mode > 2) { ctx->err = std::string(what) + ": mode must be 0 (direction) or 1 (camera)"; return PCR_EINVAL; }
    if (mode != 2 && !ref) { ctx->err = std::string(what) + ": null reference"; return PCR_EINVAL; }
    if (mode == 1 && n > 0 && !xyz) { ctx->err = std::string(what) + ": the camera mode needs the cloud"; return PCR_EINVAL; }
    if (n == 0) return PCR_OK;
    PCR_LAUNCH(ctx, k_ori_elementwise, ori_grid(n), dim3(ORI_BS), 0, ctx->stream, xyz, normals, (int)n, mode, ref ? ref[0] : 0.0, ref ? ref[1] : 0.0, ref ? ref[2] : 0.0);
    return PCR_OK;
}
extern "C" int pcr_orient_normals(pcr_context *ctx, const float *xyz, float *normals, int64_t n, int mode, const double ref[3]) {
    return pcr_api_call(ctx, [&]() -> int {
        if (mode == 2) { ctx->err = "orient_normals: mode must be 0 (direction) or 1 (camera)"; return PCR_EINVAL; }
        return ori_elementwise(ctx, "orient_normals", xyz, normals, n, mode, ref);
    });
}
extern "C" int pcr_normalize_normals(pcr_context *ctx, float *normals, int64_t n) {
    return pcr_api_call(ctx, [&]() -> int { return ori_elementwise(ctx, "normalize_normals", nullptr, normals, n, 2, nullptr); });
}
