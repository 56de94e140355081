// pcr_search.hip -- the public nearest-neighbour search on gfx950: a persistent index over a cloud and three batched searches (k nearest,
// all within a radius, the nearest max_nn within a radius) over arbitrary query points.
// Reference behaviour: Open3D KDTreeFlann::{SearchKNN, SearchRadius, SearchHybrid} and core::nns::NearestNeighborSearch (the rule is
// stated next to the entry points in include/pcr_hip.h).  The index is the Morton-sorted cloud with the octree of pcr_octree.h in ONE
// device allocation of its own; the searches walk it with one query per octet, each with its own bottom-up walk from its greedy leaf
// (oct_search), like k_cloud_distance.  Nothing here touches the kernels of the other units.
//
// ONE ORDER for the three searches: the dataset is ordered for a query by (float64 d^2 unfused, caller index).  Candidates are screened
// with the float32 d^2 against a slightly wide float bound; only the survivors get their float64 key, and the k-best keeps (key bits,
// caller index) pairs -- d^2 >= 0, so the bits order like the values.
#include <cstring>
#include "pcr_octree.h"

#define SRCH_BS 256
#define SRCH_FAR 3.4e38f
#define SRCH_EMPTY_K 0xffffffffffffffffull       // an unfilled place of a k-best: larger than the bits of every d^2 (+inf included)
#define SRCH_EMPTY_I 0x7fffffff
#define SRCH_MAX_POINTS 0x7fffffffLL             // the clouds of this library are counted in int
#define SRCH_MAX_K 200

struct pcr_index {
    int device = 0;
    int64_t n = 0;
    char *block = nullptr;       // the one allocation: sorted points (w = caller index), keys, octree
    size_t bytes = 0;
    DevCloud c;
};

__device__ static inline bool srch_lt(unsigned long long ak, int ai, unsigned long long bk, int bi) { return ak < bk || (ak == bk && ai < bi); }
template <int CTRL> __device__ static inline unsigned long long srch_dpp_u64(unsigned long long v) {
    const unsigned lo = (unsigned)pcr_dpp_i<CTRL>((int)(unsigned)v), hi = (unsigned)pcr_dpp_i<CTRL>((int)(unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// smallest (key, caller index) of the octet, in all 8 lanes
__device__ static inline void srch_octet_min(unsigned long long &k, int &i) {
    { const unsigned long long o = srch_dpp_u64<PCR_DPP_XOR1>(k); const int oi = pcr_dpp_i<PCR_DPP_XOR1>(i); if (srch_lt(o, oi, k, i)) { k = o; i = oi; } }
    { const unsigned long long o = srch_dpp_u64<PCR_DPP_XOR2>(k); const int oi = pcr_dpp_i<PCR_DPP_XOR2>(i); if (srch_lt(o, oi, k, i)) { k = o; i = oi; } }
    { const unsigned long long o = srch_dpp_u64<PCR_DPP_HMIRROR>(k); const int oi = pcr_dpp_i<PCR_DPP_HMIRROR>(i); if (srch_lt(o, oi, k, i)) { k = o; i = oi; } }
}

// The octet's k-best by (key, caller index): slot s lives in lane s % 8, register s / 8, every lane keeps its registers in DESCENDING
// order (places beyond k, (0, -1), at the end: smaller than every entry), so the octet's worst entry is the 8-lane maximum of the
// heads.  An equal key with a lower caller index IS smaller and displaces the worst.  `bnd` is the float32 bound of the walk: the wide
// float of the worst key, never below the smallest normal float -- a worst key of 0 (k copies of the query) must still let the strict
// box and screen tests pass the other copies -- and never above `cap` (the radius of the hybrid search).
template <int SLOTS>
struct OctetBest {
    unsigned long long sk[SLOTS]; int si[SLOTS];
    unsigned long long wk; int wi;       // the octet's worst entry (octet-uniform)
    int wlane, ol;
    float cap, bnd;
    __device__ void init(int k, float cap_, int ol_) {
        ol = ol_; cap = cap_;
#pragma unroll
        for (int j = 0; j < SLOTS; j++) { const bool on = ol + OCT * j < k; sk[j] = on ? SRCH_EMPTY_K : 0ull; si[j] = on ? SRCH_EMPTY_I : -1; }
        refresh();
    }
    __device__ void refresh() {
        unsigned long long k = sk[0]; int i = si[0];
        { const unsigned long long o = srch_dpp_u64<PCR_DPP_XOR1>(k); const int oi = pcr_dpp_i<PCR_DPP_XOR1>(i); if (srch_lt(k, i, o, oi)) { k = o; i = oi; } }
        { const unsigned long long o = srch_dpp_u64<PCR_DPP_XOR2>(k); const int oi = pcr_dpp_i<PCR_DPP_XOR2>(i); if (srch_lt(k, i, o, oi)) { k = o; i = oi; } }
        { const unsigned long long o = srch_dpp_u64<PCR_DPP_HMIRROR>(k); const int oi = pcr_dpp_i<PCR_DPP_HMIRROR>(i); if (srch_lt(k, i, o, oi)) { k = o; i = oi; } }
        wk = k; wi = i;
        const unsigned long long own = __ballot(sk[0] == wk && si[0] == wi);
        wlane = __builtin_ctz(((uint32_t)(own >> (threadIdx.x & 56)) & 0xffu) | 0x100u) & 7;
        float b = cap;
        if (wk != SRCH_EMPTY_K) b = fminf(fmaxf((float)(__longlong_as_double((long long)wk) * (1.0 + 1e-6)), 1.17549435e-38f), cap);
        bnd = b;
    }
    // All 8 lanes call with the same candidate.  One below the worst replaces the head of the owning lane and sinks with one pass of
    // compare-exchanges; one that is not below the worst (an unfilled place, the dummy of an octet without candidates) changes nothing.
    __device__ void insert(unsigned long long ck, int ci) {
        const bool own = ol == wlane && srch_lt(ck, ci, wk, wi);
        sk[0] = own ? ck : sk[0]; si[0] = own ? ci : si[0];
#pragma unroll
        for (int j = 0; j + 1 < SLOTS; j++) {
            const bool sw = srch_lt(sk[j], si[j], sk[j + 1], si[j + 1]);
            const unsigned long long a = sk[j], b = sk[j + 1]; const int ia = si[j], ib = si[j + 1];
            sk[j] = sw ? b : a; sk[j + 1] = sw ? a : b; si[j] = sw ? ib : ia; si[j + 1] = sw ? ia : ib;
        }
        refresh();
    }
    // drop the worst entry (the owner's head): the next worst becomes (wk, wi)
    __device__ void pop() {
        const bool own = ol == wlane;
#pragma unroll
        for (int j = 0; j + 1 < SLOTS; j++) { sk[j] = own ? sk[j + 1] : sk[j]; si[j] = own ? si[j + 1] : si[j]; }
        sk[SLOTS - 1] = own ? 0ull : sk[SLOTS - 1]; si[SLOTS - 1] = own ? -1 : si[SLOTS - 1];
        refresh();
    }
};

struct SearchArgs {
    OctView t; const float *q; const uint32_t *qperm; int m;     // queries (caller rows); qperm: optional order in which the octets take them
    int k; float r2f; double r2;
    int32_t *idx; double *d2; int32_t *counts;
    const int64_t *splits; int sort;                             // radius fill
};

// the frame of the four kernels: the octet's query, and the record of its greedy leaf for oct_search
struct SearchQuery { int i; bool inr, live; float4 q; int node, s_first, s_count, s_parent, s_sib, s_nsib; uint64_t s_key; };
__device__ static inline SearchQuery srch_query(const SearchArgs &a, const OctMeta &m, int slot, int ol) {
    SearchQuery s = {};
    s.inr = slot < a.m;
    s.i = s.inr ? (a.qperm ? (int)a.qperm[slot] : slot) : 0;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    if (s.inr) { qx = a.q[(size_t)s.i * 3]; qy = a.q[(size_t)s.i * 3 + 1]; qz = a.q[(size_t)s.i * 3 + 2]; }
    s.q = make_float4(qx, qy, qz, 0.0f);
    // a query with a non-finite coordinate finds nothing
    s.live = s.inr && fabsf(qx) <= 3.4028235e38f && fabsf(qy) <= 3.4028235e38f && fabsf(qz) <= 3.4028235e38f && m.nl >= 1 && m.n >= 1;
    s.s_nsib = 1;
    const int g = oct_greedy_leaf(a.t, m, s.live, qx, qy, qz, ol);
    if (s.live) {
        s.node = g;
        const size_t j = (size_t)(m.off[0] + g);
        s.s_first = __float_as_int(a.t.nodes[2 * j].w); s.s_count = __float_as_int(a.t.nodes[2 * j + 1].w);
        const int4 u = a.t.up[j]; s.s_key = a.t.keys[s.s_first];
        s.s_parent = u.x; s.s_sib = u.y; s.s_nsib = u.z;
    }
    return s;
}

// ============================================================================================ k nearest / hybrid
// HYBRID: the k-best's bound starts at the wide float of r^2 and a candidate must pass d^2 < r^2 (strict, float64) as well.  The rows
// come out by K pops of the octet's worst entry, last place first; unfilled places are the first to go and become the padding.
// ONE (k = 1): only the smallest candidate of a range can enter, so every lane keeps the best of the candidates it tested and the octet
// inserts its minimum once per range -- the reduction of k_cloud_distance on (key, caller index) -- instead of one round per candidate.
template <int SLOTS, bool HYBRID, bool ONE>
__global__ void __launch_bounds__(SRCH_BS) k_index_knn(SearchArgs a) {
    constexpr int OPB = SRCH_BS / OCT;
    __shared__ OctMeta m;
    __shared__ OctStack<OPB> stk;
    if (threadIdx.x == 0) m = *a.t.meta;
    __syncthreads();
    const int lane = threadIdx.x & 63, oct = lane >> 3, ol = lane & 7, ob = threadIdx.x >> 3;
    const SearchQuery s = srch_query(a, m, blockIdx.x * OPB + ob, ol);
    if (__ballot(s.inr) == 0ull) return;
    OctetBest<SLOTS> tk;
    tk.init(a.k, HYBRID ? a.r2f : SRCH_FAR, ol);
    auto visit = [&](int first, int count) {                 // wave-wide; count == 0: octet idle
        int base = first; const int end = first + count;
        unsigned long long mk = SRCH_EMPTY_K; int mi = SRCH_EMPTY_I;        // ONE: the best candidate this lane tested in the range
        while (__ballot(base < end) != 0ull) {
            float4 p[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { const int idx = base + OCT * u + ol; p[u] = a.t.pts[idx < end ? idx : (end > first ? end - 1 : 0)]; }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int idx = base + OCT * u + ol;
                unsigned long long ck = SRCH_EMPTY_K; int ci = SRCH_EMPTY_I; bool pass = false;
                if (idx < end && pcr_d2(p[u].x - s.q.x, p[u].y - s.q.y, p[u].z - s.q.z) < tk.bnd) {
                    const double d = pcr_d2_f64_unfused(s.q, p[u]);
                    if (!HYBRID || d < a.r2) { ck = (unsigned long long)__double_as_longlong(d); ci = __float_as_int(p[u].w); pass = srch_lt(ck, ci, tk.wk, tk.wi); }
                }
                if (ONE) { if (pass && srch_lt(ck, ci, mk, mi)) { mk = ck; mi = ci; } continue; }
                unsigned long long bal = __ballot(pass);
                uint32_t surv = (uint32_t)(bal >> (oct * 8)) & 0xffu;
                while (bal != 0ull) {                        // one candidate per octet and round
                    const int sl = __builtin_ctz(surv | 0x100u) & 7;
                    const unsigned long long bk = __shfl(ck, sl, OCT); const int bi = __shfl(ci, sl, OCT);
                    tk.insert(surv ? bk : SRCH_EMPTY_K, surv ? bi : SRCH_EMPTY_I);
                    surv &= surv - 1;
                    bal = __ballot(surv != 0);
                }
            }
            base += 4 * OCT;
        }
        if (ONE) { srch_octet_min(mk, mi); tk.insert(mk, mi); }
    };
    if (__ballot(s.live) != 0ull)
        oct_search<OPB>(a.t, m, stk, s.live, s.node, 0, s.s_first, s.s_count, s.s_key, s.s_parent, s.s_sib, s.s_nsib, s.q.x, s.q.y, s.q.z,
                        [&]() { return tk.bnd; }, visit, [](int, int) { return false; }, ol, oct, ob);
    int cnt = 0;
    const double pad = HYBRID ? 0.0 : (double)__builtin_inff();
    for (int t = a.k - 1; t >= 0; t--) {
        const bool real = tk.wk != SRCH_EMPTY_K;
        if (s.inr && ol == 0) {
            const size_t o = (size_t)s.i * (size_t)a.k + (size_t)t;
            a.idx[o] = real ? tk.wi : -1;
            a.d2[o] = real ? __longlong_as_double((long long)tk.wk) : pad;
        }
        cnt += real ? 1 : 0;
        tk.pop();
    }
    if (a.counts && s.inr && ol == 0) a.counts[s.i] = cnt;
}

// ================================================================================================ radius: count, then fill
// The same walk with the fixed bound.  FILL writes every member into the query's segment [splits[i], splits[i + 1]) in walk order and,
// asked to sort, the octet then orders its segment in place with a bitonic network whose comparators all put the smaller entry at the
// lower position: places at and beyond the segment's end act as +inf and never move, so any length sorts without padding.
template <bool FILL>
__global__ void __launch_bounds__(SRCH_BS) k_index_radius(SearchArgs a) {
    constexpr int OPB = SRCH_BS / OCT;
    __shared__ OctMeta m;
    __shared__ OctStack<OPB> stk;
    if (threadIdx.x == 0) m = *a.t.meta;
    __syncthreads();
    const int lane = threadIdx.x & 63, oct = lane >> 3, ol = lane & 7, ob = threadIdx.x >> 3;
    const SearchQuery s = srch_query(a, m, blockIdx.x * OPB + ob, ol);
    if (__ballot(s.inr) == 0ull) return;
    int64_t seg = 0; int room = 0;
    if (FILL && s.inr) { seg = a.splits[s.i]; const int64_t r = a.splits[s.i + 1] - seg; room = r < 0 ? 0 : (r > 0x7fffffffLL ? 0x7fffffff : (int)r); }
    int total = 0;                                            // FILL: members so far (octet-uniform); else this lane's count
    auto visit = [&](int first, int count) {
        const int end = first + count;
        for (int base = first; __ballot(base < end) != 0ull; base += OCT) {
            const int idx = base + ol;
            bool in = false; double d = 0.0; int ci = 0;
            if (idx < end) {
                const float4 p = a.t.pts[idx];
                if (pcr_d2(p.x - s.q.x, p.y - s.q.y, p.z - s.q.z) < a.r2f) { d = pcr_d2_f64_unfused(s.q, p); in = d < a.r2; ci = __float_as_int(p.w); }
            }
            if (FILL) {
                const unsigned mask = (unsigned)(__ballot(in) >> (oct * 8)) & 0xffu;
                const int pos = total + __builtin_popcount(mask & ((1u << ol) - 1u));
                if (in && pos < room) { a.idx[seg + pos] = ci; a.d2[seg + pos] = d; }
                total += __builtin_popcount(mask);
            } else total += in ? 1 : 0;
        }
    };
    if (__ballot(s.live) != 0ull)
        oct_search<OPB>(a.t, m, stk, s.live, s.node, 0, s.s_first, s.s_count, s.s_key, s.s_parent, s.s_sib, s.s_nsib, s.q.x, s.q.y, s.q.z,
                        [&]() { return s.live ? a.r2f : 0.0f; }, visit, [](int, int) { return false; }, ol, oct, ob);
    if (!FILL) {
        total = pcr_octet_sum_i(total);
        if (s.inr && ol == 0) a.counts[s.i] = total;
        return;
    }
    if (!a.sort) return;
    const int c = total < room ? total : room;                // octet-uniform
    int32_t *const ri = a.idx + seg; double *const rd = a.d2 + seg;
    // between two steps of the network: the eight lanes of a row share a wavefront, hence an L1, so workgroup scope orders their stores and
    // loads (agent scope wrote back and invalidated the L2 at every step: 15 x the time of the whole search)
    auto fence = [&]() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); };
    fence();
    for (long long kk = 2; (kk >> 1) < c; kk <<= 1) {
        for (long long j = kk >> 1; j > 0; j >>= 1) {
            for (long long lo = ol; lo < c; lo += OCT) {
                const long long hi = (j == (kk >> 1)) ? (lo ^ (kk - 1)) : (lo ^ j);
                if (hi > lo && hi < c) {
                    const double dl = rd[lo], dh = rd[hi]; const int il = ri[lo], ih = ri[hi];
                    if (srch_lt((unsigned long long)__double_as_longlong(dh), ih, (unsigned long long)__double_as_longlong(dl), il)) { rd[lo] = dh; rd[hi] = dl; ri[lo] = ih; ri[hi] = il; }
                }
            }
            fence();
        }
    }
}

// rows of an index without points, and the caller index in the w of the index's points
__global__ void k_index_pad(int32_t *idx, double *d2, size_t total, double pad, int32_t *counts, int m) {
    const size_t i = (size_t)blockIdx.x * SRCH_BS + threadIdx.x;
    if (idx && i < total) { idx[i] = -1; d2[i] = pad; }
    if (counts && i < (size_t)m) counts[i] = 0;
}
__global__ void k_index_tag(float4 *pts, const uint32_t *perm, int n) {
    const int i = blockIdx.x * SRCH_BS + threadIdx.x;
    if (i < n) pts[i].w = __int_as_float((int)perm[i]);
}

// Morton keys of the queries on the index's lattice (clamped into it; a non-finite coordinate gives 0): the order in which the octets take them
struct QueryKeyArgs { const float *q; int m; float ox, oy, oz, s; uint64_t *keys; uint32_t *vals; };
__global__ void __launch_bounds__(SRCH_BS) k_query_keys(QueryKeyArgs a) {
    const int i = blockIdx.x * SRCH_BS + threadIdx.x;
    if (i >= a.m) return;
    const uint32_t ix = (uint32_t)fminf(fmaxf((a.q[(size_t)i * 3] - a.ox) * a.s, 0.0f), 65535.0f);
    const uint32_t iy = (uint32_t)fminf(fmaxf((a.q[(size_t)i * 3 + 1] - a.oy) * a.s, 0.0f), 65535.0f);
    const uint32_t iz = (uint32_t)fminf(fmaxf((a.q[(size_t)i * 3 + 2] - a.oz) * a.s, 0.0f), 65535.0f);
    a.keys[i] = pcr_morton3(ix, iy, iz);
    a.vals[i] = (uint32_t)i;
}

// ====================================================================================================== C ABI
// device bytes of an index over n points: what pcr_alloc_cloud takes for a cloud with a tree (every array rounded up to 256 B)
static size_t index_block_bytes(int64_t n) {
    const size_t cc = (size_t)(n > 0 ? n : 1), nodes = oct_node_capacity((int)cc);
    return cc * (sizeof(float4) + sizeof(uint64_t) + sizeof(int) + sizeof(int4) + sizeof(int2)) + nodes * (sizeof(int) + 2 * sizeof(float4) + sizeof(int4)) +
           sizeof(int) + sizeof(OctMeta) + 16 * 256;
}

extern "C" int pcr_index_create(pcr_context *ctx, const float *xyz, int64_t n, pcr_index **out) {
    return pcr_api_call(ctx, [&]() -> int {
    if (!out || n < 0 || n > SRCH_MAX_POINTS || (n > 0 && !xyz)) { ctx->err = "index_create: bad cloud or output pointer"; return PCR_EINVAL; }
    *out = nullptr;
    pcr_index *ix = new pcr_index();
    ix->device = ctx->device; ix->n = n;
    if (n == 0) { *out = ix; return PCR_OK; }
    auto build = [&]() -> int {
        PCR_TRY(pcr_arena_reserve(ctx, pcr_scratch_bytes_for(n) + (size_t)n * 64));
        double b6[6];
        PCR_TRY(pcr_dev_bounds(ctx, xyz, n, b6));
        ix->bytes = index_block_bytes(n);
        if (hipMalloc((void **)&ix->block, ix->bytes) != hipSuccess) { ix->block = nullptr; ctx->err = "hipMalloc(index)"; return PCR_ENOMEM; }
        {   // the cloud record's arrays come out of the index's block; everything else is scratch of the context's arena
            SideLane own(ctx, ix->block, ix->bytes, ctx->stream);
            PCR_TRY(pcr_alloc_cloud(ctx, &ix->c, (int)n, false, true));
        }
        uint32_t *perm = arena<uint32_t>(ctx, n);
        if (!perm) return PCR_ENOMEM;
        PCR_TRY(pcr_dev_sort_cloud(ctx, xyz, n, b6, &ix->c, perm));
        PCR_TRY(pcr_dev_build_bvh(ctx, &ix->c));
        PCR_LAUNCH(ctx, k_index_tag, dim3((unsigned)((n + SRCH_BS - 1) / SRCH_BS)), dim3(SRCH_BS), 0, ctx->stream, ix->c.pts, (const uint32_t *)perm, (int)n);
        // finished before the call returns: the caller may overwrite xyz, and any context may search the index
        PCR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        return PCR_OK;
    };
    const int rc = build();
    if (rc != PCR_OK) { if (ix->block) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(ix->block); } delete ix; return rc; }
    *out = ix;
    return PCR_OK;
    });
}

extern "C" int pcr_index_destroy(pcr_index *index) {
    if (!index) return PCR_OK;
    if (index->block) {
        if (hipSetDevice(index->device) != hipSuccess) return PCR_EHIP;
        (void)hipFree(index->block);                          // waits for the device: no search is still reading the block
    }
    delete index;
    return PCR_OK;
}

// what a unit that walks an index with a kernel of its own needs of it (pcr_multiway.hip): the sorted cloud and the device it lives on
const DevCloud *pcr_index_cloud(const pcr_index *index, int *device, int64_t *n) {
    if (device) *device = index->device;
    if (n) *n = index->n;
    return &index->c;
}

static int search_check(pcr_context *ctx, const pcr_index *index, const float *q, int64_t m, const char *what) {
    if (!index || m < 0 || m > SRCH_MAX_POINTS || (m > 0 && !q)) { ctx->err = std::string(what) + ": bad index, query pointer or query count"; return PCR_EINVAL; }
    if (index->device != ctx->device) { ctx->err = std::string(what) + ": the index lives on another device than the context"; return PCR_EINVAL; }
    return PCR_OK;
}
static SearchArgs search_args(const pcr_index *index, const float *q, int64_t m) {
    SearchArgs a; std::memset(&a, 0, sizeof a);
    a.t = oct_view(&index->c); a.q = q; a.m = (int)m;
    return a;
}
// The order of the queries.  A wavefront serves 8 queries, and its 8 walks run in lockstep: queries that lie far apart make every
// walk as long as the longest and share no cache lines.  Taking them in the Morton order of their keys on the index's lattice (one radix
// sort in the context's arena; every row is still written to its caller position) shortens the kernel, and the sort costs more than a third
// of a k = 1 search of the same queries: it pays for large batches of the searches with long walks only, from `sort_min` queries on
// (0: never; DESIGN.md 4.13 has the measurements).  The option "search_sort_queries" forces one form (0 / 1): the same bits either way.
// *qperm = nullptr: caller order.
static int search_order(pcr_context *ctx, const pcr_index *index, const float *q, int64_t m, int64_t sort_min, const uint32_t **qperm) {
    *qperm = nullptr;
    const int forced = pcr_options().search_sort_queries.load(std::memory_order_relaxed);
    if (forced >= 0 ? forced == 0 : (sort_min <= 0 || m < sort_min)) return PCR_OK;
    if (m < 2 || index->n == 0) return PCR_OK;
    const size_t tb = pcr_sort_temp_bytes((size_t)m);
    PCR_TRY(pcr_arena_reserve(ctx, (size_t)m * 24 + tb + (1u << 16)));
    uint64_t *k0 = arena<uint64_t>(ctx, m), *k1 = arena<uint64_t>(ctx, m);
    uint32_t *v0 = arena<uint32_t>(ctx, m), *v1 = arena<uint32_t>(ctx, m);
    void *temp = pcr_arena_alloc(ctx, tb);
    if (!k0 || !k1 || !v0 || !v1 || !temp) return PCR_ENOMEM;
    QueryKeyArgs a; a.q = q; a.m = (int)m; a.ox = index->c.key_org[0]; a.oy = index->c.key_org[1]; a.oz = index->c.key_org[2];
    a.s = index->c.key_unit[0] > 0.0f ? 1.0f / index->c.key_unit[0] : 0.0f; a.keys = k0; a.vals = v0;
    PCR_LAUNCH(ctx, k_query_keys, dim3((unsigned)((m + SRCH_BS - 1) / SRCH_BS)), dim3(SRCH_BS), 0, ctx->stream, a);
    PCR_TRY(pcr_sort_pairs(ctx, temp, tb, k0, k1, v0, v1, (size_t)m, 48));
    *qperm = v1;
    return PCR_OK;
}
// queries from which a k-best search sorts them: never up to k = 8, from 131072 up to k = 64, from 32768 beyond (the 25-slot kernel)
static int64_t knn_sort_min(int k) { return k <= 8 ? 0 : (k <= 64 ? 131072 : 32768); }
static dim3 search_grid(int64_t m) { return dim3((unsigned)(((size_t)m * OCT + SRCH_BS - 1) / SRCH_BS)); }
static int search_pad(pcr_context *ctx, int32_t *idx, double *d2, size_t total, double pad, int32_t *counts, int64_t m) {
    const size_t work = total > (size_t)m ? total : (size_t)m;
    if (work == 0) return PCR_OK;
    PCR_LAUNCH(ctx, k_index_pad, dim3((unsigned)((work + SRCH_BS - 1) / SRCH_BS)), dim3(SRCH_BS), 0, ctx->stream, idx, d2, total, pad, counts, (int)m);
    return PCR_OK;
}
// the k-best kernel with the register slots per lane that k asks for
template <bool HYBRID>
static int launch_index_knn(pcr_context *ctx, const SearchArgs &a) {
    const dim3 grid = search_grid(a.m);
    if (a.k == 1) PCR_LAUNCH(ctx, (k_index_knn<1, HYBRID, true>), grid, dim3(SRCH_BS), 0, ctx->stream, a);
    else if (a.k <= 8) PCR_LAUNCH(ctx, (k_index_knn<1, HYBRID, false>), grid, dim3(SRCH_BS), 0, ctx->stream, a);
    else if (a.k <= 32) PCR_LAUNCH(ctx, (k_index_knn<4, HYBRID, false>), grid, dim3(SRCH_BS), 0, ctx->stream, a);
    else if (a.k <= 64) PCR_LAUNCH(ctx, (k_index_knn<8, HYBRID, false>), grid, dim3(SRCH_BS), 0, ctx->stream, a);
    else PCR_LAUNCH(ctx, (k_index_knn<25, HYBRID, false>), grid, dim3(SRCH_BS), 0, ctx->stream, a);
    return PCR_OK;
}

int pcr_dev_tagged_knn(pcr_context *ctx, const DevCloud *c, const float *query_xyz, int64_t m, const uint32_t *qperm, int k, int32_t *idx, double *d2) {
    if (k < 1 || k > SRCH_MAX_K || m < 1 || m > SRCH_MAX_POINTS) { ctx->err = "tagged_knn: k or query count out of range"; return PCR_EINVAL; }
    SearchArgs a; std::memset(&a, 0, sizeof a);
    a.t = oct_view(c); a.q = query_xyz; a.m = (int)m; a.qperm = qperm; a.k = k; a.idx = idx; a.d2 = d2;
    return launch_index_knn<false>(ctx, a);
}

int pcr_dev_tagged_hybrid(pcr_context *ctx, const DevCloud *c, const float *query_xyz, int64_t m, const uint32_t *qperm, double radius, int max_nn, int32_t *idx, double *d2,
                          int32_t *counts) {
    if (max_nn < 1 || max_nn > SRCH_MAX_K || !(radius > 0.0) || m < 1 || m > SRCH_MAX_POINTS) { ctx->err = "tagged_hybrid: max_nn, radius or query count out of range"; return PCR_EINVAL; }
    SearchArgs a; std::memset(&a, 0, sizeof a);
    a.t = oct_view(c); a.q = query_xyz; a.m = (int)m; a.qperm = qperm; a.k = max_nn; a.r2 = radius * radius; a.r2f = pcr_wide_r2f(a.r2);
    a.idx = idx; a.d2 = d2; a.counts = counts;
    return launch_index_knn<true>(ctx, a);
}

extern "C" int pcr_index_knn(pcr_context *ctx, const pcr_index *index, const float *query_xyz, int64_t m, int k, int32_t *idx, double *d2) {
    return pcr_api_call(ctx, [&]() -> int {
    PCR_TRY(search_check(ctx, index, query_xyz, m, "index_knn"));
    if (k < 1 || k > SRCH_MAX_K) { ctx->err = "index_knn: k outside 1..200"; return PCR_EINVAL; }
    if (m > 0 && (!idx || !d2)) { ctx->err = "index_knn: null output"; return PCR_EINVAL; }
    if (m == 0) return PCR_OK;
    if (index->n == 0) return search_pad(ctx, idx, d2, (size_t)m * k, (double)__builtin_inff(), nullptr, m);
    SearchArgs a = search_args(index, query_xyz, m);
    a.k = k; a.idx = idx; a.d2 = d2;
    PCR_TRY(search_order(ctx, index, query_xyz, m, knn_sort_min(k), &a.qperm));
    return launch_index_knn<false>(ctx, a);
    });
}

extern "C" int pcr_index_hybrid(pcr_context *ctx, const pcr_index *index, const float *query_xyz, int64_t m, double radius, int max_nn, int32_t *idx, double *d2,
                                int32_t *counts) {
    return pcr_api_call(ctx, [&]() -> int {
    PCR_TRY(search_check(ctx, index, query_xyz, m, "index_hybrid"));
    if (max_nn < 1 || max_nn > SRCH_MAX_K || !(radius > 0.0)) { ctx->err = "index_hybrid: max_nn outside 1..200 or radius <= 0"; return PCR_EINVAL; }
    if (m > 0 && (!idx || !d2 || !counts)) { ctx->err = "index_hybrid: null output"; return PCR_EINVAL; }
    if (m == 0) return PCR_OK;
    if (index->n == 0) return search_pad(ctx, idx, d2, (size_t)m * max_nn, 0.0, counts, m);
    SearchArgs a = search_args(index, query_xyz, m);
    a.k = max_nn; a.r2 = radius * radius; a.r2f = pcr_wide_r2f(a.r2); a.idx = idx; a.d2 = d2; a.counts = counts;
    PCR_TRY(search_order(ctx, index, query_xyz, m, knn_sort_min(max_nn), &a.qperm));
    return launch_index_knn<true>(ctx, a);
    });
}

extern "C" int pcr_index_radius_count(pcr_context *ctx, const pcr_index *index, const float *query_xyz, int64_t m, double radius, int32_t *counts) {
    return pcr_api_call(ctx, [&]() -> int {
    PCR_TRY(search_check(ctx, index, query_xyz, m, "index_radius_count"));
    if (!(radius > 0.0)) { ctx->err = "index_radius_count: radius <= 0"; return PCR_EINVAL; }
    if (m > 0 && !counts) { ctx->err = "index_radius_count: null output"; return PCR_EINVAL; }
    if (m == 0) return PCR_OK;
    if (index->n == 0) return search_pad(ctx, nullptr, nullptr, 0, 0.0, counts, m);
    SearchArgs a = search_args(index, query_xyz, m);
    a.r2 = radius * radius; a.r2f = pcr_wide_r2f(a.r2); a.counts = counts;
    PCR_TRY(search_order(ctx, index, query_xyz, m, 0, &a.qperm));
    PCR_LAUNCH(ctx, k_index_radius<false>, search_grid(m), dim3(SRCH_BS), 0, ctx->stream, a);
    return PCR_OK;
    });
}

extern "C" int pcr_index_radius_fill(pcr_context *ctx, const pcr_index *index, const float *query_xyz, int64_t m, double radius, const int64_t *row_splits, int32_t *idx,
                                     double *d2, int sort) {
    return pcr_api_call(ctx, [&]() -> int {
    PCR_TRY(search_check(ctx, index, query_xyz, m, "index_radius_fill"));
    if (!(radius > 0.0)) { ctx->err = "index_radius_fill: radius <= 0"; return PCR_EINVAL; }
    if (m > 0 && !row_splits) { ctx->err = "index_radius_fill: null row_splits"; return PCR_EINVAL; }
    if (m == 0 || index->n == 0 || !idx || !d2) return PCR_OK;       // (no members anywhere: nothing to write)
    SearchArgs a = search_args(index, query_xyz, m);
    a.r2 = radius * radius; a.r2f = pcr_wide_r2f(a.r2); a.idx = idx; a.d2 = d2; a.splits = row_splits; a.sort = sort;
    PCR_TRY(search_order(ctx, index, query_xyz, m, 0, &a.qperm));
    PCR_LAUNCH(ctx, k_index_radius<true>, search_grid(m), dim3(SRCH_BS), 0, ctx->stream, a);
    return PCR_OK;
    });
}
