// HNSW graph index (faiss IndexHNSWFlat as eval/utils/get_index_faiss.py:88-96 builds it: M = 16, efConstruction = 80,
// efSearch = 16, search_bounded_queue), gfx950.  Opt-in from eval/eval_faiss.py (NAFP_HNSW=1 next to NAFP_APPROX_INDEX=1);
// the host side is eval/hnsw.py, the contract is in include/nafp.h "HNSW" and restated in float64 by tests/_hnsw_ref.py.
//
// The build is round based: the rows of a round search the graph as it stood when the round began (hnsw_layer_search_kernel),
// choose their own lists (hnsw_select_forward_kernel), and only then are added to the lists of the rows they chose
// (hnsw_rev_*).  Nothing waits on another workgroup, every loop has a static bound, and every result is a function of SETS
// (the pool of a search, the union a reverse list is chosen from), never of an arrival order: atomics only count.
//
// ONE WAVE PER QUERY / ROW / TARGET (64-thread workgroups, so __syncthreads is the wave's own barrier):
//   hnsw_layer_search_kernel<D>   the bounded-pool search of one level.  The pool (<= 128 keys of 8 bytes: distance bits,
//                                 id, expanded flag; 1 KB of LDS) stays sorted.  Per expansion: the <= 32 neighbours are
//                                 de-duplicated against the pool (64 lanes = 32 neighbours x 2 pool halves), their fp32
//                                 distances computed 4 at a time by 16-lane groups (a row is 1 / 2 / 4 float4 per lane, the
//                                 query stays in registers), and merged by rank: a new key lands at (keys below it in the pool:
//                                 binary search) + (new keys below it: counted), a pool key moves up by the new keys below it.
//                                 There is no visited filter: exactness rests on the pool (a key that lost once can never
//                                 win later), and re-evaluating a neighbour costs one L2-resident row.
//   hnsw_select_forward_kernel<D> the shrink heuristic over a search's result: candidates in order, each tested against the
//                                 accepted ones 4 at a time (same groups), first rejection ends the test
//   hnsw_rev_count / offsets / scatter_kernel   per chosen old row the new rows that chose it: integer counts, a scan over the
//                                 touched rows only, a scatter whose order inside a row is arbitrary ...
//   hnsw_rev_apply_kernel<D>      ... because the wave of a touched row walks its union in (distance, id) order by repeated
//                                 minimum extraction (keys in the workspace; the old list in registers) and selects from it
#include "nafp_common.h"

#include <algorithm>

namespace nafp {

typedef unsigned long long hnsw_key;
constexpr int HNSW_M = 16;
constexpr int HNSW_MAX_EF = 128;
constexpr int HNSW_MAX_K = 32;
constexpr int HNSW_MAX_LEVEL = 7;
constexpr hnsw_key HNSW_EMPTY = ~0ull;

// pool key: distance bits (non-negative floats order as integers) | id << 1 | expanded
__device__ __forceinline__ hnsw_key hk_make(float dist, int id) { return ((hnsw_key)__float_as_uint(dist) << 32) | ((hnsw_key)(unsigned)id << 1); }
__device__ __forceinline__ int hk_id(hnsw_key k) { return (int)((unsigned)(k & 0xffffffffull) >> 1); }
__device__ __forceinline__ float hk_dist(hnsw_key k) { return __uint_as_float((unsigned)(k >> 32)); }
// key of the reverse pass: distance bits | id
__device__ __forceinline__ hnsw_key rk_make(float dist, int id) { return ((hnsw_key)__float_as_uint(dist) << 32) | (hnsw_key)(unsigned)id; }
__device__ __forceinline__ int rk_id(hnsw_key k) { return (int)(unsigned)(k & 0xffffffffull); }

__device__ __forceinline__ hnsw_key shfl_key(hnsw_key v, int src) {
    const unsigned lo = __shfl((unsigned)(v & 0xffffffffull), src, 64), hi = __shfl((unsigned)(v >> 32), src, 64);
    return ((hnsw_key)hi << 32) | lo;
}
__device__ __forceinline__ hnsw_key wave_min_key(hnsw_key v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)(v & 0xffffffffull), o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
        const hnsw_key w = ((hnsw_key)hi << 32) | lo;
        v = w < v ? w : v;
    }
    return v;
}

// A row as the 16 lanes of a group hold it: float4 number t * 16 + sub, t < D / 64.
template <int D>
__device__ __forceinline__ void hnsw_load(const float* __restrict__ row, int sub, float4 (&v)[D / 64]) {
#pragma unroll
    for (int t = 0; t < D / 64; ++t) v[t] = reinterpret_cast<const float4*>(row)[t * 16 + sub];
}
// this lane's share of |a - row|^2 (fixed order); hnsw_sum16 completes it over the group, the same bits in its 16 lanes
template <int D>
__device__ __forceinline__ float hnsw_partial(const float4 (&a)[D / 64], const float* __restrict__ row, int sub) {
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < D / 64; ++t) {
        const float4 b = reinterpret_cast<const float4*>(row)[t * 16 + sub];
        const float dx = a[t].x - b.x, dy = a[t].y - b.y, dz = a[t].z - b.z, dw = a[t].w - b.w;
        acc = fmaf(dx, dx, acc); acc = fmaf(dy, dy, acc); acc = fmaf(dz, dz, acc); acc = fmaf(dw, dw, acc);
    }
    return acc;
}
__device__ __forceinline__ float hnsw_sum16(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The lists of one level: row r's list is links[(slot ? slot[r] : r) * stride .. + deg), -1 padded.
struct HnswLevel {
    const int* links; const int* slot; long long n_link_rows, stride; int deg;
    __device__ __forceinline__ long long list_of(int row) const {
        const long long r = slot ? (long long)slot[row] : (long long)row;
        return (r >= 0 && r < n_link_rows) ? r * stride : -1;
    }
};

// distances of the ids lanes 0 .. 31 hold (mask: which of them) to the row `a`, 4 per round; lane j < 32 gets its own
template <int D>
__device__ __forceinline__ float hnsw_dist32(const float* __restrict__ x, const float4 (&a)[D / 64], int id_of_lane, unsigned long long mask, int lane) {
    const int sub = lane & 15, grp = lane >> 4;
    float mine = 0.f;
    for (int r4 = 0; r4 < 8; ++r4) {
        if (!((mask >> (4 * r4)) & 0xFull)) continue;                       // wave-uniform
        const int j = 4 * r4 + grp;
        const int id = __shfl(id_of_lane, j, 64);
        float part = 0.f;
        if ((mask >> j) & 1ull) part = hnsw_partial<D>(a, x + (long long)id * D, sub);
        part = hnsw_sum16(part);
        const float v = __shfl(part, (lane & 3) * 16, 64);
        if ((lane >> 2) == r4) mine = v;
    }
    return mine;
}

struct HnswSearchParams {
    const float* x; long long n_rows;
    HnswLevel lv;
    const float* q; const int* entries; const int* qlevels; int level;
    int ef, max_exp, n_out; float* out_dist; int* out_ids;
};

template <int D>
__global__ __launch_bounds__(64) void hnsw_layer_search_kernel(const HnswSearchParams p) {
    __shared__ hnsw_key pool[HNSW_MAX_EF];
    const int lane = threadIdx.x, sub = lane & 15;
    const long long qi = blockIdx.x;
    const int ef = (p.qlevels && p.qlevels[qi] < p.level) ? 1 : p.ef;       // a row above its own levels only descends
    float4 qv[D / 64];
    hnsw_load<D>(p.q + qi * D, sub, qv);
    const int entry = p.entries[qi];
    int size = 0;
    hnsw_key first = HNSW_EMPTY;
    if (entry >= 0 && entry < p.n_rows) {
        first = hk_make(hnsw_sum16(hnsw_partial<D>(qv, p.x + (long long)entry * D, sub)), entry);
        size = 1;
    }
    pool[lane] = lane == 0 ? first : HNSW_EMPTY;
    pool[lane + 64] = HNSW_EMPTY;
    for (int it = 0; it < p.max_exp; ++it) {
        __syncthreads();
        hnsw_key k0 = lane < size ? pool[lane] : HNSW_EMPTY;
        hnsw_key k1 = lane + 64 < size ? pool[lane + 64] : HNSW_EMPTY;
        const unsigned long long m0 = __ballot(k0 != HNSW_EMPTY && !(k0 & 1ull)), m1 = __ballot(k1 != HNSW_EMPTY && !(k1 & 1ull));
        if (!(m0 | m1)) break;                                              // nothing left to expand
        const int idx = m0 ? __ffsll((long long)m0) - 1 : 64 + __ffsll((long long)m1) - 1;
        const int c = hk_id(shfl_key(idx < 64 ? k0 : k1, idx & 63));
        if (lane == (idx & 63)) {
            if (idx < 64) { k0 |= 1ull; pool[idx] = k0; } else { k1 |= 1ull; pool[idx] = k1; }
        }
        const long long base = p.lv.list_of(c);
        int nb = -1;
        if (lane < p.lv.deg && base >= 0) nb = p.lv.links[base + lane];
        if (nb < 0 || nb >= p.n_rows) nb = -1;
        for (int i = 0; i < 31; ++i) {                                      // a list holds no row twice; an uploaded one might
            const int o = __shfl(nb, i, 64);
            if (i < lane && o == nb) nb = -1;
        }
        const int nbm = __shfl(nb, lane & 31, 64);
        int dup = 0;
        for (int pi = lane >> 5; pi < size; pi += 2) dup |= hk_id(pool[pi]) == nbm;
        dup |= __shfl_xor(dup, 32, 64);
        const bool need = lane < 32 && nb >= 0 && !dup;
        const unsigned long long needmask = __ballot(need);
        if (!needmask) continue;
        const float mydist = hnsw_dist32<D>(p.x, qv, nb, needmask, lane);
        const hnsw_key key = need ? hk_make(mydist, nb) : HNSW_EMPTY;
        int cn = 0, c0 = 0, c1 = 0;
        for (int i = 0; i < 32; ++i) {
            if (!((needmask >> i) & 1ull)) continue;                        // wave-uniform
            const hnsw_key ki = shfl_key(key, i);
            cn += ki < key; c0 += ki < k0; c1 += ki < k1;
        }
        int lo = 0, hi = size;
        for (int s = 0; s < 8; ++s) {                                       // lower bound among <= 128 keys
            if (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (pool[mid] < key) lo = mid + 1; else hi = mid;
            }
        }
        __syncthreads();
        if (lane < size && lane + c0 < ef) pool[lane + c0] = k0;
        if (lane + 64 < size && lane + 64 + c1 < ef) pool[lane + 64 + c1] = k1;
        if (key != HNSW_EMPTY && lo + cn < ef) pool[lo + cn] = key;
        size = min(ef, size + __popcll(needmask));
    }
    __syncthreads();
    for (int i = lane; i < p.n_out; i += 64) {
        const bool has = i < size;
        const hnsw_key k = has ? pool[i] : 0ull;
        p.out_ids[qi * p.n_out + i] = has ? hk_id(k) : -1;
        p.out_dist[qi * p.n_out + i] = has ? hk_dist(k) : __builtin_inff();
    }
}

// candidate c (its distance to the owner: dco) against the accepted rows (lane a < n_acc holds accepted[a]): true unless one of
// them is nearer to c than the owner is
template <int D>
__device__ __forceinline__ bool hnsw_accept(const float* __restrict__ x, int c, float dco, int acc_id, int n_acc, int lane) {
    const int sub = lane & 15, grp = lane >> 4;
    float4 cv[D / 64];
    hnsw_load<D>(x + (long long)c * D, sub, cv);
    for (int r4 = 0; r4 < 8 && 4 * r4 < n_acc; ++r4) {
        const int j = 4 * r4 + grp;
        const int a = __shfl(acc_id, j, 64);
        float part = 0.f;
        if (j < n_acc) part = hnsw_partial<D>(cv, x + (long long)a * D, sub);
        part = hnsw_sum16(part);
        if (__ballot(j < n_acc && part < dco)) return false;
    }
    return true;
}

struct HnswSelectParams {
    const float* x; long long n_rows;
    int* links; const int* slot; long long n_link_rows, stride; int deg;
    long long row0; const int* new_levels; int level;
    const float* cand_dist; const int* cand_ids; int ef;
};

template <int D>
__global__ __launch_bounds__(64) void hnsw_select_forward_kernel(const HnswSelectParams p) {
    const int lane = threadIdx.x;
    const long long i = blockIdx.x, row = p.row0 + i;
    if (p.new_levels[i] < p.level) return;
    const long long r = p.slot ? (long long)p.slot[row] : row;
    if (r < 0 || r >= p.n_link_rows) return;
    const float* cd = p.cand_dist + i * p.ef;
    const int* ci = p.cand_ids + i * p.ef;
    int acc_id = -1, n_acc = 0, prev = -1;
    for (int t = 0; t < p.ef && n_acc < p.deg; ++t) {
        const int c = ci[t];
        if (c < 0 || c >= p.n_rows) break;                                  // -1: the end of the candidates
        if (c == row || c == prev) continue;                                // (in order, a duplicate follows its twin)
        prev = c;
        if (hnsw_accept<D>(p.x, c, cd[t], acc_id, n_acc, lane)) {
            if (lane == n_acc) acc_id = c;
            ++n_acc;
        }
    }
    if (lane < p.deg) p.links[r * p.stride + lane] = lane < n_acc ? acc_id : -1;
}

// ---- reverse links ---------------------------------------------------------------------------------------------------------
struct HnswRevParams {
    const float* x; long long n_rows;
    int* links; const int* slot; long long n_link_rows, stride; int deg;
    long long row0, n_new; const int* new_levels; int level;
    int* n_touched; int* cnt; int* fill; int* tslot; int* touched; int* off; int* inc; hnsw_key* keys;
};

// the (new row, target) edge of thread e, or -1
__device__ __forceinline__ int hnsw_rev_edge(const HnswRevParams& p, long long e, long long* src) {
    const long long i = e / p.deg;
    if (i >= p.n_new || p.new_levels[i] < p.level) return -1;
    const long long row = p.row0 + i, r = p.slot ? (long long)p.slot[row] : row;
    if (r < 0 || r >= p.n_link_rows) return -1;
    const int j = p.links[r * p.stride + (int)(e % p.deg)];
    *src = row;
    return (j >= 0 && j < p.row0) ? j : -1;                                 // targets are rows of the frozen graph
}

__global__ __launch_bounds__(256) void hnsw_rev_count_kernel(const HnswRevParams p) {
    long long src;
    const int j = hnsw_rev_edge(p, (long long)blockIdx.x * 256 + threadIdx.x, &src);
    if (j < 0) return;
    if (atomicAdd(&p.cnt[j], 1) == 0) {                                     // integer counts: their totals are order-free
        const int t = atomicAdd(p.n_touched, 1);                            // (the order of `touched` is arbitrary: rows are independent)
        p.touched[t] = j;
        p.tslot[j] = t;
    }
}

__global__ __launch_bounds__(1024) void hnsw_rev_offsets_kernel(const HnswRevParams p) {
    __shared__ int part[1024];
    const int tid = threadIdx.x, nt = *p.n_touched;
    const int chunk = (nt + 1023) / 1024, t0 = min(nt, tid * chunk), t1 = min(nt, t0 + chunk);
    int s = 0;
    for (int t = t0; t < t1; ++t) s += p.cnt[p.touched[t]];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 1024; ++i) { const int v = part[i]; part[i] = run; run += v; }
    }
    __syncthreads();
    int run = part[tid];
    for (int t = t0; t < t1; ++t) { p.off[t] = run; run += p.cnt[p.touched[t]]; }
}

__global__ __launch_bounds__(256) void hnsw_rev_scatter_kernel(const HnswRevParams p) {
    long long src;
    const int j = hnsw_rev_edge(p, (long long)blockIdx.x * 256 + threadIdx.x, &src);
    if (j < 0) return;
    const int t = p.tslot[j];
    p.inc[p.off[t] + atomicAdd(&p.fill[t], 1)] = (int)src;                  // any order: the target's wave walks them by key
}

template <int D>
__global__ __launch_bounds__(64) void hnsw_rev_apply_kernel(const HnswRevParams p) {
    const int lane = threadIdx.x, sub = lane & 15, grp = lane >> 4;
    const int nt = *p.n_touched;
    for (int t = blockIdx.x; t < nt; t += gridDim.x) {
        const int j = p.touched[t], c = p.cnt[j], o = p.off[t];
        const long long r = p.slot ? (long long)p.slot[j] : (long long)j;
        if (r < 0 || r >= p.n_link_rows) continue;
        int* lst = p.links + r * p.stride;
        float4 ov[D / 64];
        hnsw_load<D>(p.x + (long long)j * D, sub, ov);
        int old = lane < p.deg ? lst[lane] : -1;
        if (old < 0 || old >= p.n_rows || old == j) old = -1;
        const unsigned long long oldmask = __ballot(old >= 0);
        const float od = hnsw_dist32<D>(p.x, ov, old, oldmask, lane);
        const hnsw_key okey = old >= 0 ? rk_make(od, old) : HNSW_EMPTY;
        for (int p0 = 0; p0 < c; p0 += 4) {                                 // the incoming rows' keys, 4 per round
            const int pp = p0 + grp;
            const int id = pp < c ? p.inc[o + pp] : -1;
            float part = 0.f;
            if (id >= 0) part = hnsw_partial<D>(ov, p.x + (long long)id * D, sub);
            part = hnsw_sum16(part);
            if (id >= 0 && sub == 0) p.keys[o + pp] = rk_make(part, id);
        }
        __syncthreads();                                                    // the keys are read across lanes
        const int n_u = __popcll(oldmask) + c;
        const bool prune = n_u > p.deg;
        int acc_id = -1, n_acc = 0;
        hnsw_key last = 0ull;
        bool have = false;
        for (int step = 0; step < n_u && n_acc < p.deg; ++step) {           // the union in (distance, id) order
            hnsw_key best = (okey != HNSW_EMPTY && (!have || okey > last)) ? okey : HNSW_EMPTY;
            for (int pp = lane; pp < c; pp += 64) {
                const hnsw_key k = p.keys[o + pp];
                if ((!have || k > last) && k < best) best = k;
            }
            best = wave_min_key(best);
            if (best == HNSW_EMPTY) break;
            last = best; have = true;
            const int cid = rk_id(best);
            if (cid == j) continue;
            if (!prune || hnsw_accept<D>(p.x, cid, __uint_as_float((unsigned)(best >> 32)), acc_id, n_acc, lane)) {
                if (lane == n_acc) acc_id = cid;
                ++n_acc;
            }
        }
        if (lane < p.deg) lst[lane] = lane < n_acc ? acc_id : -1;
    }
}

__global__ __launch_bounds__(256) void hnsw_fill_kernel(int* __restrict__ out, long long n, int v) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = v;
}

static bool hnsw_dim_ok(int d) { return d == 64 || d == 128 || d == 256; }
// NAFP_OK, or why not: the limits every HNSW entry point shares (before any GPU call)
static int hnsw_limits(int dim, int M, int level, int ef, int k) {
    if (dim <= 0 || M <= 0 || level < 0 || ef < 1 || k < 1) return NAFP_ERR_INVALID_ARG;
    if (!hnsw_dim_ok(dim) || M != HNSW_M || level > HNSW_MAX_LEVEL || ef > HNSW_MAX_EF || k > HNSW_MAX_K) return NAFP_ERR_UNSUPPORTED;
    return NAFP_OK;
}

struct HnswRevLayout { int64_t clear_bytes, tslot, touched, off, inc, keys, total; };
static HnswRevLayout hnsw_rev_layout(int64_t n_old, int64_t edges) {
    HnswRevLayout l;
    int64_t at = 16;                                  // n_touched
    at += n_old * 4;                                  // cnt
    at += edges * 4;                                  // fill
    l.clear_bytes = at;
    l.tslot = at; at += n_old * 4;
    l.touched = at; at += edges * 4;
    l.off = at; at += edges * 4;
    l.inc = at; at += edges * 4;
    at = (at + 15) / 16 * 16;
    l.keys = at; at += edges * 8;
    l.total = at;
    return l;
}

static int hnsw_search_layer_launch(int dim, const HnswSearchParams& p, int64_t nq, hipStream_t st) {
    if (nq == 0) return NAFP_OK;
    const dim3 grid((unsigned)nq), block(64);
    if (dim == 64) hipLaunchKernelGGL(hnsw_layer_search_kernel<64>, grid, block, 0, st, p);
    else if (dim == 128) hipLaunchKernelGGL(hnsw_layer_search_kernel<128>, grid, block, 0, st, p);
    else hipLaunchKernelGGL(hnsw_layer_search_kernel<256>, grid, block, 0, st, p);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

}  // namespace nafp

using namespace nafp;

extern "C" {

int nafp_hnsw_default_max_expansions(int ef) { return ef < 1 || ef > HNSW_MAX_EF ? -1 : 4 * ef + 256; }

int64_t nafp_hnsw_reverse_workspace_bytes(int64_t n_old, int64_t n_new, int M, int level) {
    if (n_old < 0 || n_new < 0 || M != HNSW_M || level < 0 || level > HNSW_MAX_LEVEL) return -1;
    if (n_old > 0x7fffffffll || n_new > (1ll << 24)) return -1;
    return hnsw_rev_layout(n_old, n_new * (level == 0 ? 2 * M : M)).total;
}

int64_t nafp_hnsw_search_workspace_bytes(int64_t n_query, int ef_search, int k) {
    if (n_query < 0 || ef_search < 1 || ef_search > HNSW_MAX_EF || k < 1 || k > HNSW_MAX_K) return -1;
    return 2 * n_query * 4 + 16;
}

int nafp_hnsw_search_layer(const float* x, int64_t n_rows, int dim, const int32_t* links, const int32_t* slot,
                           int64_t n_link_rows, int64_t link_stride, int M, int level, const float* query, int64_t n_query,
                           const int32_t* entries, const int32_t* query_levels, int ef, int max_expansions, int n_out,
                           float* out_dist, int32_t* out_ids, void* stream) {
    if (!x || !links || !query || !entries || !out_dist || !out_ids || n_rows < 0 || n_query < 0 || n_link_rows < 0 || link_stride < 0 ||
        max_expansions < 0 || n_out < 0)
        return NAFP_ERR_INVALID_ARG;
    const int rc = hnsw_limits(dim, M, level, ef, 1);
    if (rc != NAFP_OK) return rc;
    const int deg = level == 0 ? 2 * M : M;
    if (n_out > ef || link_stride < deg) return NAFP_ERR_INVALID_ARG;
    if (n_rows > 0x7fffffffll || n_query > 0x7fffffffll) return NAFP_ERR_UNSUPPORTED;
    // a block writes its results when it ends, while others may not have read their entry yet: the two must not share memory
    const char *e0 = (const char*)entries, *e1 = e0 + n_query * 4;
    const char *i0 = (const char*)out_ids, *d0 = (const char*)out_dist;
    const int64_t out_bytes = n_query * n_out * 4;
    if ((e0 < i0 + out_bytes && i0 < e1) || (e0 < d0 + out_bytes && d0 < e1)) return NAFP_ERR_INVALID_ARG;
    HnswSearchParams p{x, n_rows, {links, slot, n_link_rows, link_stride, deg}, query, entries, query_levels, level, ef, max_expansions,
                       n_out, out_dist, out_ids};
    return hnsw_search_layer_launch(dim, p, n_query, (hipStream_t)stream);
}

int nafp_hnsw_select_forward(const float* x, int64_t n_rows, int dim, int64_t row0, int64_t n_new, const int32_t* new_levels,
                             int level, int M, const float* cand_dist, const int32_t* cand_ids, int ef, int32_t* links,
                             const int32_t* slot, int64_t n_link_rows, int64_t link_stride, void* stream) {
    if (!x || !new_levels || !cand_dist || !cand_ids || !links || n_rows < 0 || row0 < 0 || n_new < 0 || n_link_rows < 0 || link_stride < 0)
        return NAFP_ERR_INVALID_ARG;
    const int rc = hnsw_limits(dim, M, level, ef, 1);
    if (rc != NAFP_OK) return rc;
    const int deg = level == 0 ? 2 * M : M;
    if (link_stride < deg || row0 + n_new > n_rows) return NAFP_ERR_INVALID_ARG;
    if (n_rows > 0x7fffffffll) return NAFP_ERR_UNSUPPORTED;
    if (n_new == 0) return NAFP_OK;
    HnswSelectParams p{x, n_rows, links, slot, n_link_rows, link_stride, deg, row0, new_levels, level, cand_dist, cand_ids, ef};
    const dim3 grid((unsigned)n_new), block(64);
    hipStream_t st = (hipStream_t)stream;
    if (dim == 64) hipLaunchKernelGGL(hnsw_select_forward_kernel<64>, grid, block, 0, st, p);
    else if (dim == 128) hipLaunchKernelGGL(hnsw_select_forward_kernel<128>, grid, block, 0, st, p);
    else hipLaunchKernelGGL(hnsw_select_forward_kernel<256>, grid, block, 0, st, p);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

int nafp_hnsw_reverse_links(const float* x, int64_t n_rows, int dim, int64_t row0, int64_t n_new, const int32_t* new_levels,
                            int level, int M, int32_t* links, const int32_t* slot, int64_t n_link_rows, int64_t link_stride,
                            void* workspace, int64_t workspace_bytes, void* stream) {
    if (!x || !new_levels || !links || n_rows < 0 || row0 < 0 || n_new < 0 || n_link_rows < 0 || link_stride < 0 || workspace_bytes < 0)
        return NAFP_ERR_INVALID_ARG;
    const int rc = hnsw_limits(dim, M, level, 1, 1);
    if (rc != NAFP_OK) return rc;
    const int deg = level == 0 ? 2 * M : M;
    if (link_stride < deg || row0 + n_new > n_rows) return NAFP_ERR_INVALID_ARG;
    const int64_t need = nafp_hnsw_reverse_workspace_bytes(row0, n_new, M, level);
    if (need < 0 || n_rows > 0x7fffffffll) return NAFP_ERR_UNSUPPORTED;
    if (n_new == 0 || row0 == 0) return NAFP_OK;
    if (!workspace) return NAFP_ERR_INVALID_ARG;
    if (workspace_bytes < need) return NAFP_ERR_WORKSPACE;
    const int64_t edges = n_new * deg;
    const HnswRevLayout l = hnsw_rev_layout(row0, edges);
    char* w = (char*)workspace;
    HnswRevParams p{x, n_rows, links, slot, n_link_rows, link_stride, deg, row0, n_new, new_levels, level,
                    (int*)w, (int*)(w + 16), (int*)(w + 16 + row0 * 4), (int*)(w + l.tslot), (int*)(w + l.touched), (int*)(w + l.off),
                    (int*)(w + l.inc), (hnsw_key*)(w + l.keys)};
    hipStream_t st = (hipStream_t)stream;
    NAFP_HIP_CHECK(hipMemsetAsync(w, 0, (size_t)l.clear_bytes, st));
    const dim3 egrid((unsigned)((edges + 255) / 256));
    hipLaunchKernelGGL(hnsw_rev_count_kernel, egrid, dim3(256), 0, st, p);
    NAFP_LAUNCH_CHECK();
    hipLaunchKernelGGL(hnsw_rev_offsets_kernel, dim3(1), dim3(1024), 0, st, p);
    NAFP_LAUNCH_CHECK();
    hipLaunchKernelGGL(hnsw_rev_scatter_kernel, egrid, dim3(256), 0, st, p);
    NAFP_LAUNCH_CHECK();
    const dim3 agrid((unsigned)std::min<int64_t>(std::min<int64_t>(edges, row0), 65536)), block(64);
    if (dim == 64) hipLaunchKernelGGL(hnsw_rev_apply_kernel<64>, agrid, block, 0, st, p);
    else if (dim == 128) hipLaunchKernelGGL(hnsw_rev_apply_kernel<128>, agrid, block, 0, st, p);
    else hipLaunchKernelGGL(hnsw_rev_apply_kernel<256>, agrid, block, 0, st, p);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

int nafp_hnsw_search(const float* x, int64_t n_rows, int dim, const int32_t* links0, const int32_t* links_upper,
                     const int32_t* slot, int64_t n_slots, int M, int entry, int entry_level, const float* query,
                     int64_t n_query, int ef_search, int k, float* out_dist, int32_t* out_ids, void* workspace,
                     int64_t workspace_bytes, void* stream) {
    if (!x || !links0 || !query || !out_dist || !out_ids || n_rows < 0 || n_query < 0 || n_slots < 0 || workspace_bytes < 0 || entry < 0 ||
        entry >= n_rows || (entry_level > 0 && (!links_upper || !slot)))
        return NAFP_ERR_INVALID_ARG;
    const int rc = hnsw_limits(dim, M, entry_level, ef_search, k);
    if (rc != NAFP_OK) return rc;
    if (n_rows > 0x7fffffffll || n_query > 0x3fffffffll) return NAFP_ERR_UNSUPPORTED;
    if (n_query == 0) return NAFP_OK;
    if (!workspace) return NAFP_ERR_INVALID_ARG;
    if (workspace_bytes < nafp_hnsw_search_workspace_bytes(n_query, ef_search, k)) return NAFP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int* cur = (int*)workspace;
    int* nxt = cur + n_query;
    float* scratch_d = out_dist;                      // the descent's one distance per query: the output's first n_query floats, rewritten below
    hipLaunchKernelGGL(hnsw_fill_kernel, dim3((unsigned)((n_query + 255) / 256)), dim3(256), 0, st, cur, (long long)n_query, entry);
    NAFP_LAUNCH_CHECK();
    for (int level = entry_level; level >= 1; --level) {
        HnswSearchParams p{x, n_rows, {links_upper + (level - 1) * M, slot, n_slots, (long long)HNSW_MAX_LEVEL * M, M}, query, cur, nullptr,
                           level, 1, nafp_hnsw_default_max_expansions(1), 1, scratch_d, nxt};
        const int r = hnsw_search_layer_launch(dim, p, n_query, st);
        if (r != NAFP_OK) return r;
        std::swap(cur, nxt);
    }
    const int ef = std::max(ef_search, k);
    HnswSearchParams p{x, n_rows, {links0, nullptr, n_rows, 2ll * M, 2 * M}, query, cur, nullptr, 0, ef, nafp_hnsw_default_max_expansions(ef),
                       k, out_dist, out_ids};
    return hnsw_search_layer_launch(dim, p, n_query, st);
}

}  // extern "C"
