// Exact nearest-neighbour search over resident fingerprints + sequence scoring, gfx950.
//
// The consumer side of the hot path's output: eval/eval_faiss.py:115-289 with the exact index
// (faiss.IndexFlatL2, eval/utils/get_index_faiss.py:57-62).  The whole index ([dummy_db ; db], N x d
// float32: 51 GB for 100 M fingerprints) stays resident in HBM; there is no training, no
// quantisation and no host round trip per query.
//
//   search_half_norms_kernel   h[i] = |x_i|^2 / 2   (+inf padding after N)
//   search_topk_kernel<D,K>    per query the K index rows with the smallest |q - x|^2, i.e. the
//                              largest key = q.x - |x|^2/2.  fp32 MFMA (v_mfma_f32_32x32x2_f32):
//                              A = a 64-row index tile staged by LDS-DMA (XOR-swizzled chunks,
//                              2-stage ring), B = the workgroup's 128 queries held in REGISTERS for the
//                              whole scan (lane <-> one query column), so the index streams through
//                              the chip once per 128 queries.  In the 32x32 C/D layout a lane owns ONE
//                              query and 16 index rows per block: it keeps that query's running top-K
//                              as a sorted register list (threshold test per score, unrolled insertion
//                              only when a score beats the K-th best).  blockIdx.y splits the index.
//   search_topk_excl_kernel<D,K>  the same body with one excluded row range per query (nafp_search_topk_l2_excl): the lane's
//                              clipped (lo, hi) in two registers, tested only where a score has beaten the K-th best
//   search_merge_kernel<K>     merges the 2 x splits partial lists of a query (key desc, id asc)
//   ivf_flat_scan_kernel<D,K>  the same body over one inverted list's rows for the queries that probe it (ivf.hip)
//   search_seq_score_kernel<D> mean_i q[t+i] . x[c+i] for candidate sequence starts c (eval_faiss.py:221-230)
//   search_seq_match_kernel<D> top-k ids -> offset-compensated unique candidates -> scores -> the n_out best (eval_faiss.py:213-232)
//   search_identify_kernel<D>  top-k ids -> (track, alignment) candidates with votes -> overlap-only scores -> the n_out best (eval/identify.py)
//   search_identify_tempo_kernel<D>  the same along slanted lines: (track, tempo hypothesis, alignment) candidates (identify --tempos)
#include "nafp_common.h"

#include <algorithm>

namespace nafp {

using f32x16 = __attribute__((ext_vector_type(16))) float;
typedef unsigned u32x4s __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u32x4s make_rsrc_s(const void* base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)base;
    u32x4s r;
    r.x = __builtin_amdgcn_readfirstlane((unsigned)a);
    r.y = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32) & 0xffffu);
    r.z = __builtin_amdgcn_readfirstlane(bytes);
    r.w = 0x00020000u;
    return r;
}
__device__ __forceinline__ void lds_dma16_s(unsigned lds_addr, unsigned voff, u32x4s rsrc) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 4\n\t"
                 "buffer_load_dwordx4 %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_addr), "v"(voff), "s"(rsrc) : "memory");
}

__global__ __launch_bounds__(256) void search_half_norms_kernel(const float* __restrict__ x, float* __restrict__ hn,
                                                                int64_t N, int64_t n_pad, int D) {
    const int64_t i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= n_pad) return;
    if (i >= N) { hn[i] = INFINITY; return; }
    const float4* r = (const float4*)(x + i * D);
    float s = 0.f;
    for (int c = 0; c < D / 4; ++c) { const float4 v = r[c]; s += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w); }
    hn[i] = 0.5f * s;
}

constexpr int TILE_ROWS = 64;

template <int D, int K, bool EXCL = false>
__device__ __forceinline__ void search_topk_body(
        const float* __restrict__ Q, const float* __restrict__ X, const float* __restrict__ hn,
        float* __restrict__ out_key, int* __restrict__ out_id, int nq, int64_t N, int tiles_per_split, int n_lists,
        int qb, int split, const int* __restrict__ qmap, const int* __restrict__ excl = nullptr) {
    // qb / split: the query block and index split of this workgroup (blockIdx.x / .y for the exact search); qmap: the row of
    // Q that query qn of the block reads (nullptr: row qn; the IVF scan reads its list's queries through it, ivf.hip)
    // EXCL (nafp_search_topk_l2_excl): excl (nq, 2) = the row range [lo, hi) query qn never takes.  A lane owns one query, so the
    // clipped pair is two registers per lane, and the range test sits where a score has already beaten the K-th best.
    constexpr int CH = D / 4;                        // 16-B chunks per row
    constexpr int SWZ = (CH < 32 ? CH : 32) - 1;      // chunk swizzle mask: the row's low bits -- the same for row rl and row 32 + rl, which share `aoff` (d = 256 has 64 chunks)
    constexpr int RPI = 64 / CH;                     // rows per DMA wave-instruction
    constexpr int NI = 16 / RPI;                     // DMA instructions per wave per tile (16 rows per wave)
    constexpr int TILE = TILE_ROWS * D;              // floats
    constexpr unsigned OOB = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) float smem[];      // [2][64][D]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rl = lane & 31, hh = lane >> 5;
    const int qn = qb * 128 + wave * 32 + rl;
    const int64_t n_tiles = (N + TILE_ROWS - 1) / TILE_ROWS;
    const int64_t t0 = (int64_t)split * tiles_per_split;
    const int64_t t1 = std::min<int64_t>(n_tiles, t0 + tiles_per_split);

    // the query column of this lane: q[8kk + 4hh + j], j = 0..3 (the k permutation A uses too)
    float4 qr[D / 8];
#pragma unroll
    for (int kk = 0; kk < D / 8; ++kk)
        qr[kk] = qn < nq ? *(const float4*)(Q + (int64_t)(qmap ? qmap[qn] : qn) * D + 8 * kk + 4 * hh) : make_float4(0.f, 0.f, 0.f, 0.f);

    // the excluded rows of this lane's query, clipped to [0, N] as plain comparisons (any int32 pair is legal; lo >= hi: none)
    int ex_lo = 0, ex_hi = 0;
    if constexpr (EXCL) {
        if (qn < nq) {
            ex_lo = std::min(std::max(excl[2 * (int64_t)qn], 0), (int)N);
            ex_hi = std::min(std::max(excl[2 * (int64_t)qn + 1], 0), (int)N);
        }
    }

    float sc[K]; int id[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { sc[j] = -INFINITY; id[j] = -1; }

    const unsigned lds0 = (unsigned)(unsigned long long)(__attribute__((address_space(3))) void*)smem;
    // DMA geometry: wave w stages rows [16w, 16w+16) of the tile; instruction i covers rows
    // 16w + i*RPI + lane/CH, physical chunk lane%CH holding logical chunk pc ^ swz(row)
    unsigned voff[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int row = wave * 16 + i * RPI + lane / CH;
        const int lc = (lane % CH) ^ (row & SWZ);
        voff[i] = (unsigned)(row * D + lc * 4) * 4u;
    }
#define NAFP_S_DMA(t_, slot_)                                                                       \
    {                                                                                               \
        const int64_t row0_l = (t_) * TILE_ROWS;                                                    \
        const int64_t left_l = (N - row0_l) * D * 4;                                                \
        const u32x4s rs_l = make_rsrc_s(X + row0_l * D, (unsigned)std::min<int64_t>(left_l, TILE * 4)); \
        _Pragma("unroll") for (int i = 0; i < NI; ++i)                                              \
            lds_dma16_s(lds0 + (unsigned)(((slot_) * TILE + (wave * 16 + i * RPI) * D) * 4), voff[i], rs_l); \
    }
    (void)OOB;
    if (t0 < t1) NAFP_S_DMA(t0, 0)
    // The f32 MFMAs share the SIMD's issue time with every vector instruction (conv.hip), so the scan loop is written for
    // instruction count: operand addresses are per-lane constants (the swizzled chunk of every kk, computed once) plus
    // immediates, the accumulators start at -|x|^2/2 (the key needs no subtraction), and a block of 16 scores is tested
    // against the K-th best with one max tree before any per-score work.
    unsigned aoff[D / 8];                          // byte offset of (row rl, logical chunk 2kk + hh) inside a tile
#pragma unroll
    for (int kk = 0; kk < D / 8; ++kk) aoff[kk] = (unsigned)((rl * D + (((2 * kk + hh) ^ (rl & SWZ)) * 4)) * 4);
    const char* sbase = (const char*)smem;
#define NAFP_S_TILE(SLOT_)                                                                          \
    {                                                                                               \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                            \
        __builtin_amdgcn_s_barrier();                                                               \
        asm volatile("" ::: "memory");                                                              \
        if (t + 1 < t1) NAFP_S_DMA(t + 1, (SLOT_) ^ 1)                                              \
        const float* hp = hn + t * TILE_ROWS;                  /* wave-uniform -> scalar loads */   \
        f32x16 acc[2];                                                                              \
        _Pragma("unroll") for (int mi = 0; mi < 2; ++mi)                                            \
            _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                        \
                const int o = mi * 32 + 8 * (r >> 2) + (r & 3);                                     \
                acc[mi][r] = -(hh ? hp[o + 4] : hp[o]);                                             \
            }                                                                                       \
        _Pragma("unroll") for (int kk = 0; kk < D / 8; ++kk) {                                      \
            float4 a[2];                                                                            \
            _Pragma("unroll") for (int mi = 0; mi < 2; ++mi)                                        \
                a[mi] = *(const float4*)(sbase + aoff[kk] + ((SLOT_) * TILE + mi * 32 * D) * 4);    \
            _Pragma("unroll") for (int mi = 0; mi < 2; ++mi) {                                      \
                acc[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].x, qr[kk].x, acc[mi], 0, 0, 0); \
                acc[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].y, qr[kk].y, acc[mi], 0, 0, 0); \
                acc[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].z, qr[kk].z, acc[mi], 0, 0, 0); \
                acc[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi].w, qr[kk].w, acc[mi], 0, 0, 0); \
            }                                                                                       \
        }                                                                                           \
        /* selection: D[i = index row][j = query]: this lane holds rows (r&3) + 8(r>>2) + 4hh of block mi */ \
        const int base_id = (int)(t * TILE_ROWS);                                                   \
        _Pragma("unroll") for (int mi = 0; mi < 2; ++mi) {                                          \
            float m = fmaxf(acc[mi][0], acc[mi][1]);                                                \
            _Pragma("unroll") for (int r = 2; r < 16; r += 2) m = fmaxf(m, fmaxf(acc[mi][r], acc[mi][r + 1])); \
            if (m > sc[K - 1]) {                                                                    \
                _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                    \
                    const float key = acc[mi][r];                                                   \
                    if (key > sc[K - 1]) {                                                          \
                        const int nid = base_id + mi * 32 + 8 * (r >> 2) + (r & 3) + 4 * hh;        \
                        if (!EXCL || nid < ex_lo || nid >= ex_hi) {                                 \
                            _Pragma("unroll") for (int j = K - 1; j >= 1; --j) {                    \
                                const bool cj = key > sc[j], cp = key > sc[j - 1];                  \
                                id[j] = cj ? (cp ? id[j - 1] : nid) : id[j];                        \
                                sc[j] = cj ? (cp ? sc[j - 1] : key) : sc[j];                        \
                            }                                                                       \
                            if (key > sc[0]) { sc[0] = key; id[0] = nid; }                          \
                        }                                                                           \
                    }                                                                               \
                }                                                                                   \
            }                                                                                       \
        }                                                                                           \
        if (++t >= t1) break;                                                                       \
    }
    if (t0 < t1)
        for (int64_t t = t0;;) {
            NAFP_S_TILE(0)
            NAFP_S_TILE(1)
        }
#undef NAFP_S_TILE
#undef NAFP_S_DMA
    if (qn < nq) {
        const int64_t o = ((int64_t)qn * n_lists + split * 2 + hh) * K;
#pragma unroll
        for (int j = 0; j < K; ++j) { out_key[o + j] = sc[j]; out_id[o + j] = id[j]; }
    }
}

template <int D, int K>
__global__ __launch_bounds__(256, 2) void search_topk_kernel(
        const float* __restrict__ Q, const float* __restrict__ X, const float* __restrict__ hn,
        float* __restrict__ out_key, int* __restrict__ out_id, int nq, int64_t N, int tiles_per_split, int n_lists) {
    search_topk_body<D, K>(Q, X, hn, out_key, out_id, nq, N, tiles_per_split, n_lists, blockIdx.x, blockIdx.y, nullptr);
}
// d = 256 (EMB_SZ 256: the encoder and NT-Xent support it, so the exact index does too): a lane keeps 128 floats of its query
// column, and the 2-tile ring is 128 KB of LDS -- one workgroup per CU either way, so the kernel may use the whole register file
template <int K>
__global__ __launch_bounds__(256, 1) void search_topk_kernel_d256(
        const float* __restrict__ Q, const float* __restrict__ X, const float* __restrict__ hn,
        float* __restrict__ out_key, int* __restrict__ out_id, int nq, int64_t N, int tiles_per_split, int n_lists) {
    search_topk_body<256, K>(Q, X, hn, out_key, out_id, nq, N, tiles_per_split, n_lists, blockIdx.x, blockIdx.y, nullptr);
}
// The masked search (nafp_search_topk_l2_excl): the same body with the per-query range test compiled in.  The partial lists have
// the layout of the unmasked kernels, so search_merge_kernel serves both.
template <int D, int K>
__global__ __launch_bounds__(256, 2) void search_topk_excl_kernel(
        const float* __restrict__ Q, const float* __restrict__ X, const float* __restrict__ hn, const int* __restrict__ excl,
        float* __restrict__ out_key, int* __restrict__ out_id, int nq, int64_t N, int tiles_per_split, int n_lists) {
    search_topk_body<D, K, true>(Q, X, hn, out_key, out_id, nq, N, tiles_per_split, n_lists, blockIdx.x, blockIdx.y, nullptr, excl);
}
template <int K>
__global__ __launch_bounds__(256, 1) void search_topk_excl_kernel_d256(
        const float* __restrict__ Q, const float* __restrict__ X, const float* __restrict__ hn, const int* __restrict__ excl,
        float* __restrict__ out_key, int* __restrict__ out_id, int nq, int64_t N, int tiles_per_split, int n_lists) {
    search_topk_body<256, K, true>(Q, X, hn, out_key, out_id, nq, N, tiles_per_split, n_lists, blockIdx.x, blockIdx.y, nullptr, excl);
}

// IVF-Flat scan (ivf.hip, nafp_ivf_flat_search): the body above over ONE inverted list's rows (padded to whole tiles, +inf half
// norms in the padding) with a 128-query block of the (query, probe) pairs that probe that list as the query block.  Task x
// (blockIdx.x) = (list l, query block qb) found in the prefix of per-list query blocks; blockIdx.y = one of `parts` row splits.
// Ids written are rows relative to the list's first row; the merge maps them back through the list's id array.
template <int D, int K>
__device__ __forceinline__ void ivf_flat_scan_body(const float* __restrict__ Q, const int* __restrict__ qmap,
                                                   const int* __restrict__ pair_off, const int* __restrict__ qblk_off, int nlist,
                                                   const float* __restrict__ Xs, const float* __restrict__ hns,
                                                   const int* __restrict__ row_off, float* __restrict__ pk, int* __restrict__ pi,
                                                   int parts) {
    const int task = blockIdx.x;
    if (task >= qblk_off[nlist]) return;                          // the grid is an upper bound of the task count
    int lo = 0, hi = nlist;                                       // the largest l with qblk_off[l] <= task
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (qblk_off[mid] <= task) lo = mid; else hi = mid; }
    const int p0 = pair_off[lo], r0 = row_off[lo];
    const int64_t N = row_off[lo + 1] - r0;
    const int64_t n_tiles = N / TILE_ROWS;
    const int tps = (int)((n_tiles + parts - 1) / parts);
    search_topk_body<D, K>(Q, Xs + (int64_t)r0 * D, hns + r0, pk + (int64_t)p0 * 2 * parts * K, pi + (int64_t)p0 * 2 * parts * K,
                           pair_off[lo + 1] - p0, N, tps, 2 * parts, task - qblk_off[lo], blockIdx.y, qmap + p0);
}
template <int D, int K>
__global__ __launch_bounds__(256, 2) void ivf_flat_scan_kernel(const float* __restrict__ Q, const int* __restrict__ qmap,
        const int* __restrict__ pair_off, const int* __restrict__ qblk_off, int nlist, const float* __restrict__ Xs,
        const float* __restrict__ hns, const int* __restrict__ row_off, float* __restrict__ pk, int* __restrict__ pi, int parts) {
    ivf_flat_scan_body<D, K>(Q, qmap, pair_off, qblk_off, nlist, Xs, hns, row_off, pk, pi, parts);
}
template <int K>
__global__ __launch_bounds__(256, 1) void ivf_flat_scan_kernel_d256(const float* __restrict__ Q, const int* __restrict__ qmap,
        const int* __restrict__ pair_off, const int* __restrict__ qblk_off, int nlist, const float* __restrict__ Xs,
        const float* __restrict__ hns, const int* __restrict__ row_off, float* __restrict__ pk, int* __restrict__ pi, int parts) {
    ivf_flat_scan_body<256, K>(Q, qmap, pair_off, qblk_off, nlist, Xs, hns, row_off, pk, pi, parts);
}

template <int D, int K>
static int launch_ivf_flat(unsigned grid_x, int parts, const float* Q, const int* qmap, const int* pair_off, const int* qblk_off,
                           int nlist, const float* Xs, const float* hns, const int* row_off, float* pk, int* pi, hipStream_t st) {
    const int lds = 2 * TILE_ROWS * D * (int)sizeof(float);
    const dim3 grid(grid_x, (unsigned)parts);
    if constexpr (D == 256) {
        NAFP_HIP_CHECK(hipFuncSetAttribute((const void*)ivf_flat_scan_kernel_d256<K>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        ivf_flat_scan_kernel_d256<K><<<grid, 256, lds, st>>>(Q, qmap, pair_off, qblk_off, nlist, Xs, hns, row_off, pk, pi, parts);
    } else {
        NAFP_HIP_CHECK(hipFuncSetAttribute((const void*)ivf_flat_scan_kernel<D, K>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        ivf_flat_scan_kernel<D, K><<<grid, 256, lds, st>>>(Q, qmap, pair_off, qblk_off, nlist, Xs, hns, row_off, pk, pi, parts);
    }
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

// host entry for ivf.hip (same library): K is 20 or 32, D 64 / 128 / 256
int ivf_flat_scan_launch(int D, int K, unsigned grid_x, int parts, const float* Q, const int* qmap, const int* pair_off,
                         const int* qblk_off, int nlist, const float* Xs, const float* hns, const int* row_off, float* pk, int* pi,
                         hipStream_t st) {
#define NAFP_IVF_L(D_, K_) launch_ivf_flat<D_, K_>(grid_x, parts, Q, qmap, pair_off, qblk_off, nlist, Xs, hns, row_off, pk, pi, st)
    if (D == 128) return K == 20 ? NAFP_IVF_L(128, 20) : NAFP_IVF_L(128, 32);
    if (D == 256) return K == 20 ? NAFP_IVF_L(256, 20) : NAFP_IVF_L(256, 32);
    return K == 20 ? NAFP_IVF_L(64, 20) : NAFP_IVF_L(64, 32);
#undef NAFP_IVF_L
}

__device__ __forceinline__ unsigned long long pack_key(float key, int id) {
    unsigned u = __float_as_uint(key);
    u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;                 // order-preserving map
    return ((unsigned long long)u << 32) | (unsigned)(0x7fffffff - id);      // ties: smaller id is larger
}

// one wave per query: K rounds of wave-wide arg-max over the n_lists*K partial results
template <int K>
__global__ __launch_bounds__(64) void search_merge_kernel(const float* __restrict__ in_key, const int* __restrict__ in_id,
                                                          const float* __restrict__ Q, float* __restrict__ out_dist,
                                                          int* __restrict__ out_ids, int n_lists, int D, int k_out) {
    extern __shared__ unsigned long long cand[];
    const int q = blockIdx.x, lane = threadIdx.x;
    const int M = n_lists * K;
    for (int i = lane; i < M; i += 64) {
        const int idv = in_id[(int64_t)q * M + i];
        cand[i] = idv >= 0 ? pack_key(in_key[(int64_t)q * M + i], idv) : 0ull;
    }
    float qq = 0.f;
    for (int c = lane; c < D; c += 64) { const float v = Q[(int64_t)q * D + c]; qq += v * v; }
    qq = wave_sum(qq);
    __syncthreads();
    for (int j = 0; j < k_out; ++j) {
        unsigned long long best = 0ull; int bi = -1;
        for (int i = lane; i < M; i += 64)
            if (cand[i] > best) { best = cand[i]; bi = i; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ob > best) { best = ob; bi = oi; }
        }
        if (lane == 0) {
            if (best == 0ull) { out_ids[(int64_t)q * k_out + j] = -1; out_dist[(int64_t)q * k_out + j] = INFINITY; }
            else {
                out_ids[(int64_t)q * k_out + j] = in_id[(int64_t)q * M + bi];
                out_dist[(int64_t)q * k_out + j] = fmaxf(qq - 2.f * in_key[(int64_t)q * M + bi], 0.f);
                cand[bi] = 0ull;
            }
        }
        __syncthreads();
    }
}

// mean_{i < len} Q[q0 + i] . X[c + i] by one wave (every lane returns it): the ONE fp32 summation order of the sequence score --
// lane l chains fmaf over (i, e = l, l + 64, ..), then the xor-butterfly, then one division.  search_seq_score_kernel and
// search_seq_match_kernel both call it, so a candidate has the same bits on either path.
template <int D>
__device__ __forceinline__ float seq_score_wave(const float* __restrict__ Q, const float* __restrict__ X, int q0, int c, int len,
                                                int lane) {
    float s = 0.f;
    for (int i = 0; i < len; ++i) {
        const float* qp = Q + (int64_t)(q0 + i) * D; const float* xp = X + (int64_t)(c + i) * D;
        for (int e = lane; e < D; e += 64) s = fmaf(qp[e], xp[e], s);
    }
    s = wave_sum(s);
    return s / (float)len;
}

// out[task, slot] = mean_{i < min(len, N - c)} Q[q0 + i] . X[c + i]  for c = cand[task, slot] >= 0, else -inf.
// One wave per (task, slot).
template <int D>
__global__ __launch_bounds__(256) void search_seq_score_kernel(
        const float* __restrict__ Q, const float* __restrict__ X, const int* __restrict__ task_q0,
        const int* __restrict__ task_len, const int* __restrict__ cand, float* __restrict__ out, int64_t N,
        int n_slots, int64_t total) {
    const int64_t w = blockIdx.x * 4ll + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= total) return;
    const int task = (int)(w / n_slots);
    const int c = cand[w];
    if (c < 0 || c >= N) { if (lane == 0) out[w] = -INFINITY; return; }
    const int q0 = task_q0[task];
    const int len = (int)std::min<int64_t>(task_len[task], N - c);
    const float s = seq_score_wave<D>(Q, X, q0, c, len, lane);
    if (lane == 0) out[w] = s;
}

// Sequence matching, from the top-k ids of the segment search to the ranked predictions (eval_faiss.py:213-232), one workgroup
// of 256 threads per task (include/nafp.h, nafp_search_seq_match, states the contract):
//   1. gather   slot (i, j) -> c = topk[q0 + i, j] - i into LDS; absent / out-of-range / negative -> SEQM_NONE; the slots are
//               padded to P, the power of two that holds this task's k * len slots
//   2. sort     bitonic, ascending, in LDS: equal candidates become runs, SEQM_NONE goes to the end
//   3. compact  the first element of each run, by ballot and prefix counts (no atomic slot allocation: the unique list is in
//               ascending id order whatever the timing), into the low word of the key array
//   4. score    the four waves walk the unique candidates, seq_score_wave once each; a NaN or -inf score drops the candidate
//               (key 0), every other becomes pack_key(score, c) in place
//   5. select   wave 0: n_out rounds of arg-max over the keys below the previous round's.  Keys are distinct (ids are), so no
//               round writes; the score comes back out of the key bit for bit.
// LDS: P ints + P keys = 12 P bytes (24 KB at the 2048-slot maximum), no global scratch, no atomics.
constexpr int SEQM_NONE = 0x7fffffff;             // never a candidate: n_index < 2^31 keeps c <= 2^31 - 2
constexpr int SEQM_MAX_SLOTS = 2048;

__device__ __forceinline__ float unpack_key_score(unsigned long long key) {
    unsigned u = (unsigned)(key >> 32);
    u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;
    return __uint_as_float(u);
}

template <int D>
__global__ __launch_bounds__(256) void search_seq_match_kernel(
        const float* __restrict__ Q, int n_query, const float* __restrict__ X, int64_t N, const int* __restrict__ topk, int k,
        const int* __restrict__ task_q0, const int* __restrict__ task_len, int max_len, int n_out, int* __restrict__ out_ids,
        float* __restrict__ out_scores, int* __restrict__ out_n_cand, int p_max) {
    extern __shared__ unsigned long long seqm_keys[];            // [p_max] keys, then [p_max] ints
    int* ids = (int*)(seqm_keys + p_max);
    __shared__ int wcnt[4];
    const int task = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q0 = task_q0[task];
    int len = 0;
    if (q0 >= 0 && q0 < n_query) len = std::max(0, std::min(std::min(task_len[task], max_len), n_query - q0));
    const int S = k * len;                                         // <= k * max_len <= p_max
    int P = 1;
    while (P < S) P <<= 1;

    // 1. gather
    for (int s = tid; s < P; s += 256) {
        int c = SEQM_NONE;
        if (s < S) {
            const int i = s / k;
            const int id = topk[(int64_t)(q0 + i) * k + (s - i * k)];
            if (id >= 0 && id < N && id >= i) c = id - i;
        }
        ids[s] = c;
    }
    __syncthreads();
    // 2. bitonic sort
    for (int kk = 2; kk <= P; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += 256) {
                const int p = i ^ j;
                if (p > i) {
                    const int a = ids[i], b = ids[p];
                    if ((a > b) == ((i & kk) == 0)) { ids[i] = b; ids[p] = a; }
                }
            }
            __syncthreads();
        }
    // 3. compact the run heads, 256 slots at a time
    int n_uniq = 0;
    for (int base = 0; base < P; base += 256) {
        const int i = base + tid;
        int c = SEQM_NONE;
        bool head = false;
        if (i < P) { c = ids[i]; head = c != SEQM_NONE && (i == 0 || ids[i - 1] != c); }
        const unsigned long long m = __ballot(head);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int before = n_uniq;
        for (int w = 0; w < wave; ++w) before += wcnt[w];
        if (head) seqm_keys[before + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned long long)(unsigned)c;
        n_uniq += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    // 4. score each unique candidate once
    int kept = 0;
    for (int n = wave; n < n_uniq; n += 4) {
        const int c = (int)(unsigned)seqm_keys[n];
        const int l = (int)std::min<int64_t>(len, N - c);
        const float sc = seq_score_wave<D>(Q, X, q0, c, l, lane);
        const bool keep = !(sc != sc) && sc != -INFINITY;
        kept += keep ? 1 : 0;
        if (lane == 0) seqm_keys[n] = keep ? pack_key(sc, c) : 0ull;
    }
    if (lane == 0) wcnt[wave] = kept;
    __syncthreads();
    if (wave != 0) return;
    if (lane == 0 && out_n_cand) out_n_cand[task] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    // 5. n_out rounds of arg-max
    unsigned long long prev = ~0ull;                              // above every key: the low word of a key is <= 0x7fffffff
    for (int r = 0; r < n_out; ++r) {
        unsigned long long best = 0ull;
        for (int n = lane; n < n_uniq; n += 64) {
            const unsigned long long v = seqm_keys[n];
            if (v < prev && v > best) best = v;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long ob = __shfl_xor(best, o, 64);
            if (ob > best) best = ob;
        }
        if (lane == 0) {
            out_ids[(int64_t)task * n_out + r] = best ? 0x7fffffff - (int)(unsigned)best : -1;
            out_scores[(int64_t)task * n_out + r] = best ? unpack_key_score(best) : -INFINITY;
        }
        prev = best;                                              // 0 once the candidates run out: the later rounds find nothing
    }
}

// Identification: the track-aware sequence matcher, one workgroup of 256 threads per task (include/nafp.h,
// nafp_search_identify, states the contract):
//   1. gather    slot (i, j) -> key = track << 32 | (a + IDENT_BIAS), a = topk[q0 + i, j] - i (any sign), track by one binary
//                search of track_first; absent / out-of-range ids -> IDENT_NONE; the slots are padded to P, the power of two that
//                holds this task's k * len slots
//   2. sort      bitonic, ascending, in LDS: equal (track, a) pairs become runs, IDENT_NONE goes to the end
//   3. compact   the first element of each run and its position, by ballot and prefix counts (no atomic slot allocation); the
//                next run's position (or the number of valid slots) minus its own is the run's length = the votes
//   4. filter    overlap with the track and the votes against the two minima; a survivor n becomes the 32-bit selection key
//                (8192 - votes) << 13 | n -- the unique list is in (track, a) order, so n breaks the vote ties as the contract
//                says -- every other slot 0xffffffff; the survivors are counted by ballot
//   5. shortlist a second bitonic sort, of the selection keys: the first n_short are the shortlist
//   6. score     the four waves walk the shortlist, seq_score_wave once each over the overlap only
//   7. select    wave 0: n_out rounds of arg-max by (score descending, key ascending) below the previous round's
// LDS: P keys + P ints = 12 P bytes (96 KB at the 8192-slot maximum, 6 KB for the default 20 x 20 window) + 6 KB static.
constexpr unsigned long long IDENT_NONE = ~0ull;
constexpr int IDENT_BIAS = 1 << 14;               // a >= -(8192 - 1), so a + bias > 0; n_index <= 2^31 - 2^14 keeps it in 31 bits
constexpr int IDENT_MAX_SLOTS = 8192;
constexpr int IDENT_MAX_SHORT = 256;

template <typename T>
__device__ __forceinline__ void bitonic_sort_lds(T* v, int P, int tid) {
    for (int kk = 2; kk <= P; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const T a = v[i], b = v[p];
                if ((a > b) == ((i & kk) == 0)) { v[i] = b; v[p] = a; }
            }
            __syncthreads();
        }
}

// the overlap [i0, i1) of a window of len rows laid at alignment a with track tr, clipped to the rows the index has
__device__ __forceinline__ void ident_overlap(const int* __restrict__ first, int n_tracks, int64_t N, int tr, int a, int len,
                                              int* i0, int* i1) {
    const int64_t lo = std::max<int64_t>(first[tr], 0), hi = std::min<int64_t>(first[tr + 1], N);
    *i0 = (int)std::max<int64_t>(0, lo - a);
    *i1 = (int)std::max<int64_t>(*i0, std::min<int64_t>(len, hi - a));
}

template <int D>
__global__ __launch_bounds__(256) void search_identify_kernel(
        const float* __restrict__ Q, int n_query, const float* __restrict__ X, int64_t N, const int* __restrict__ topk, int k,
        const int* __restrict__ task_q0, const int* __restrict__ task_len, int max_len, const int* __restrict__ first, int n_tracks,
        int min_overlap, int min_votes, int n_short, int n_out, int* __restrict__ out_track, int* __restrict__ out_align,
        float* __restrict__ out_score, int* __restrict__ out_votes, int* __restrict__ out_overlap, int* __restrict__ out_n_cand,
        int p_max) {
    extern __shared__ unsigned long long ident_keys[];           // [p_max] keys, then [p_max] unsigned
    unsigned* aux = (unsigned*)(ident_keys + p_max);
    __shared__ unsigned long long sl_key[IDENT_MAX_SHORT];
    __shared__ unsigned sl_su[IDENT_MAX_SHORT];                  // the score as an ordered unsigned; 0: dropped
    __shared__ float sl_score[IDENT_MAX_SHORT];
    __shared__ int sl_votes[IDENT_MAX_SHORT], sl_ov[IDENT_MAX_SHORT];
    __shared__ int wcnt[4], wval[4];
    const int task = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q0 = task_q0[task];
    int len = 0;
    if (q0 >= 0 && q0 < n_query) len = std::max(0, std::min(std::min(task_len[task], max_len), n_query - q0));
    const int S = k * len;                                         // <= k * max_len <= p_max
    int P = 1;
    while (P < S) P <<= 1;

    // 1. gather
    for (int s = tid; s < P; s += 256) {
        unsigned long long key = IDENT_NONE;
        if (s < S) {
            const int i = s / k;
            const int id = topk[(int64_t)(q0 + i) * k + (s - i * k)];
            if (id >= 0 && id < N) {
                int lo = 0, hi = n_tracks - 1;                       // the last track whose first row is <= id
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (first[mid] <= id) lo = mid; else hi = mid - 1;
                }
                key = ((unsigned long long)(unsigned)lo << 32) | (unsigned)(id - i + IDENT_BIAS);
            }
        }
        ident_keys[s] = key;
    }
    __syncthreads();
    // 2. sort
    bitonic_sort_lds(ident_keys, P, tid);
    // 3. compact the run heads and their positions, 256 slots at a time.  Head i moves to a slot <= i, and slot base - 1, which the
    //    next pass reads as its first predecessor, can only have been written by element base - 1 itself.
    int n_uniq = 0, n_valid = 0;
    for (int base = 0; base < P; base += 256) {
        const int i = base + tid;
        unsigned long long c = IDENT_NONE;
        bool head = false;
        if (i < P) { c = ident_keys[i]; head = c != IDENT_NONE && (i == 0 || ident_keys[i - 1] != c); }
        const unsigned long long m = __ballot(head), mv = __ballot(c != IDENT_NONE);
        if (lane == 0) { wcnt[wave] = __popcll(m); wval[wave] = __popcll(mv); }
        __syncthreads();
        int before = n_uniq;
        for (int w = 0; w < wave; ++w) before += wcnt[w];
        if (head) {
            const int pos = before + __popcll(m & ((1ull << lane) - 1ull));
            ident_keys[pos] = c;
            aux[pos] = (unsigned)i;
        }
        n_uniq += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        n_valid += wval[0] + wval[1] + wval[2] + wval[3];
        __syncthreads();
    }
    // 4. votes, overlap, the two minima -> selection keys in place of the positions
    int P2 = 1;
    while (P2 < n_uniq) P2 <<= 1;                                  // <= P: n_uniq <= S
    const int need_ov = std::min(min_overlap, len);
    int n_cand = 0;
    for (int base = 0; base < P2; base += 256) {
        const int n = base + tid;
        unsigned sel = 0xffffffffu;
        if (n < n_uniq) {
            const int v = (int)(n + 1 < n_uniq ? aux[n + 1] : (unsigned)n_valid) - (int)aux[n];
            const unsigned long long key = ident_keys[n];
            int i0, i1;
            ident_overlap(first, n_tracks, N, (int)(key >> 32), (int)(unsigned)key - IDENT_BIAS, len, &i0, &i1);
            if (i1 - i0 >= need_ov && i1 > i0 && v >= min_votes) sel = ((unsigned)(IDENT_MAX_SLOTS - v) << 13) | (unsigned)n;
        }
        const unsigned long long m = __ballot(sel != 0xffffffffu);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();                                           // every aux[n + 1] of this pass is read
        if (n < P2) aux[n] = sel;
        n_cand += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    if (tid == 0 && out_n_cand) out_n_cand[task] = n_cand;
    // 5. shortlist
    bitonic_sort_lds(aux, P2, tid);
    const int n_sl = std::min(n_short, n_cand);
    // 6. score each shortlisted candidate once, over its overlap
    for (int m = wave; m < n_sl; m += 4) {
        const unsigned sel = aux[m];
        const unsigned long long key = ident_keys[sel & 8191u];
        const int a = (int)(unsigned)key - IDENT_BIAS;
        int i0, i1;
        ident_overlap(first, n_tracks, N, (int)(key >> 32), a, len, &i0, &i1);
        const float sc = seq_score_wave<D>(Q, X, q0 + i0, a + i0, i1 - i0, lane);
        if (lane == 0) {
            const bool keep = !(sc != sc) && sc != -INFINITY;
            unsigned u = __float_as_uint(sc == 0.f ? 0.f : sc);       // -0 ranks with +0
            u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
            sl_key[m] = key; sl_su[m] = keep ? u : 0u; sl_score[m] = sc;
            sl_votes[m] = IDENT_MAX_SLOTS - (int)(sel >> 13); sl_ov[m] = i1 - i0;
        }
    }
    __syncthreads();
    if (wave != 0) return;
    // 7. n_out rounds of arg-max: score descending, then (track, a) ascending.  The keys are distinct, so the order is total.
    unsigned long long prev_su = 1ull << 32, prev_key = 0ull;      // above every candidate
    for (int r = 0; r < n_out; ++r) {
        unsigned long long b_su = 0ull, b_key = IDENT_NONE;
        int b_m = -1;
        for (int m = lane; m < n_sl; m += 64) {
            const unsigned long long su = sl_su[m], key = sl_key[m];
            const bool below = su < prev_su || (su == prev_su && key > prev_key);
            const bool better = su > b_su || (su == b_su && key < b_key);
            if (su != 0ull && below && better) { b_su = su; b_key = key; b_m = m; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long o_su = __shfl_xor(b_su, o, 64), o_key = __shfl_xor(b_key, o, 64);
            const int o_m = __shfl_xor(b_m, o, 64);
            if (o_su > b_su || (o_su == b_su && o_key < b_key)) { b_su = o_su; b_key = o_key; b_m = o_m; }
        }
        if (lane == 0) {
            const int64_t o = (int64_t)task * n_out + r;
            const bool got = b_m >= 0;
            out_track[o] = got ? (int)(b_key >> 32) : -1;
            out_align[o] = got ? (int)(unsigned)b_key - IDENT_BIAS : 0;
            out_score[o] = got ? sl_score[b_m] : -INFINITY;
            out_votes[o] = got ? sl_votes[b_m] : 0;
            out_overlap[o] = got ? sl_ov[b_m] : 0;
        }
        if (b_m < 0) { prev_su = 0ull; prev_key = IDENT_NONE; }   // the candidates ran out: the later rounds find nothing
        else { prev_su = b_su; prev_key = b_key; }
    }
}

// Identification under tempo hypotheses: search_identify_kernel along slanted lines (include/nafp.h,
// nafp_search_identify_tempo, states the contract).  Hypothesis r advances off_r(i) = (i * rho[r] + 32768) >> 16 library rows in
// i query segments, so slot (i, j) gives one key per r: track << 36 | r << 32 | (a + IDENT_BIAS), a = topk[q0 + i, j] - off_r(i)
// (off_r(8191) <= 10239 at rho = 81920: the bias of 2^14 still covers it).  The seven steps and the 12 P bytes of LDS are those of
// search_identify_kernel with P the power of two that holds k * len * n_rho slots; what differs:
//   1. gather    one binary search of track_first per slot, then n_rho keys; the keys of hypothesis r lie at [r * k * len, ..)
//   4. filter    i0 / i1 = the first segment whose row a + off_r(i) reaches the track's first row / the next track's: two binary
//                searches over i (off_r is non-decreasing); the rows of [i0, i1) then lie in the track and in [0, N)
//   6. score     seq_score_wave's order over the rows a + off_r(i): the bits of nafp_search_seq_scores on the gathered rows
// The sorted key order is (track, r, a): it breaks the ties of the shortlist and of the ranking as the contract says.
// The hypotheses come by value in the kernel arguments and are copied to LDS once (a lane-dependent index into an argument
// would be a scratch copy per lane).
constexpr int IDENT_MAX_RHO = 16;
constexpr int IDENT_RHO_MIN = 52429, IDENT_RHO_MAX = 81920;      // 0.8 .. 1.25 in 16.16
struct IdentRho { int v[IDENT_MAX_RHO]; };

__device__ __forceinline__ int ident_off(int i, int rho) { return (i * rho + 32768) >> 16; }      // i < 8192: below 2^30

// the smallest i in [0, len] with a + off(i) >= bound, len if there is none
__device__ __forceinline__ int ident_first_at(int a, int rho, int len, int64_t bound) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)a + ident_off(mid, rho) >= bound) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ void ident_overlap_tempo(const int* __restrict__ first, int64_t N, int tr, int a, int rho, int len,
                                                    int* i0, int* i1) {
    const int64_t lo = std::max<int64_t>(first[tr], 0), hi = std::min<int64_t>(first[tr + 1], N);
    *i0 = ident_first_at(a, rho, len, lo);
    *i1 = std::max(*i0, ident_first_at(a, rho, len, hi));
}

// mean_{i0 <= i < i1} Q[q0 + i] . X[a + off(i)] by one wave, in the order of seq_score_wave
template <int D>
__device__ __forceinline__ float seq_score_wave_tempo(const float* __restrict__ Q, const float* __restrict__ X, int q0, int a,
                                                      int rho, int i0, int i1, int lane) {
    float s = 0.f;
    for (int i = i0; i < i1; ++i) {
        const float* qp = Q + (int64_t)(q0 + i) * D; const float* xp = X + ((int64_t)a + ident_off(i, rho)) * D;
        for (int e = lane; e < D; e += 64) s = fmaf(qp[e], xp[e], s);
    }
    s = wave_sum(s);
    return s / (float)(i1 - i0);
}

template <int D>
__global__ __launch_bounds__(256) void search_identify_tempo_kernel(
        const float* __restrict__ Q, int n_query, const float* __restrict__ X, int64_t N, const int* __restrict__ topk, int k,
        const int* __restrict__ task_q0, const int* __restrict__ task_len, int max_len, const int* __restrict__ first, int n_tracks,
        IdentRho rho, int n_rho, int min_overlap, int min_votes, int n_short, int n_out, int* __restrict__ out_track,
        int* __restrict__ out_align, float* __restrict__ out_score, int* __restrict__ out_votes, int* __restrict__ out_overlap,
        int* __restrict__ out_n_cand, int* __restrict__ out_rho, int p_max) {
    extern __shared__ unsigned long long ident_keys[];           // [p_max] keys, then [p_max] unsigned
    unsigned* aux = (unsigned*)(ident_keys + p_max);
    __shared__ unsigned long long sl_key[IDENT_MAX_SHORT];
    __shared__ unsigned sl_su[IDENT_MAX_SHORT];                  // the score as an ordered unsigned; 0: dropped
    __shared__ float sl_score[IDENT_MAX_SHORT];
    __shared__ int sl_votes[IDENT_MAX_SHORT], sl_ov[IDENT_MAX_SHORT];
    __shared__ int wcnt[4], wval[4], rho_s[IDENT_MAX_RHO];
    const int task = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < IDENT_MAX_RHO) {
        int v = 0;
#pragma unroll
        for (int r = 0; r < IDENT_MAX_RHO; ++r) v = tid == r ? rho.v[r] : v;
        rho_s[tid] = v;
    }
    const int q0 = task_q0[task];
    int len = 0;
    if (q0 >= 0 && q0 < n_query) len = std::max(0, std::min(std::min(task_len[task], max_len), n_query - q0));
    const int S0 = k * len, S = S0 * n_rho;                        // <= k * max_len * n_rho <= p_max
    int P = 1;
    while (P < S) P <<= 1;
    __syncthreads();

    // 1. gather
    for (int s = tid; s < S0; s += 256) {
        const int i = s / k;
        const int id = topk[(int64_t)(q0 + i) * k + (s - i * k)];
        const bool present = id >= 0 && id < N;
        int lo = 0, hi = n_tracks - 1;                             // the last track whose first row is <= id
        while (present && lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (first[mid] <= id) lo = mid; else hi = mid - 1;
        }
        for (int r = 0; r < n_rho; ++r)
            ident_keys[r * S0 + s] = !present ? IDENT_NONE
                : ((unsigned long long)(unsigned)lo << 36) | ((unsigned long long)r << 32) | (unsigned)(id - ident_off(i, rho_s[r]) + IDENT_BIAS);
    }
    for (int s = S + tid; s < P; s += 256) ident_keys[s] = IDENT_NONE;
    __syncthreads();
    // 2. sort
    bitonic_sort_lds(ident_keys, P, tid);
    // 3. compact the run heads and their positions, 256 slots at a time (as search_identify_kernel does)
    int n_uniq = 0, n_valid = 0;
    for (int base = 0; base < P; base += 256) {
        const int i = base + tid;
        unsigned long long c = IDENT_NONE;
        bool head = false;
        if (i < P) { c = ident_keys[i]; head = c != IDENT_NONE && (i == 0 || ident_keys[i - 1] != c); }
        const unsigned long long m = __ballot(head), mv = __ballot(c != IDENT_NONE);
        if (lane == 0) { wcnt[wave] = __popcll(m); wval[wave] = __popcll(mv); }
        __syncthreads();
        int before = n_uniq;
        for (int w = 0; w < wave; ++w) before += wcnt[w];
        if (head) {
            const int pos = before + __popcll(m & ((1ull << lane) - 1ull));
            ident_keys[pos] = c;
            aux[pos] = (unsigned)i;
        }
        n_uniq += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        n_valid += wval[0] + wval[1] + wval[2] + wval[3];
        __syncthreads();
    }
    // 4. votes, overlap, the two minima -> selection keys in place of the positions
    int P2 = 1;
    while (P2 < n_uniq) P2 <<= 1;                                  // <= P: n_uniq <= S
    const int need_ov = std::min(min_overlap, len);
    int n_cand = 0;
    for (int base = 0; base < P2; base += 256) {
        const int n = base + tid;
        unsigned sel = 0xffffffffu;
        if (n < n_uniq) {
            const int v = (int)(n + 1 < n_uniq ? aux[n + 1] : (unsigned)n_valid) - (int)aux[n];
            const unsigned long long key = ident_keys[n];
            int i0, i1;
            ident_overlap_tempo(first, N, (int)(key >> 36), (int)(unsigned)key - IDENT_BIAS, rho_s[(key >> 32) & 15u], len, &i0, &i1);
            if (i1 - i0 >= need_ov && i1 > i0 && v >= min_votes) sel = ((unsigned)(IDENT_MAX_SLOTS - v) << 13) | (unsigned)n;
        }
        const unsigned long long m = __ballot(sel != 0xffffffffu);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();                                           // every aux[n + 1] of this pass is read
        if (n < P2) aux[n] = sel;
        n_cand += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    if (tid == 0 && out_n_cand) out_n_cand[task] = n_cand;
    // 5. shortlist
    bitonic_sort_lds(aux, P2, tid);
    const int n_sl = std::min(n_short, n_cand);
    // 6. score each shortlisted candidate once, over its overlap
    for (int m = wave; m < n_sl; m += 4) {
        const unsigned sel = aux[m];
        const unsigned long long key = ident_keys[sel & 8191u];
        const int a = (int)(unsigned)key - IDENT_BIAS, rh = rho_s[(key >> 32) & 15u];
        int i0, i1;
        ident_overlap_tempo(first, N, (int)(key >> 36), a, rh, len, &i0, &i1);
        const float sc = seq_score_wave_tempo<D>(Q, X, q0, a, rh, i0, i1, lane);
        if (lane == 0) {
            const bool keep = !(sc != sc) && sc != -INFINITY;
            unsigned u = __float_as_uint(sc == 0.f ? 0.f : sc);       // -0 ranks with +0
            u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
            sl_key[m] = key; sl_su[m] = keep ? u : 0u; sl_score[m] = sc;
            sl_votes[m] = IDENT_MAX_SLOTS - (int)(sel >> 13); sl_ov[m] = i1 - i0;
        }
    }
    __syncthreads();
    if (wave != 0) return;
    // 7. n_out rounds of arg-max: score descending, then (track, r, a) ascending.  The keys are distinct, so the order is total.
    unsigned long long prev_su = 1ull << 32, prev_key = 0ull;      // above every candidate
    for (int r = 0; r < n_out; ++r) {
        unsigned long long b_su = 0ull, b_key = IDENT_NONE;
        int b_m = -1;
        for (int m = lane; m < n_sl; m += 64) {
            const unsigned long long su = sl_su[m], key = sl_key[m];
            const bool below = su < prev_su || (su == prev_su && key > prev_key);
            const bool better = su > b_su || (su == b_su && key < b_key);
            if (su != 0ull && below && better) { b_su = su; b_key = key; b_m = m; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long o_su = __shfl_xor(b_su, o, 64), o_key = __shfl_xor(b_key, o, 64);
            const int o_m = __shfl_xor(b_m, o, 64);
            if (o_su > b_su || (o_su == b_su && o_key < b_key)) { b_su = o_su; b_key = o_key; b_m = o_m; }
        }
        if (lane == 0) {
            const int64_t o = (int64_t)task * n_out + r;
            const bool got = b_m >= 0;
            out_track[o] = got ? (int)(b_key >> 36) : -1;
            out_align[o] = got ? (int)(unsigned)b_key - IDENT_BIAS : 0;
            out_rho[o] = got ? (int)((b_key >> 32) & 15u) : -1;
            out_score[o] = got ? sl_score[b_m] : -INFINITY;
            out_votes[o] = got ? sl_votes[b_m] : 0;
            out_overlap[o] = got ? sl_ov[b_m] : 0;
        }
        if (b_m < 0) { prev_su = 0ull; prev_key = IDENT_NONE; }   // the candidates ran out: the later rounds find nothing
        else { prev_su = b_su; prev_key = b_key; }
    }
}

template <int D, int K>
static int launch_topk(const float* Q, int nq, const float* X, const float* hn, int64_t N, float* pk, int* pi, int splits,
                       int tps, hipStream_t st) {
    const int lds = 2 * TILE_ROWS * D * (int)sizeof(float);
    const dim3 grid((unsigned)((nq + 127) / 128), (unsigned)splits);
    if constexpr (D == 256) {
        NAFP_HIP_CHECK(hipFuncSetAttribute((const void*)search_topk_kernel_d256<K>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        search_topk_kernel_d256<K><<<grid, 256, lds, st>>>(Q, X, hn, pk, pi, nq, N, tps, 2 * splits);
    } else {
        NAFP_HIP_CHECK(hipFuncSetAttribute((const void*)search_topk_kernel<D, K>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        search_topk_kernel<D, K><<<grid, 256, lds, st>>>(Q, X, hn, pk, pi, nq, N, tps, 2 * splits);
    }
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

template <int D, int K>
static int launch_topk_excl(const float* Q, int nq, const float* X, const float* hn, const int* excl, int64_t N, float* pk, int* pi,
                            int splits, int tps, hipStream_t st) {
    const int lds = 2 * TILE_ROWS * D * (int)sizeof(float);
    const dim3 grid((unsigned)((nq + 127) / 128), (unsigned)splits);
    if constexpr (D == 256) {
        NAFP_HIP_CHECK(hipFuncSetAttribute((const void*)search_topk_excl_kernel_d256<K>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        search_topk_excl_kernel_d256<K><<<grid, 256, lds, st>>>(Q, X, hn, excl, pk, pi, nq, N, tps, 2 * splits);
    } else {
        NAFP_HIP_CHECK(hipFuncSetAttribute((const void*)search_topk_excl_kernel<D, K>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        search_topk_excl_kernel<D, K><<<grid, 256, lds, st>>>(Q, X, hn, excl, pk, pi, nq, N, tps, 2 * splits);
    }
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

static void plan_splits(int nq, int64_t N, int K, int* splits, int* tps) {
    const int64_t n_tiles = (N + TILE_ROWS - 1) / TILE_ROWS;
    const int q_tiles = (nq + 127) / 128;
    int64_t s = std::max<int64_t>(1, 2048 / q_tiles);
    s = std::min<int64_t>(s, std::max<int64_t>(1, n_tiles / 8));     // at least 8 tiles per workgroup
    s = std::min<int64_t>(s, 4096 / (2 * K));                          // merge kernel: <= 4096 partial results
    *tps = (int)((n_tiles + s - 1) / s);
    *splits = (int)((n_tiles + *tps - 1) / *tps);
}

}  // namespace nafp

using namespace nafp;

extern "C" int64_t nafp_search_index_aux_floats(int64_t n_index) {
    return n_index < 0 ? -1 : (n_index + 63) / 64 * 64 + 64;
}

extern "C" int nafp_search_index_prepare(const float* index, int64_t n_index, int dim, float* aux, void* stream) {
    if (!index || !aux || n_index <= 0) return NAFP_ERR_INVALID_ARG;
    if (dim != 64 && dim != 128 && dim != 256) return NAFP_ERR_UNSUPPORTED;
    const int64_t n_pad = nafp_search_index_aux_floats(n_index);
    search_half_norms_kernel<<<(unsigned)((n_pad + 255) / 256), 256, 0, (hipStream_t)stream>>>(index, aux, n_index, n_pad, dim);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int64_t nafp_search_workspace_bytes(int64_t n_query, int64_t n_index, int k) {
    if (n_query < 0 || n_index <= 0 || k <= 0 || k > 32 || n_query > (1 << 30)) return -1;
    const int K = k <= 20 ? 20 : 32;
    int splits, tps;
    plan_splits((int)n_query, n_index, K, &splits, &tps);
    return (int64_t)n_query * 2 * splits * K * 8 + 256;
}

extern "C" int nafp_search_topk_l2(const float* query, int64_t n_query, const float* index, const float* aux,
                                   int64_t n_index, int dim, int k, float* out_dist, int32_t* out_ids,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    if (!query || !index || !aux || !out_dist || !out_ids || !workspace || n_query < 0 || n_index <= 0 || k <= 0)
        return NAFP_ERR_INVALID_ARG;
    if ((dim != 64 && dim != 128 && dim != 256) || k > 32 || n_index >= ((int64_t)1 << 31) || n_query > (1 << 30)) return NAFP_ERR_UNSUPPORTED;
    if (n_query == 0) return NAFP_OK;
    if (workspace_bytes < nafp_search_workspace_bytes(n_query, n_index, k)) return NAFP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int K = k <= 20 ? 20 : 32;
    int splits, tps;
    plan_splits((int)n_query, n_index, K, &splits, &tps);
    char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    float* pk = (float*)ws;
    int* pi = (int*)(ws + (int64_t)n_query * 2 * splits * K * 4);
    int rc;
    if (dim == 128) rc = K == 20 ? launch_topk<128, 20>(query, (int)n_query, index, aux, n_index, pk, pi, splits, tps, st)
                                 : launch_topk<128, 32>(query, (int)n_query, index, aux, n_index, pk, pi, splits, tps, st);
    else if (dim == 256) rc = K == 20 ? launch_topk<256, 20>(query, (int)n_query, index, aux, n_index, pk, pi, splits, tps, st)
                                      : launch_topk<256, 32>(query, (int)n_query, index, aux, n_index, pk, pi, splits, tps, st);
    else            rc = K == 20 ? launch_topk<64, 20>(query, (int)n_query, index, aux, n_index, pk, pi, splits, tps, st)
                                 : launch_topk<64, 32>(query, (int)n_query, index, aux, n_index, pk, pi, splits, tps, st);
    if (rc != NAFP_OK) return rc;
    const int M = 2 * splits * K;
    if (K == 20) search_merge_kernel<20><<<(unsigned)n_query, 64, M * 8, st>>>(pk, pi, query, out_dist, out_ids, 2 * splits, dim, k);
    else         search_merge_kernel<32><<<(unsigned)n_query, 64, M * 8, st>>>(pk, pi, query, out_dist, out_ids, 2 * splits, dim, k);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int nafp_search_topk_l2_excl(const float* query, int64_t n_query, const float* index, const float* aux,
                                        int64_t n_index, int dim, int k, const int32_t* excl, float* out_dist, int32_t* out_ids,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
    if (!query || !index || !aux || !excl || !out_dist || !out_ids || !workspace || n_query < 0 || n_index <= 0 || k <= 0)
        return NAFP_ERR_INVALID_ARG;
    if ((dim != 64 && dim != 128 && dim != 256) || k > 32 || n_index >= ((int64_t)1 << 31) || n_query > (1 << 30)) return NAFP_ERR_UNSUPPORTED;
    if (n_query == 0) return NAFP_OK;
    if (workspace_bytes < nafp_search_workspace_bytes(n_query, n_index, k)) return NAFP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int K = k <= 20 ? 20 : 32;
    int splits, tps;
    plan_splits((int)n_query, n_index, K, &splits, &tps);
    char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    float* pk = (float*)ws;
    int* pi = (int*)(ws + (int64_t)n_query * 2 * splits * K * 4);
#define NAFP_TOPK_X(D_, K_) launch_topk_excl<D_, K_>(query, (int)n_query, index, aux, excl, n_index, pk, pi, splits, tps, st)
    int rc;
    if (dim == 128) rc = K == 20 ? NAFP_TOPK_X(128, 20) : NAFP_TOPK_X(128, 32);
    else if (dim == 256) rc = K == 20 ? NAFP_TOPK_X(256, 20) : NAFP_TOPK_X(256, 32);
    else rc = K == 20 ? NAFP_TOPK_X(64, 20) : NAFP_TOPK_X(64, 32);
#undef NAFP_TOPK_X
    if (rc != NAFP_OK) return rc;
    const int M = 2 * splits * K;
    if (K == 20) search_merge_kernel<20><<<(unsigned)n_query, 64, M * 8, st>>>(pk, pi, query, out_dist, out_ids, 2 * splits, dim, k);
    else         search_merge_kernel<32><<<(unsigned)n_query, 64, M * 8, st>>>(pk, pi, query, out_dist, out_ids, 2 * splits, dim, k);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int nafp_search_seq_scores(const float* query, const float* index, int64_t n_index, int dim,
                                      const int32_t* task_q0, const int32_t* task_len, int64_t n_tasks,
                                      const int32_t* cand, int n_slots, float* out_scores, void* stream) {
    if (!query || !index || !task_q0 || !task_len || !cand || !out_scores || n_tasks < 0 || n_slots <= 0 || n_index <= 0)
        return NAFP_ERR_INVALID_ARG;
    if (dim != 64 && dim != 128 && dim != 256) return NAFP_ERR_UNSUPPORTED;
    const int64_t total = n_tasks * n_slots;
    if (total == 0) return NAFP_OK;
    const unsigned blocks = (unsigned)((total + 3) / 4);
    if (dim == 128) search_seq_score_kernel<128><<<blocks, 256, 0, (hipStream_t)stream>>>(query, index, task_q0, task_len, cand, out_scores, n_index, n_slots, total);
    else if (dim == 256) search_seq_score_kernel<256><<<blocks, 256, 0, (hipStream_t)stream>>>(query, index, task_q0, task_len, cand, out_scores, n_index, n_slots, total);
    else            search_seq_score_kernel<64><<<blocks, 256, 0, (hipStream_t)stream>>>(query, index, task_q0, task_len, cand, out_scores, n_index, n_slots, total);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int nafp_search_seq_match(const float* query, int64_t n_query, const float* index, int64_t n_index, int dim,
                                     const int32_t* topk_ids, int k, const int32_t* task_q0, const int32_t* task_len,
                                     int64_t n_tasks, int max_len, int n_out, int32_t* out_ids, float* out_scores,
                                     int32_t* out_n_cand, void* stream) {
    if (!query || !index || !topk_ids || !task_q0 || !task_len || !out_ids || !out_scores || n_query < 0 || n_index < 0 || n_tasks < 0)
        return NAFP_ERR_INVALID_ARG;
    if (dim != 64 && dim != 128 && dim != 256) return NAFP_ERR_UNSUPPORTED;
    if (k < 1 || k > 32 || max_len < 1 || k * (int64_t)max_len > SEQM_MAX_SLOTS || n_out < 1 || n_out > 32) return NAFP_ERR_UNSUPPORTED;
    if (n_index >= ((int64_t)1 << 31) || n_query >= ((int64_t)1 << 31) || n_tasks >= ((int64_t)1 << 31)) return NAFP_ERR_UNSUPPORTED;
    if (n_tasks == 0) return NAFP_OK;
    int p_max = 1;
    while (p_max < k * max_len) p_max <<= 1;
    const int lds = p_max * 12;
    hipStream_t st = (hipStream_t)stream;
#define NAFP_SEQM(D_) search_seq_match_kernel<D_><<<(unsigned)n_tasks, 256, lds, st>>>(query, (int)n_query, index, n_index, topk_ids, k, \
        task_q0, task_len, max_len, n_out, out_ids, out_scores, out_n_cand, p_max)
    if (dim == 128) NAFP_SEQM(128);
    else if (dim == 256) NAFP_SEQM(256);
    else NAFP_SEQM(64);
#undef NAFP_SEQM
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int nafp_search_identify_check_tracks_host(const int32_t* track_first_host, int n_tracks, int64_t n_index) {
    if (!track_first_host || n_tracks < 1 || n_index < 1 || n_index >= ((int64_t)1 << 31)) return NAFP_ERR_INVALID_ARG;
    if (track_first_host[0] != 0 || track_first_host[n_tracks] != n_index) return NAFP_ERR_INVALID_ARG;
    for (int t = 0; t < n_tracks; ++t)
        if (track_first_host[t + 1] <= track_first_host[t]) return NAFP_ERR_INVALID_ARG;
    return NAFP_OK;
}

extern "C" int nafp_search_identify(const float* query, int64_t n_query, const float* index, int64_t n_index, int dim,
                                    const int32_t* topk_ids, int k, const int32_t* task_q0, const int32_t* task_len,
                                    int64_t n_tasks, int max_len, const int32_t* track_first, int n_tracks, int min_overlap,
                                    int min_votes, int n_short, int n_out, int32_t* out_track, int32_t* out_align,
                                    float* out_score, int32_t* out_votes, int32_t* out_overlap, int32_t* out_n_cand, void* stream) {
    if (!query || !index || !topk_ids || !task_q0 || !task_len || !track_first || !out_track || !out_align || !out_score ||
        !out_votes || !out_overlap || n_query < 0 || n_index < 0 || n_tasks < 0)
        return NAFP_ERR_INVALID_ARG;
    if (dim != 64 && dim != 128 && dim != 256) return NAFP_ERR_UNSUPPORTED;
    if (k < 1 || k > 32 || max_len < 1 || k * (int64_t)max_len > IDENT_MAX_SLOTS) return NAFP_ERR_UNSUPPORTED;
    if (n_short < 1 || n_short > IDENT_MAX_SHORT || n_out < 1 || n_out > 32 || n_out > n_short) return NAFP_ERR_UNSUPPORTED;
    if (min_overlap < 1 || min_votes < 1 || n_tracks < 1 || n_tracks > (1 << 24)) return NAFP_ERR_UNSUPPORTED;
    if (n_index > ((int64_t)1 << 31) - IDENT_BIAS || n_query >= ((int64_t)1 << 31) || n_tasks >= ((int64_t)1 << 31)) return NAFP_ERR_UNSUPPORTED;
    if (n_tasks == 0) return NAFP_OK;
    int p_max = 1;
    while (p_max < k * max_len) p_max <<= 1;
    const int lds = p_max * 12;                                    // sized by this task set, not by the limit: 96 KB only at 8192 slots
    hipStream_t st = (hipStream_t)stream;
#define NAFP_IDENT(D_)                                                                                                          \
    {                                                                                                                           \
        if (lds > 48 * 1024)                                                                                                    \
            NAFP_HIP_CHECK(hipFuncSetAttribute((const void*)search_identify_kernel<D_>, hipFuncAttributeMaxDynamicSharedMemorySize, lds)); \
        search_identify_kernel<D_><<<(unsigned)n_tasks, 256, lds, st>>>(query, (int)n_query, index, n_index, topk_ids, k, task_q0,  \
            task_len, max_len, track_first, n_tracks, min_overlap, min_votes, n_short, n_out, out_track, out_align, out_score,    \
            out_votes, out_overlap, out_n_cand, p_max);                                                                         \
    }
    if (dim == 128) NAFP_IDENT(128)
    else if (dim == 256) NAFP_IDENT(256)
    else NAFP_IDENT(64)
#undef NAFP_IDENT
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int nafp_search_identify_tempo(const float* query, int64_t n_query, const float* index, int64_t n_index, int dim,
                                          const int32_t* topk_ids, int k, const int32_t* task_q0, const int32_t* task_len,
                                          int64_t n_tasks, int max_len, const int32_t* track_first, int n_tracks,
                                          const int32_t* rho_host, int n_rho, int min_overlap, int min_votes, int n_short,
                                          int n_out, int32_t* out_track, int32_t* out_align, float* out_score, int32_t* out_votes,
                                          int32_t* out_overlap, int32_t* out_n_cand, int32_t* out_rho, void* stream) {
    if (!query || !index || !topk_ids || !task_q0 || !task_len || !track_first || !rho_host || !out_track || !out_align ||
        !out_score || !out_votes || !out_overlap || !out_rho || n_query < 0 || n_index < 0 || n_tasks < 0)
        return NAFP_ERR_INVALID_ARG;
    if (dim != 64 && dim != 128 && dim != 256) return NAFP_ERR_UNSUPPORTED;
    if (n_rho < 1 || n_rho > IDENT_MAX_RHO) return NAFP_ERR_UNSUPPORTED;
    if (k < 1 || k > 32 || max_len < 1 || k * (int64_t)max_len * n_rho > IDENT_MAX_SLOTS) return NAFP_ERR_UNSUPPORTED;
    if (n_short < 1 || n_short > IDENT_MAX_SHORT || n_out < 1 || n_out > 32 || n_out > n_short) return NAFP_ERR_UNSUPPORTED;
    if (min_overlap < 1 || min_votes < 1 || n_tracks < 1 || n_tracks > (1 << 24)) return NAFP_ERR_UNSUPPORTED;
    if (n_index > ((int64_t)1 << 31) - IDENT_BIAS || n_query >= ((int64_t)1 << 31) || n_tasks >= ((int64_t)1 << 31)) return NAFP_ERR_UNSUPPORTED;
    IdentRho rho = {};
    for (int r = 0; r < n_rho; ++r) {
        if (rho_host[r] < IDENT_RHO_MIN || rho_host[r] > IDENT_RHO_MAX) return NAFP_ERR_UNSUPPORTED;
        rho.v[r] = rho_host[r];
    }
    if (n_tasks == 0) return NAFP_OK;
    int p_max = 1;
    while (p_max < k * max_len * n_rho) p_max <<= 1;
    const int lds = p_max * 12;
    hipStream_t st = (hipStream_t)stream;
#define NAFP_IDENT_TEMPO(D_)                                                                                                    \
    {                                                                                                                           \
        if (lds > 48 * 1024)                                                                                                    \
            NAFP_HIP_CHECK(hipFuncSetAttribute((const void*)search_identify_tempo_kernel<D_>, hipFuncAttributeMaxDynamicSharedMemorySize, lds)); \
        search_identify_tempo_kernel<D_><<<(unsigned)n_tasks, 256, lds, st>>>(query, (int)n_query, index, n_index, topk_ids, k,  \
            task_q0, task_len, max_len, track_first, n_tracks, rho, n_rho, min_overlap, min_votes, n_short, n_out, out_track,    \
            out_align, out_score, out_votes, out_overlap, out_n_cand, out_rho, p_max);                                          \
    }
    if (dim == 128) NAFP_IDENT_TEMPO(128)
    else if (dim == 256) NAFP_IDENT_TEMPO(256)
    else NAFP_IDENT_TEMPO(64)
#undef NAFP_IDENT_TEMPO
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

// ---- in-training mini search(model/utils/mini_search_subroutines.py:28-220) ------------------------------
namespace nafp {

// scores[q, x] = max(|q|^2 + |x|^2 - 2 q.x, 0)  (mode 0)  or  q.x  (mode 1); any dim (1024 for the un-projected
// features f(.), 128 for the fingerprints).  32 x 32 output tile per workgroup, operands staged through LDS.
__global__ __launch_bounds__(256) void pairwise_scores_kernel(const float* __restrict__ Q, const float* __restrict__ X,
                                                              float* __restrict__ out, int nQ, int nD, int D, int mode) {
    __shared__ float sq[32][33], sx[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;           // 32 x 8
    const int q0 = blockIdx.y * 32, x0 = blockIdx.x * 32;
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, qq[4] = {0.f, 0.f, 0.f, 0.f}, xx = 0.f;
    for (int k0 = 0; k0 < D; k0 += 32) {
        for (int r = ty; r < 32; r += 8) {
            sq[r][tx] = (q0 + r < nQ && k0 + tx < D) ? Q[(int64_t)(q0 + r) * D + k0 + tx] : 0.f;
            sx[r][tx] = (x0 + r < nD && k0 + tx < D) ? X[(int64_t)(x0 + r) * D + k0 + tx] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < 32; ++k) {
            const float xv = sx[tx][k];
            xx = fmaf(xv, xv, xx);
#pragma unroll
            for (int j = 0; j < 4; ++j) { const float qv = sq[ty + 8 * j][k]; acc[j] = fmaf(qv, xv, acc[j]); qq[j] = fmaf(qv, qv, qq[j]); }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = q0 + ty + 8 * j, x = x0 + tx;
        if (q < nQ && x < nD) out[(int64_t)q * nD + x] = mode == 1 ? acc[j] : fmaxf(qq[j] + xx - 2.f * acc[j], 0.f);
    }
}

// rank[t] = number of candidate starts c whose length-s diagonal sum beats the ground truth's (conv_eye_func +
// argsort + np.where(sorted == gt)): smaller sum wins in mode 0, larger in mode 1; equal sums: smaller id first.
__global__ __launch_bounds__(256) void diag_rank_kernel(const float* __restrict__ scores, int* __restrict__ rank, int nQ, int nD,
                                                        int s, int mode, int gt_offset) {
    const int t = blockIdx.x, tid = threadIdx.x;
    const int n_c = nD - s + 1, gt = t + gt_offset;
    __shared__ float ref;
    __shared__ int cnt[4];
    if (tid == 0) {
        float r = 0.f;
        for (int i = 0; i < s; ++i) r += scores[(int64_t)(t + i) * nD + gt + i];
        ref = r;
    }
    __syncthreads();
    const float r = ref;
    int mine = 0;
    for (int c = tid; c < n_c; c += 256) {
        float v = 0.f;
        for (int i = 0; i < s; ++i) v += scores[(int64_t)(t + i) * nD + c + i];
        const bool better = mode == 1 ? (v > r || (v == r && c > gt)) : (v < r || (v == r && c < gt));   // argsort order incl. the reversal
        mine += better ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((tid & 63) == 0) cnt[tid >> 6] = mine;
    __syncthreads();
    if (tid == 0) rank[t] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

}  // namespace nafp

extern "C" int nafp_minisearch_scores(const float* query, const float* db, int64_t n_query, int64_t n_db, int dim, int mode,
                                      float* out_scores, void* stream) {
    if (!query || !db || !out_scores || n_query <= 0 || n_db <= 0 || dim <= 0) return NAFP_ERR_INVALID_ARG;
    if ((mode != 0 && mode != 1) || n_query > (1 << 20) || n_db > (1 << 20)) return NAFP_ERR_UNSUPPORTED;
    pairwise_scores_kernel<<<dim3((unsigned)((n_db + 31) / 32), (unsigned)((n_query + 31) / 32)), 256, 0, (hipStream_t)stream>>>(
        query, db, out_scores, (int)n_query, (int)n_db, dim, mode);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int nafp_minisearch_ranks(const float* scores, int64_t n_query, int64_t n_db, int scope, int mode, int gt_id_offset,
                                     int32_t* out_rank, void* stream) {
    if (!scores || !out_rank || scope <= 0 || n_query < scope || n_db < scope) return NAFP_ERR_INVALID_ARG;
    if (mode != 0 && mode != 1) return NAFP_ERR_UNSUPPORTED;
    const int n_t = (int)(n_query - scope + 1);
    if (gt_id_offset < 0 || n_t - 1 + gt_id_offset > n_db - scope) return NAFP_ERR_INVALID_ARG;
    diag_rank_kernel<<<n_t, 256, 0, (hipStream_t)stream>>>(scores, out_rank, (int)n_query, (int)n_db, scope, mode, gt_id_offset);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}
