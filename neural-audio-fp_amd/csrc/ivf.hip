// Approximate indexes: IVF-Flat, IVF-PQ and IVFPQ-RR (faiss IndexIVFFlat / IndexIVFPQ / IndexIVFPQR as
// eval/utils/get_index_faiss.py:64-80 builds them), gfx950.  Opt-in from eval/eval_faiss.py (NAFP_APPROX_INDEX=1, NAFP_IVFPQ_RR=1);
// the host side is eval/ivf.py.
//
//   ivf_bucket_{count,scan_tiles,offsets,scatter}_kernel   stable counting sort of item ids by key (histogram per 4096-item
//                              tile, scan over tiles per bucket, scan over buckets, scatter).  The scatter keeps ascending ids
//                              inside a bucket: one wave per tile walks its items in order, 64 at a time, and ranks equal keys
//                              inside the 64 by ballots over the key bits -- no atomic slot claims.  Serves the inverted lists
//                              (rows by list), the k-means update (training points by cluster) and the search ((query, probe)
//                              pairs by list).  `batch` independent sorts at once (the M sub-quantizers of PQ training).
//   ivf_kmeans_update_kernel   centroid = mean of its bucketed points, summed in bucket (= ascending id) order in double:
//                              no float atomics, so training is bit-reproducible
//   ivf_pq_encode_kernel<DSUB> residual to the assigned coarse centroid, then per sub-space the nearest of 256 codewords
//                              (equal distances: the smaller code); the codebooks of 64 / DSUB sub-spaces (64 KB) sit in LDS,
//                              blockIdx.y walks the sub-space groups (d = 128: 128 KB of codebooks, 2 groups; d = 256: 4)
//   ivf_probe_kernel           per query the nprobe nearest coarse centroids (exact fp32 |q - c|^2; rank by counting, ties:
//                              smaller list id)
//   ivf_flat_lists_kernel      the lists' rows copied contiguously, each list padded to whole 64-row tiles (+inf half norms)
//   ivf_flat_scan_kernel       (search.hip) the exact search's fp32-MFMA body over one list for the queries probing it
//   the three IVF-PQ scans     one workgroup per (query, list) pair and part of the list.  What they share is written once:
//                              ivf_scan_prologue (residual to the coarse centroid; the 64 x 256 ADC table in LDS through
//                              ivf_adc_entry, fp32 or rounded once to binary16; the part's rows), IvfRowCodes::load (a row's 64
//                              code bytes, loaded one row ahead) and ivf_row_key (64 LDS lookups, summed in fp32 in sub-space
//                              order).  Each kernel keeps its own loop header, selection and LDS carve-up
//                              (ivf_pq_scan*_lds_bytes next to it):
//   ivf_pq_scan_kernel<DSUB,K>      fp32 table.  K sorted entries per lane in registers, then a workgroup-wide K-way arg-max
//                              over the lane lists parked in the table area
//   ivf_pq_scan_f16_kernel<DSUB,K>  binary16 table (NAFP_IVF_LUT_F16, the reference's useFloat16 lookup tables).  K sorted
//                              entries per lane, each wave reduces its 64 lane lists in registers (K rounds of a wave
//                              arg-max of the heads, the winner shifts its list), the 4 x K wave results ranked by counting
//   ivf_pq_scan_wide_kernel<DSUB,LUT>  IVFPQ-RR's first stage, either table, K <= 128 at run time.  A filter per wave
//                              (threshold + LDS candidate buffer, pruned to K by bisection when full), the 4 x (<= K) wave
//                              results ranked by counting
//   ivf_pq_adc_tables_kernel<DSUB,LUT>  the tables themselves for given (query, list) pairs (ivf_adc_entry, as the scans)
//   ivf_merge_kernel           per query: the probes' partial lists -> k results (distance asc, id asc), -1 / +inf padding
//   ivf_pq_residual2_kernel    x - decode(codes): what the refine quantizer is trained on and encodes
//   ivf_refine_encode_kernel<DR>  per row the nearest of 16 codewords in each of 4 sub-spaces of DR = 16 / 32 / 64 dimensions
//   ivf_pqr_rerank_kernel<DSUB>  per query: the candidates' list, PQ code and refine code gathered, the fp32 distance to the
//                              refined reconstruction, the k nearest
#include "nafp_common.h"

#include <hip/hip_fp16.h>

#include <algorithm>
#include <type_traits>

namespace nafp {

int ivf_flat_scan_launch(int D, int K, unsigned grid_x, int parts, const float* Q, const int* qmap, const int* pair_off,
                         const int* qblk_off, int nlist, const float* Xs, const float* hns, const int* row_off, float* pk, int* pi,
                         hipStream_t st);                                     // search.hip

constexpr int BUCKET_TILE = 4096;           // items per wave in the bucketing kernels
constexpr int IVF_MAX_BUCKETS = 16384;      // one int per bucket in LDS (64 KB)
constexpr int IVF_MAX_CANDS = 16384;        // partial results per query in the merge (128 KB of LDS)
constexpr int PQ_KS = 256;                  // codewords per sub-space (nbits = 8)
constexpr int PQ_M = 64;                    // sub-quantizers

__device__ __forceinline__ unsigned long long ivf_pack(float key, int id) {
    unsigned u = __float_as_uint(key);
    u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;                              // order-preserving map
    return ((unsigned long long)u << 32) | (unsigned)(0x7fffffff - id);       // ties: smaller id is larger
}
__device__ __forceinline__ float ivf_unpack_key(unsigned long long v) {
    unsigned u = (unsigned)(v >> 32);
    u = (u >> 31) ? (u ^ 0x80000000u) : ~u;
    return __uint_as_float(u);
}
__device__ __forceinline__ int ivf_unpack_id(unsigned long long v) { return 0x7fffffff - (int)(unsigned)(v & 0xffffffffull); }

template <typename KT>
__device__ __forceinline__ int bucket_key(const KT* keys, int64_t i, int batch, int b) { return (int)keys[i * batch + b]; }

// ---- stable counting sort ------------------------------------------------------------------------------------------
template <typename KT>
__global__ __launch_bounds__(64) void ivf_bucket_count_kernel(const KT* __restrict__ keys, int64_t n, int nb, int batch,
                                                              int* __restrict__ tile_counts, int n_tiles) {
    extern __shared__ int cnt[];
    const int lane = threadIdx.x, t = blockIdx.x, b = blockIdx.y;
    for (int j = lane; j < nb; j += 64) cnt[j] = 0;
    __syncthreads();
    const int64_t i0 = (int64_t)t * BUCKET_TILE, i1 = std::min<int64_t>(n, i0 + BUCKET_TILE);
    for (int64_t i = i0 + lane; i < i1; i += 64) {
        const int k = bucket_key(keys, i, batch, b);
        if ((unsigned)k < (unsigned)nb) atomicAdd(&cnt[k], 1);               // integer counts: order-free
    }
    __syncthreads();
    int* out = tile_counts + ((int64_t)b * n_tiles + t) * nb;
    for (int j = lane; j < nb; j += 64) out[j] = cnt[j];
}

// per (batch, bucket): exclusive prefix over the tiles in place, total into totals
__global__ __launch_bounds__(256) void ivf_bucket_scan_tiles_kernel(int* __restrict__ tile_counts, int n_tiles, int nb,
                                                                    int* __restrict__ totals) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= nb) return;
    int* c = tile_counts + (int64_t)b * n_tiles * nb + j;
    int run = 0;
    for (int t = 0; t < n_tiles; ++t) { const int v = c[(int64_t)t * nb]; c[(int64_t)t * nb] = run; run += v; }
    totals[(int64_t)b * nb + j] = run;
}

// per batch: offsets[0..nb] = exclusive prefix of the totals
__global__ __launch_bounds__(256) void ivf_bucket_offsets_kernel(const int* __restrict__ totals, int nb, int* __restrict__ offsets) {
    __shared__ int part[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int chunk = (nb + 255) / 256, j0 = std::min(nb, tid * chunk), j1 = std::min(nb, j0 + chunk);
    const int* tt = totals + (int64_t)b * nb;
    int s = 0;
    for (int j = j0; j < j1; ++j) s += tt[j];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = run; run += v; }
        offsets[(int64_t)b * (nb + 1) + nb] = run;
    }
    __syncthreads();
    int run = part[tid];
    for (int j = j0; j < j1; ++j) { offsets[(int64_t)b * (nb + 1) + j] = run; run += tt[j]; }
}

template <typename KT>
__global__ __launch_bounds__(64) void ivf_bucket_scatter_kernel(const KT* __restrict__ keys, int64_t n, int nb, int batch,
                                                                const int* __restrict__ tile_prefix, const int* __restrict__ offsets,
                                                                int* __restrict__ ids, int n_tiles, int nbits) {
    extern __shared__ int base[];
    const int lane = threadIdx.x, t = blockIdx.x, b = blockIdx.y;
    const int* tp = tile_prefix + ((int64_t)b * n_tiles + t) * nb;
    const int* of = offsets + (int64_t)b * (nb + 1);
    for (int j = lane; j < nb; j += 64) base[j] = of[j] + tp[j];
    __syncthreads();
    const int64_t i0 = (int64_t)t * BUCKET_TILE, i1 = std::min<int64_t>(n, i0 + BUCKET_TILE);
    const unsigned long long below = (1ull << lane) - 1ull;
    int* out = ids + (int64_t)b * n;
    for (int64_t c0 = i0; c0 < i1; c0 += 64) {                    // items in order, 64 at a time (one wave: lockstep)
        const int64_t i = c0 + lane;
        int k = i < i1 ? bucket_key(keys, i, batch, b) : -1;
        const bool valid = (unsigned)k < (unsigned)nb;
        unsigned long long same = __ballot(valid);
        for (int bit = 0; bit < nbits; ++bit) {                   // lanes with the same key: agree on every key bit
            const bool v = (k >> bit) & 1;
            const unsigned long long bb = __ballot(valid && v);
            same &= v ? bb : ~bb;
        }
        if (valid) {
            const int slot = base[k] + __popcll(same & below);
            out[slot] = (int)i;
            if ((same >> lane) == 1ull) base[k] += __popcll(same);    // the last lane of the group moves the bucket's cursor
        }
        __syncthreads();
    }
}

// ---- k-means update ------------------------------------------------------------------------------------------------
// cluster c of sort b: points ids[b][offsets[c] .. offsets[c+1]), coordinates x[i * dim + b * dsub + dd]
__global__ __launch_bounds__(64) void ivf_kmeans_update_kernel(const float* __restrict__ x, int64_t n, int dim, int dsub,
                                                               const int* __restrict__ offsets, const int* __restrict__ ids,
                                                               int nb, float* __restrict__ cent, int* __restrict__ counts) {
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int* of = offsets + (int64_t)b * (nb + 1);
    const int o0 = of[c], o1 = of[c + 1];
    if (tid == 0) counts[(int64_t)b * nb + c] = o1 - o0;
    if (o1 == o0) return;                                         // empty: the host splits a donor into it
    const int* id = ids + (int64_t)b * n;
    for (int dd = tid; dd < dsub; dd += 64) {
        double s = 0.0;
        for (int p = o0; p < o1; ++p) s += (double)x[(int64_t)id[p] * dim + b * dsub + dd];
        cent[((int64_t)b * nb + c) * dsub + dd] = (float)(s / (double)(o1 - o0));
    }
}

__global__ __launch_bounds__(256) void ivf_residual_kernel(const float* __restrict__ x, int64_t n, int dim,
                                                           const int* __restrict__ assign, const float* __restrict__ cent,
                                                           float* __restrict__ out) {
    const int64_t e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= n * dim) return;
    const int64_t i = e / dim;
    const int dd = (int)(e - i * dim);
    out[e] = x[e] - cent[(int64_t)assign[i] * dim + dd];
}

// ---- PQ encode -----------------------------------------------------------------------------------------------------
template <int DSUB>
__global__ __launch_bounds__(256) void ivf_pq_encode_kernel(const float* __restrict__ x, int64_t n, const int* __restrict__ assign,
                                                            const float* __restrict__ coarse, const float* __restrict__ pq,
                                                            unsigned char* __restrict__ codes) {
    constexpr int D = PQ_M * DSUB, MG = PQ_M / DSUB;             // sub-spaces per workgroup: 64 KB of codebooks
    __shared__ float cb[MG * PQ_KS * DSUB];
    const int tid = threadIdx.x, m0 = blockIdx.y * MG;
    for (int e = tid; e < MG * PQ_KS * DSUB; e += 256) cb[e] = pq[(int64_t)m0 * PQ_KS * DSUB + e];
    __syncthreads();
    const int64_t i = blockIdx.x * 256ll + tid;
    if (i >= n) return;
    const float* xr = x + i * D;
    const float* cr = assign ? coarse + (int64_t)assign[i] * D : nullptr;
    for (int mm = 0; mm < MG; ++mm) {
        const int m = m0 + mm;
        float r[DSUB];
#pragma unroll
        for (int u = 0; u < DSUB; ++u) r[u] = cr ? xr[m * DSUB + u] - cr[m * DSUB + u] : xr[m * DSUB + u];
        float best = INFINITY;
        int bj = 0;
        const float* c = cb + mm * PQ_KS * DSUB;
        for (int j = 0; j < PQ_KS; ++j) {
            float s = 0.f;
#pragma unroll
            for (int u = 0; u < DSUB; ++u) { const float t = r[u] - c[j * DSUB + u]; s += t * t; }
            if (s < best) { best = s; bj = j; }
        }
        codes[i * PQ_M + m] = (unsigned char)bj;
    }
}

// ---- probe selection -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ivf_probe_kernel(const float* __restrict__ Q, const float* __restrict__ cent, int nlist,
                                                        int dim, int nprobe, int* __restrict__ probe) {
    extern __shared__ float sm[];                                 // [dim] query, [nlist] distances
    float* qs = sm;
    float* dist = sm + dim;
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x;
    for (int dd = tid; dd < dim; dd += 256) qs[dd] = Q[q * dim + dd];
    __syncthreads();
    for (int c = tid; c < nlist; c += 256) {
        const float* cr = cent + (int64_t)c * dim;
        float s = 0.f;
        for (int dd = 0; dd < dim; ++dd) { const float t = qs[dd] - cr[dd]; s += t * t; }
        dist[c] = s;
    }
    __syncthreads();
    for (int c = tid; c < nlist; c += 256) {
        const float dc = dist[c];
        int r = 0;
        for (int c2 = 0; c2 < nlist; ++c2) { const float d2 = dist[c2]; r += (d2 < dc || (d2 == dc && c2 < c)) ? 1 : 0; }
        if (r < nprobe) probe[q * nprobe + r] = c;
    }
}

// ---- list storage --------------------------------------------------------------------------------------------------
// row_off[l] = sum over l' < l of the list lengths rounded up to whole tiles
__global__ void ivf_padded_offsets_kernel(const int* __restrict__ off, int nlist, int* __restrict__ row_off) {
    if (threadIdx.x != 0) return;
    int run = 0;
    for (int l = 0; l < nlist; ++l) { row_off[l] = run; run += (off[l + 1] - off[l] + 63) / 64 * 64; }
    row_off[nlist] = run;
}

__device__ __forceinline__ int ivf_find_list(const int* __restrict__ off, int nlist, int64_t p) {
    int lo = 0, hi = nlist;                                       // the largest l with off[l] <= p
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= p) lo = mid; else hi = mid; }
    return lo;
}

__global__ __launch_bounds__(256) void ivf_flat_lists_kernel(const float* __restrict__ x, int dim, const int* __restrict__ off,
                                                             const int* __restrict__ ids, int nlist, const int* __restrict__ row_off,
                                                             int64_t bound, float* __restrict__ xs, float* __restrict__ hn,
                                                             int* __restrict__ row_ids) {
    const int64_t p = blockIdx.x * 256ll + threadIdx.x;
    if (p >= bound || p >= row_off[nlist]) return;
    const int l = ivf_find_list(row_off, nlist, p);
    const int64_t local = p - row_off[l];
    float4* dst = (float4*)(xs + p * dim);
    if (local < off[l + 1] - off[l]) {
        const int src = ids[off[l] + local];
        const float4* r = (const float4*)(x + (int64_t)src * dim);
        float s = 0.f;                                            // search_half_norms_kernel's order
        for (int c = 0; c < dim / 4; ++c) { const float4 v = r[c]; dst[c] = v; s += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w); }
        hn[p] = 0.5f * s;
        row_ids[p] = src;
    } else {
        for (int c = 0; c < dim / 4; ++c) dst[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        hn[p] = INFINITY;
        row_ids[p] = -1;
    }
}

__global__ __launch_bounds__(256) void ivf_gather_codes_kernel(const uint4* __restrict__ codes, const int* __restrict__ ids, int64_t n,
                                                               uint4* __restrict__ out) {
    const int64_t e = blockIdx.x * 256ll + threadIdx.x;            // PQ_M / 16 = 4 uint4 per row
    if (e >= n * 4) return;
    out[e] = codes[(int64_t)ids[e >> 2] * 4 + (e & 3)];
}

// ---- search --------------------------------------------------------------------------------------------------------
// pos = position of pair e = (query e / np, probe e % np) in list order
__global__ __launch_bounds__(256) void ivf_pairs_kernel(const int* __restrict__ sorted, const int* __restrict__ probe, int64_t n_pairs,
                                                        int np, int* __restrict__ qmap, int* __restrict__ plist, int* __restrict__ inv) {
    const int64_t pos = blockIdx.x * 256ll + threadIdx.x;
    if (pos >= n_pairs) return;
    const int e = sorted[pos];
    qmap[pos] = e / np;
    plist[pos] = probe[e];
    inv[e] = (int)pos;
}

__global__ void ivf_qblock_prefix_kernel(const int* __restrict__ pair_off, int nlist, int* __restrict__ qblk_off) {
    if (threadIdx.x != 0) return;
    int run = 0;
    for (int l = 0; l < nlist; ++l) { qblk_off[l] = run; run += (pair_off[l + 1] - pair_off[l] + 127) / 128; }
    qblk_off[nlist] = run;
}

// ---- the IVF-PQ scans' shared pieces --------------------------------------------------------------------------------------
// What an IVF-PQ distance IS, once: the residual, the table entry and its rounding point, the split of a list into parts, the
// load of a row's codes and the 64-lookup sum.  The three scan kernels below differ in their selection only.
constexpr int PQ_NT = PQ_M * PQ_KS;         // entries of an ADC table
template <int LUT> using ivf_lut_t = std::conditional_t<LUT == 0, float, __half>;     // LUT 0: fp32 entries, LUT 1: binary16

// rr[0 .. D) = query q - coarse centroid l (the caller's barrier follows)
template <int DSUB>
__device__ __forceinline__ void ivf_residual_fill(float* rr, const float* Q, int q, const float* coarse, int l) {
    constexpr int D = PQ_M * DSUB;
    for (int dd = threadIdx.x; dd < D; dd += 256) rr[dd] = Q[(int64_t)q * D + dd] - coarse[(int64_t)l * D + dd];
}

// ADC table entry e = m * 256 + c of the residual rr (fp32, D entries): sum_u (rr[m * DSUB + u] - P[m][c][u])^2, u ascending.
// The one place an entry is computed: the scans' table fill (ivf_scan_prologue) and the export call it.
template <int DSUB>
__device__ __forceinline__ float ivf_adc_entry(const float* rr, const float* __restrict__ pq, int e) {
    const int m = e >> 8;
    const float* c = pq + (int64_t)e * DSUB;
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < DSUB; ++u) { const float t = rr[m * DSUB + u] - c[u]; s += t * t; }
    return s;
}

// Workgroup (blockIdx.x, blockIdx.y) = (pair, part): the pair's residual into rr, its ADC table into `table` -- every entry in
// fp32, for LUT 1 rounded once to binary16 (nearest even, subnormals kept: v_cvt_f16_f32 follows the f16 denormal mode, which is
// on) -- and the part's rows: [r0, r1) of the list that starts at row o0 of the sorted codes.  rr is dead after the second barrier.
struct IvfScanTask { int o0, r0, r1; };
template <int DSUB, int LUT>
__device__ __forceinline__ IvfScanTask ivf_scan_prologue(ivf_lut_t<LUT>* table, float* rr, const float* Q, const int* qmap,
                                                         const int* plist, const float* coarse, const float* pq, const int* off,
                                                         int parts) {
    const int tid = threadIdx.x;
    const int64_t pos = blockIdx.x;
    const int part = blockIdx.y;
    const int q = qmap[pos], l = plist[pos];
    ivf_residual_fill<DSUB>(rr, Q, q, coarse, l);
    __syncthreads();
    for (int e = tid; e < PQ_NT; e += 256) {
        const float ent = ivf_adc_entry<DSUB>(rr, pq, e);
        if constexpr (LUT == 0) table[e] = ent;
        else                    table[e] = __float2half_rn(ent);
    }
    __syncthreads();
    const int o0 = off[l];
    const int len = off[l + 1] - o0;
    const int per = (len + parts - 1) / parts;
    const int r0 = std::min(len, part * per);
    return {o0, r0, std::min(len, r0 + per)};
}

// a row's 64 code bytes.  The scans load the next row's before this row's lookups (they come from L2 / MALL; 8 - 16 waves per
// CU hide little): `next.load(..)` ahead of the loop, then per trip `cur = next`, the next load, the lookups of cur.
struct IvfRowCodes {
    uint4 w0 = make_uint4(0u, 0u, 0u, 0u), w1 = w0, w2 = w0, w3 = w0;
    __device__ __forceinline__ void load(const unsigned char* codes, int row) {
        const uint4* cp = (const uint4*)(codes + (int64_t)row * PQ_M);
        w0 = cp[0]; w1 = cp[1]; w2 = cp[2]; w3 = cp[3];
    }
    __device__ __forceinline__ unsigned code(int m) const {      // sub-space m's code (m: a constant of an unrolled loop)
        const unsigned w[16] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w, w3.x, w3.y, w3.z, w3.w};
        return (w[m >> 2] >> (8 * (m & 3))) & 255u;
    }
};

// the key of a row, -distance: the 64 entries its codes pick, m ascending, added in fp32 (binary16 entries widened first).
// The one place a row's distance is computed.
template <int LUT>
__device__ __forceinline__ float ivf_row_key(const ivf_lut_t<LUT>* table, const IvfRowCodes& c) {
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < PQ_M; ++m) {
        if constexpr (LUT == 0) s += table[m * PQ_KS + c.code(m)];
        else                    s += __half2float(table[m * PQ_KS + c.code(m)]);
    }
    return -s;
}

// sorted insert into a lane's descending (sc, id) list; the caller has checked key > sc[K - 1].  Rows ascend within the
// lane, so the strict comparisons keep the smaller id first among equal keys.
template <int K>
__device__ __forceinline__ void ivf_topk_insert(float (&sc)[K], int (&id)[K], float key, int nid) {
#pragma unroll
    for (int j = K - 1; j >= 1; --j) {
        const bool cj = key > sc[j], cp2 = key > sc[j - 1];
        id[j] = cj ? (cp2 ? id[j - 1] : nid) : id[j];
        sc[j] = cj ? (cp2 ? sc[j - 1] : key) : sc[j];
    }
    if (key > sc[0]) { sc[0] = key; id[0] = nid; }
}

// The fp32 narrow scan.  Selection: K sorted entries per lane in registers, then the 256 lane lists go to the table area (the
// table is done) and K rounds of a workgroup-wide arg-max of the heads pick the results.
// LDS: 65 536 B table + 1 024 B residual + 32 B wave bests = 66 592 B: two workgroups per CU.
constexpr int ivf_pq_scan_lds_bytes() { return PQ_NT * 4 + 256 * 4 + 4 * 8; }
template <int DSUB, int K>
__global__ __launch_bounds__(256) void ivf_pq_scan_kernel(const float* __restrict__ Q, const int* __restrict__ qmap,
                                                          const int* __restrict__ plist, const float* __restrict__ coarse,
                                                          const float* __restrict__ pq, const unsigned char* __restrict__ codes,
                                                          const int* __restrict__ off, const int* __restrict__ ids, int parts,
                                                          float* __restrict__ pk, int* __restrict__ pi) {
    extern __shared__ __attribute__((aligned(16))) float lut[];   // [PQ_NT] table, then [256] residual, [4] x u64 wave bests
    float* rr = lut + PQ_NT;
    unsigned long long* wbest = (unsigned long long*)(rr + 256);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t pos = blockIdx.x;
    const int part = blockIdx.y;
    const IvfScanTask t = ivf_scan_prologue<DSUB, 0>(lut, rr, Q, qmap, plist, coarse, pq, off, parts);
    float sc[K]; int id[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { sc[j] = -INFINITY; id[j] = -1; }
    IvfRowCodes next;
    if (t.r0 + tid < t.r1) next.load(codes, t.o0 + t.r0 + tid);
    for (int r = t.r0 + tid; r < t.r1; r += 256) {                // a per-lane trip count
        const IvfRowCodes cur = next;
        if (r + 256 < t.r1) next.load(codes, t.o0 + r + 256);
        const float key = ivf_row_key<0>(lut, cur);
        if (key > sc[K - 1]) ivf_topk_insert<K>(sc, id, key, ids[t.o0 + r]);
    }
    __syncthreads();
    unsigned long long* cl = (unsigned long long*)lut;
#pragma unroll
    for (int j = 0; j < K; ++j) cl[tid * K + j] = id[j] >= 0 ? ivf_pack(sc[j], id[j]) : 0ull;
    __syncthreads();
    int h = 0;
    const int64_t o = (pos * parts + part) * K;
    for (int j = 0; j < K; ++j) {
        const unsigned long long v = h < K ? cl[tid * K + h] : 0ull;
        unsigned long long b = v;
#pragma unroll
        for (int s2 = 32; s2 > 0; s2 >>= 1) { const unsigned long long ob = __shfl_xor(b, s2, 64); b = ob > b ? ob : b; }
        if (lane == 0) wbest[wave] = b;
        __syncthreads();
        unsigned long long best = wbest[0];
        for (int w2 = 1; w2 < 4; ++w2) best = wbest[w2] > best ? wbest[w2] : best;
        if (best != 0ull && v == best) ++h;
        if (tid == 0) {
            pk[o + j] = best ? ivf_unpack_key(best) : -INFINITY;
            pi[o + j] = best ? ivf_unpack_id(best) : -1;
        }
        __syncthreads();
    }
}

// The fp16 narrow scan (NAFP_IVF_LUT_F16): the same rows and sums over the table in binary16.  Table layout: plain [m][c]
// halves, i.e. codes c and c ^ 1 share a dword and dword c / 2 of a sub-table sits on bank (c / 2) % 32.  A lookup instruction
// reads ONE sub-table for all lanes (same m, the lanes' own codes), and the codes of different rows are unrelated, so any
// placement of the 256 entries on 128 dwords puts 4 dwords on each bank and meets the same conflicts; this one needs no address
// arithmetic beyond c * 2 (m * 512 is the instruction's offset) and its table fill is conflict-free.  Lanes with equal or
// paired codes read one dword (broadcast).  Selection: K sorted entries per lane as above, but not through the table area: each
// wave reduces its 64 lane lists in registers, then the 4 x K wave results are ranked by counting.
// LDS: 32 768 B table + 1 024 B residual + 4 * K * 8 B wave results = 34 432 / 34 816 B (K = 20 / 32): four workgroups per CU
// (16 waves, 4 per SIMD); the registers allow that (83 / 116 VGPRs, build/ivf.resources.txt).
constexpr int ivf_pq_scan_f16_lds_bytes(int K) { return PQ_NT * 2 + 256 * 4 + 4 * K * 8; }
template <int DSUB, int K>
__global__ __launch_bounds__(256) void ivf_pq_scan_f16_kernel(const float* __restrict__ Q, const int* __restrict__ qmap,
                                                              const int* __restrict__ plist, const float* __restrict__ coarse,
                                                              const float* __restrict__ pq, const unsigned char* __restrict__ codes,
                                                              const int* __restrict__ off, const int* __restrict__ ids, int parts,
                                                              float* __restrict__ pk, int* __restrict__ pi) {
    extern __shared__ __attribute__((aligned(16))) float lds_f16[];    // [PQ_NT] halves, then [256] residual, [4 * K] x u64 wave results
    __half* lut = (__half*)lds_f16;
    float* rr = lds_f16 + PQ_NT / 2;
    unsigned long long* wres = (unsigned long long*)(rr + 256);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t pos = blockIdx.x;
    const int part = blockIdx.y;
    const IvfScanTask t = ivf_scan_prologue<DSUB, 1>(lut, rr, Q, qmap, plist, coarse, pq, off, parts);
    float sc[K]; int id[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { sc[j] = -INFINITY; id[j] = -1; }
    IvfRowCodes next;
    if (t.r0 + tid < t.r1) next.load(codes, t.o0 + t.r0 + tid);
    for (int r = t.r0 + tid; r < t.r1; r += 256) {                // a per-lane trip count
        const IvfRowCodes cur = next;
        if (r + 256 < t.r1) next.load(codes, t.o0 + r + 256);
        const float key = ivf_row_key<1>(lut, cur);
        if (key > sc[K - 1]) ivf_topk_insert<K>(sc, id, key, ids[t.o0 + r]);
    }
    // wave top-K in registers: K rounds of a wave-wide arg-max of the lanes' heads; the winning lane drops its head (a shift
    // by one with static indices: no scratch).  Packed values are distinct (ids are), 0 = nothing left.
#pragma unroll 1
    for (int j = 0; j < K; ++j) {
        const unsigned long long v = id[0] >= 0 ? ivf_pack(sc[0], id[0]) : 0ull;
        unsigned long long b = v;
#pragma unroll
        for (int s2 = 32; s2 > 0; s2 >>= 1) { const unsigned long long ob = __shfl_xor(b, s2, 64); b = ob > b ? ob : b; }
        if (lane == 0) wres[wave * K + j] = b;
        if (b != 0ull && v == b) {
#pragma unroll
            for (int i = 0; i < K - 1; ++i) { sc[i] = sc[i + 1]; id[i] = id[i + 1]; }
            sc[K - 1] = -INFINITY; id[K - 1] = -1;
        }
    }
    __syncthreads();
    // the 4 x K wave results ranked by counting (distinct values): rank < K goes out, the rest of the K slots is padding
    const int64_t o = (pos * parts + part) * K;
    if (tid < 4 * K) {
        const unsigned long long v = wres[tid];
        int rank = 0, filled = 0;
#pragma unroll 4
        for (int i = 0; i < 4 * K; ++i) { const unsigned long long u = wres[i]; rank += u > v ? 1 : 0; filled += u != 0ull ? 1 : 0; }
        if (v != 0ull && rank < K) { pk[o + rank] = ivf_unpack_key(v); pi[o + rank] = ivf_unpack_id(v); }
        if (tid < K && tid >= filled) { pk[o + tid] = -INFINITY; pi[o + tid] = -1; }
    }
}

// the ADC table of pair p = (query pair_query[p], list pair_list[p]) as the scans build it: out (n_pairs, 64, 256) fp32 (LUT 0)
// or binary16 (LUT 1).  A pair that names a query or a list outside the arrays gets NaNs (nothing is read for it).
template <int DSUB, int LUT>
__global__ __launch_bounds__(256) void ivf_pq_adc_tables_kernel(const float* __restrict__ Q, int64_t n_query, const int* __restrict__ pair_query,
                                                                const int* __restrict__ pair_list, const float* __restrict__ coarse, int nlist,
                                                                const float* __restrict__ pq, void* __restrict__ out) {
    __shared__ float rr[256];
    const int tid = threadIdx.x;
    const int64_t p = blockIdx.x;
    const int q = pair_query[p], l = pair_list[p];
    const bool ok = q >= 0 && q < n_query && l >= 0 && l < nlist;
    if (ok) ivf_residual_fill<DSUB>(rr, Q, q, coarse, l);
    __syncthreads();
    for (int e = tid; e < PQ_NT; e += 256) {
        const float s = ok ? ivf_adc_entry<DSUB>(rr, pq, e) : NAN;
        if (LUT == 0) ((float*)out)[p * PQ_NT + e] = s;
        else          ((__half*)out)[p * PQ_NT + e] = __float2half_rn(s);
    }
}

// ---- IVFPQ-RR: the wide first stage, the refine codes, the re-rank -------------------------------------------------------
// The wide scan (K <= 128 at run time).  K sorted entries per lane do not fit registers, so the selection is a filter: every wave
// keeps a buffer of WIDE_CAP packed (distance, id) candidates in LDS and a threshold, the K-th best it has seen at its last prune.
// A row whose packed value beats the threshold is appended (slot = the wave's count + the lane's rank in the ballot: the count is
// wave-uniform, so neither an atomic nor a barrier is needed inside the scan); when an append would not fit, the wave prunes its
// buffer to its K best: the entries go to registers (WIDE_CAP / 64 per lane), the K-th largest value is found by bisection over the
// 64 bits of the packed value (per round one compare and one ballot per register), and the survivors are written back compacted.
// Packed values are distinct (ids are), so after a prune exactly K remain and the threshold is exact.  What a wave holds at the end
// is the K best of ITS rows whatever the order of appends and the timing of prunes; the 4 x (<= K) wave results are then ranked by
// counting, as the fp16 scan does, and the K best go out sorted.  Results therefore do not depend on scheduling or batching.
// The table fill, the rows and the 64-lookup sum are the narrow scans' (the shared pieces above).
// LDS: the table, then the four buffers (they overlay the residual, which is dead once the table is built) and 4 counts:
// table + 7 680 + 16, i.e. fp32 65 536 + 7 680 + 16 = 73 232 B (two workgroups per CU), fp16 32 768 + 7 680 + 16 = 40 464 B (four).
constexpr int WIDE_CAP = 240;               // candidates per wave buffer (>= 128 + 64: a prune always makes room for one append)
constexpr int WIDE_REGS = (WIDE_CAP + 63) / 64;
constexpr int WIDE_KMAX = 128;

// the wave's buffer -> its K best (cnt > K on entry, all values distinct and non-zero); returns the K-th largest value
__device__ __forceinline__ unsigned long long ivf_wide_prune(unsigned long long* buf, int cnt, int K, int lane) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    unsigned long long v[WIDE_REGS];
#pragma unroll
    for (int j = 0; j < WIDE_REGS; ++j) v[j] = lane + 64 * j < cnt ? buf[lane + 64 * j] : 0ull;
    unsigned long long t = 0ull;
#pragma unroll 1
    for (int bit = 63; bit >= 0; --bit) {                         // the largest t with at least K values >= t
        const unsigned long long c = t | (1ull << bit);
        int n = 0;
#pragma unroll
        for (int j = 0; j < WIDE_REGS; ++j) n += __popcll(__ballot(v[j] >= c));
        if (n >= K) t = c;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const unsigned long long below = (1ull << lane) - 1ull;
    int at = 0;
#pragma unroll
    for (int j = 0; j < WIDE_REGS; ++j) {
        const bool keep = v[j] >= t;
        const unsigned long long b = __ballot(keep);
        if (keep) buf[at + __popcll(b & below)] = v[j];
        at += __popcll(b);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return t;
}

constexpr int ivf_pq_scan_wide_lds_bytes(int lut) { return PQ_NT * (lut == 0 ? 4 : 2) + 4 * WIDE_CAP * 8 + 16; }
template <int DSUB, int LUT>
__global__ __launch_bounds__(256) void ivf_pq_scan_wide_kernel(const float* __restrict__ Q, const int* __restrict__ qmap,
                                                               const int* __restrict__ plist, const float* __restrict__ coarse,
                                                               const float* __restrict__ pq, const unsigned char* __restrict__ codes,
                                                               const int* __restrict__ off, const int* __restrict__ ids, int parts, int K,
                                                               float* __restrict__ pk, int* __restrict__ pi) {
    constexpr int TABLE_FLOATS = LUT == 0 ? PQ_NT : PQ_NT / 2;
    extern __shared__ __attribute__((aligned(16))) float lds_wide[];  // table, then [4][WIDE_CAP] u64 (over the residual), [4] counts
    ivf_lut_t<LUT>* lut = (ivf_lut_t<LUT>*)lds_wide;
    unsigned long long* cbuf = (unsigned long long*)(lds_wide + TABLE_FLOATS);
    int* wcnt = (int*)(cbuf + 4 * WIDE_CAP);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t pos = blockIdx.x;
    const int part = blockIdx.y;
    // the residual is dead after the prologue: its place is the buffers'
    const IvfScanTask t = ivf_scan_prologue<DSUB, LUT>(lut, lds_wide + TABLE_FLOATS, Q, qmap, plist, coarse, pq, off, parts);
    const int o0 = t.o0, r1 = t.r1;
    unsigned long long* buf = cbuf + wave * WIDE_CAP;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long thr = 0ull;                                // a candidate must beat it (0: nothing yet)
    float thr_key = -INFINITY;
    int cnt = 0;
    IvfRowCodes next;
    if (t.r0 + tid < r1) next.load(codes, o0 + t.r0 + tid);
    for (int rb = t.r0; rb < r1; rb += 256) {                     // a uniform trip count: the wave's count stays wave-uniform
        const int r = rb + tid;
        const IvfRowCodes cur = next;
        if (r + 256 < r1) next.load(codes, o0 + r + 256);
        const float key = ivf_row_key<LUT>(lut, cur);
        unsigned long long p = 0ull;
        if (r < r1 && key >= thr_key) p = ivf_pack(key, ids[o0 + r]);     // equal distances: the ids decide, below
        const bool take = p > thr;
        const unsigned long long b = __ballot(take);
        if (b != 0ull) {
            const int na = __popcll(b);
            if (cnt + na > WIDE_CAP) {                            // cnt > WIDE_CAP - 64 >= K: prune, then K + na <= WIDE_CAP
                thr = ivf_wide_prune(buf, cnt, K, lane);
                thr_key = ivf_unpack_key(thr);
                cnt = K;
            }
            if (take) buf[cnt + __popcll(b & below)] = p;         // (one that no longer beats the new threshold falls at the next prune)
            cnt += na;
        }
    }
    cnt = __builtin_amdgcn_readfirstlane(cnt);
    if (cnt > K) { ivf_wide_prune(buf, cnt, K, lane); cnt = K; }
    if (lane == 0) wcnt[wave] = cnt;
    __syncthreads();
    // the 4 x (<= K) wave results ranked by counting (distinct values): rank < K goes out, the rest of the K slots is padding
    const int c0 = wcnt[0], c1 = wcnt[1], c2 = wcnt[2], c3 = wcnt[3];
    const int total = c0 + c1 + c2 + c3;
    const int64_t o = (pos * parts + part) * K;
    unsigned long long mine[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {                                 // slot s = wave (s / 128), entry (s % 128)
        const int s = tid + 256 * j, ws = s >> 7, is = s & 127;
        mine[j] = is < wcnt[ws] ? cbuf[ws * WIDE_CAP + is] : 0ull;
    }
    int rank0 = 0, rank1 = 0;
    for (int w2 = 0; w2 < 4; ++w2) {
        const int cw = w2 == 0 ? c0 : w2 == 1 ? c1 : w2 == 2 ? c2 : c3;
        const unsigned long long* bw = cbuf + w2 * WIDE_CAP;
        for (int i = 0; i < cw; ++i) { const unsigned long long u = bw[i]; rank0 += u > mine[0] ? 1 : 0; rank1 += u > mine[1] ? 1 : 0; }
    }
    if (mine[0] != 0ull && rank0 < K) { pk[o + rank0] = ivf_unpack_key(mine[0]); pi[o + rank0] = ivf_unpack_id(mine[0]); }
    if (mine[1] != 0ull && rank1 < K) { pk[o + rank1] = ivf_unpack_key(mine[1]); pi[o + rank1] = ivf_unpack_id(mine[1]); }
    if (tid < K && tid >= total) { pk[o + tid] = -INFINITY; pi[o + tid] = -1; }
}

// out = x - decode(codes): the second-level residuals the refine quantizer is trained on and encodes
__global__ __launch_bounds__(256) void ivf_pq_residual2_kernel(const float* __restrict__ x, int64_t n, int dim, int dsub,
                                                               const float* __restrict__ pq, const unsigned char* __restrict__ codes,
                                                               float* __restrict__ out) {
    const int64_t e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= n * dim) return;
    const int64_t i = e / dim;
    const int dd = (int)(e - i * dim), m = dd / dsub, u = dd - m * dsub;
    out[e] = x[e] - pq[((int64_t)m * PQ_KS + codes[i * PQ_M + m]) * dsub + u];
}

constexpr int RF_M = 4;                     // refine sub-quantizers
constexpr int RF_KS = 16;                   // codewords each (4 bits)

// per row and refine sub-space the nearest of 16 codewords (equal distances: the smaller code); DR = dim / 4 = 16 / 32 / 64.
// packed: 2 bytes per row (c0 | c1 << 4, c2 | c3 << 4); else 4 bytes, one code each (the k-means bucketing's keys)
template <int DR>
__global__ __launch_bounds__(256) void ivf_refine_encode_kernel(const float* __restrict__ x, int64_t n, const float* __restrict__ refine,
                                                                int packed, unsigned char* __restrict__ out) {
    constexpr int D = RF_M * DR;
    __shared__ __attribute__((aligned(16))) float cb[RF_M * RF_KS * DR];
    const int tid = threadIdx.x;
    for (int e = tid; e < RF_M * RF_KS * DR; e += 256) cb[e] = refine[e];
    __syncthreads();
    const int64_t i = blockIdx.x * 256ll + tid;
    if (i >= n) return;
    const float4* xr = (const float4*)(x + i * D);
    unsigned code[RF_M];
#pragma unroll
    for (int mr = 0; mr < RF_M; ++mr) {
        float s[RF_KS];
#pragma unroll
        for (int j = 0; j < RF_KS; ++j) s[j] = 0.f;
        const float* c = cb + mr * RF_KS * DR;
#pragma unroll 2
        for (int u4 = 0; u4 < DR / 4; ++u4) {
            const float4 v = xr[mr * (DR / 4) + u4];
            const float xv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int a = 0; a < 4; ++a) {
#pragma unroll
                for (int j = 0; j < RF_KS; ++j) { const float t = xv[a] - c[j * DR + u4 * 4 + a]; s[j] += t * t; }
            }
        }
        float best = s[0];
        unsigned bj = 0;
#pragma unroll
        for (int j = 1; j < RF_KS; ++j)
            if (s[j] < best) { best = s[j]; bj = j; }
        code[mr] = bj;
    }
    if (packed) {
        out[i * 2] = (unsigned char)(code[0] | (code[1] << 4));
        out[i * 2 + 1] = (unsigned char)(code[2] | (code[3] << 4));
    } else {
#pragma unroll
        for (int mr = 0; mr < RF_M; ++mr) out[i * RF_M + mr] = (unsigned char)code[mr];
    }
}

// one workgroup per query, one thread per first-stage candidate: its list, PQ code and refine code are gathered (insertion
// order arrays), the row is reconstructed and the distance summed in fp32 with the dimension ascending; then the k1 packed
// (distance, id) values are ranked by counting (equal values, i.e. a candidate named twice: the earlier slot first)
template <int DSUB>
__global__ __launch_bounds__(WIDE_KMAX) void ivf_pqr_rerank_kernel(const float* __restrict__ Q, const int* __restrict__ cand, int k1,
                                                                   const float* __restrict__ coarse, const int* __restrict__ assign,
                                                                   const float* __restrict__ pq, const unsigned char* __restrict__ codes,
                                                                   const float* __restrict__ refine, const unsigned char* __restrict__ rcodes,
                                                                   int64_t n_rows, int k, float* __restrict__ out_dist, int* __restrict__ out_ids) {
    constexpr int D = PQ_M * DSUB, DR = D / RF_M;
    __shared__ float qs[D];
    __shared__ float rf[RF_M * RF_KS * DR];
    __shared__ unsigned long long cv[WIDE_KMAX];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    for (int dd = tid; dd < D; dd += WIDE_KMAX) qs[dd] = Q[q * D + dd];
    for (int e = tid; e < RF_M * RF_KS * DR; e += WIDE_KMAX) rf[e] = refine[e];
    __syncthreads();
    unsigned long long v = 0ull;
    const int id = tid < k1 ? cand[q * k1 + tid] : -1;
    if (id >= 0 && id < n_rows) {
        const float* cr = coarse + (int64_t)assign[id] * D;
        IvfRowCodes row;
        row.load(codes, id);
        const unsigned rc = (unsigned)rcodes[(int64_t)id * 2] | ((unsigned)rcodes[(int64_t)id * 2 + 1] << 8);
        float s = 0.f;
#pragma unroll
        for (int m = 0; m < PQ_M; ++m) {
            const float* pc = pq + ((int64_t)m * PQ_KS + row.code(m)) * DSUB;
            const int mr = m >> 4;                                // DR = 16 * DSUB: 16 PQ sub-spaces per refine sub-space
            const float* rp = rf + (mr * RF_KS + ((rc >> (4 * mr)) & 15u)) * DR + (m & 15) * DSUB;
#pragma unroll
            for (int u = 0; u < DSUB; ++u) {
                const float rec = (cr[m * DSUB + u] + pc[u]) + rp[u];
                const float t = qs[m * DSUB + u] - rec;
                s += t * t;
            }
        }
        v = ivf_pack(-s, id);
    }
    cv[tid] = v;
    __syncthreads();
    int rank = 0, filled = 0;
    for (int i = 0; i < k1; ++i) {
        const unsigned long long u = cv[i];
        rank += (u > v || (u == v && i < tid)) ? 1 : 0;
        filled += u != 0ull ? 1 : 0;
    }
    if (v != 0ull && rank < k) { out_dist[q * k + rank] = -ivf_unpack_key(v); out_ids[q * k + rank] = ivf_unpack_id(v); }
    if (tid < k && tid >= filled) { out_dist[q * k + tid] = INFINITY; out_ids[q * k + tid] = -1; }
}

// one wave per query: the np x slots x K partial results of its probes -> k_out results.  mode 0 (flat): keys are
// q.x - |x|^2/2 with list-relative row ids (mapped through row_ids); mode 1 (PQ): keys are -distance with global ids.
__global__ __launch_bounds__(64) void ivf_merge_kernel(const float* __restrict__ pk, const int* __restrict__ pi,
                                                       const int* __restrict__ inv, const int* __restrict__ probe, int np, int slotsK,
                                                       const int* __restrict__ row_ids, const int* __restrict__ row_off,
                                                       const float* __restrict__ Q, int D, int mode, float* __restrict__ out_dist,
                                                       int* __restrict__ out_ids, int k_out) {
    extern __shared__ unsigned long long cand[];
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const int M = np * slotsK;
    for (int i = lane; i < M; i += 64) {
        const int p = i / slotsK, s = i - p * slotsK;
        const int64_t e = q * np + p;
        const int64_t o = (int64_t)inv[e] * slotsK + s;
        int gid = pi[o];
        if (gid >= 0 && mode == 0) gid = row_ids[row_off[probe[e]] + gid];
        cand[i] = gid >= 0 ? ivf_pack(pk[o], gid) : 0ull;
    }
    float qq = 0.f;
    if (mode == 0) {
        for (int c = lane; c < D; c += 64) { const float v = Q[q * D + c]; qq += v * v; }
        qq = wave_sum(qq);
    }
    __syncthreads();
    for (int j = 0; j < k_out; ++j) {
        unsigned long long best = 0ull; int bi = -1;
        for (int i = lane; i < M; i += 64)
            if (cand[i] > best) { best = cand[i]; bi = i; }
#pragma unroll
        for (int s2 = 32; s2 > 0; s2 >>= 1) {
            const unsigned long long ob = __shfl_xor(best, s2, 64);
            const int oi = __shfl_xor(bi, s2, 64);
            if (ob > best) { best = ob; bi = oi; }
        }
        if (lane == 0) {
            if (best == 0ull) { out_ids[q * k_out + j] = -1; out_dist[q * k_out + j] = INFINITY; }
            else {
                const float key = ivf_unpack_key(best);
                out_ids[q * k_out + j] = ivf_unpack_id(best);
                out_dist[q * k_out + j] = mode == 0 ? fmaxf(qq - 2.f * key, 0.f) : -key;
                cand[bi] = 0ull;
            }
        }
        __syncthreads();
    }
}

static bool ivf_dim_ok(int dim) { return dim == 64 || dim == 128 || dim == 256; }

// The one dispatch of a run-time size onto the compiled ones: f(std::integral_constant<int, DSUB>) for dsub = dim / 64 in
// 1, 2, 4 (the caller has checked ivf_dim_ok), and a choice between two (K = 20 / 32, lut = 0 / 1) to nest inside it.
template <int V> using ivf_const = std::integral_constant<int, V>;
template <typename F>
static void ivf_with_dsub(int dim, F&& f) {
    switch (dim / PQ_M) {
        case 1: f(ivf_const<1>{}); break;
        case 2: f(ivf_const<2>{}); break;
        default: f(ivf_const<4>{}); break;
    }
}
template <int A, int B, typename F>
static void ivf_with_either(bool first, F&& f) { if (first) f(ivf_const<A>{}); else f(ivf_const<B>{}); }
static int ivf_nbits(int nb) { int b = 0; while ((1 << b) < nb) ++b; return b; }
static int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

// parts per list of a search: enough workgroups for the chip when few queries probe, within the merge's candidate budget
static int ivf_parts(int64_t n_pairs, int np, int K, int kind) {
    const int slots_per_part = kind == 0 ? 2 : 1;
    const int64_t cap = std::max<int64_t>(1, IVF_MAX_CANDS / ((int64_t)np * slots_per_part * K));
    const int64_t base = kind == 0 ? (n_pairs + 127) / 128 : n_pairs;
    const int64_t want = base > 0 ? (2048 + base - 1) / base : 1;
    return (int)std::max<int64_t>(1, std::min(cap, want));
}

struct IvfSearchLayout {
    int np, K, parts, slotsK;
    int64_t n_pairs, bucket_ws;
    int64_t o_probe, o_pair_off, o_sorted, o_qmap, o_plist, o_inv, o_qblk, o_pk, o_pi, o_bucket, total;
};

}  // namespace nafp

using namespace nafp;

extern "C" int64_t nafp_ivf_bucket_workspace_bytes(int64_t n, int n_buckets, int batch) {
    if (n < 0 || n >= ((int64_t)1 << 31) || n_buckets <= 0 || n_buckets > IVF_MAX_BUCKETS || batch <= 0) return -1;
    const int64_t n_tiles = std::max<int64_t>(1, (n + BUCKET_TILE - 1) / BUCKET_TILE);
    return align256((int64_t)batch * n_tiles * n_buckets * 4) + align256((int64_t)batch * n_buckets * 4) + 256;
}

extern "C" int nafp_ivf_bucket(const void* keys, int key_bytes, int64_t n, int n_buckets, int batch, int32_t* offsets, int32_t* ids,
                               void* workspace, int64_t workspace_bytes, void* stream) {
    if (!keys || !offsets || !ids || !workspace || n < 0 || n_buckets <= 0 || batch <= 0) return NAFP_ERR_INVALID_ARG;
    if ((key_bytes != 1 && key_bytes != 4) || n_buckets > IVF_MAX_BUCKETS || n >= ((int64_t)1 << 31)) return NAFP_ERR_UNSUPPORTED;
    if (workspace_bytes < nafp_ivf_bucket_workspace_bytes(n, n_buckets, batch)) return NAFP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int n_tiles = (int)std::max<int64_t>(1, (n + BUCKET_TILE - 1) / BUCKET_TILE);
    char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    int* tc = (int*)ws;
    int* totals = (int*)(ws + align256((int64_t)batch * n_tiles * n_buckets * 4));
    const dim3 grid((unsigned)n_tiles, (unsigned)batch);
    const int lds = n_buckets * 4, nbits = ivf_nbits(n_buckets);
    if (key_bytes == 1) ivf_bucket_count_kernel<unsigned char><<<grid, 64, lds, st>>>((const unsigned char*)keys, n, n_buckets, batch, tc, n_tiles);
    else                ivf_bucket_count_kernel<int><<<grid, 64, lds, st>>>((const int*)keys, n, n_buckets, batch, tc, n_tiles);
    NAFP_LAUNCH_CHECK();
    ivf_bucket_scan_tiles_kernel<<<dim3((unsigned)((n_buckets + 255) / 256), (unsigned)batch), 256, 0, st>>>(tc, n_tiles, n_buckets, totals);
    NAFP_LAUNCH_CHECK();
    ivf_bucket_offsets_kernel<<<(unsigned)batch, 256, 0, st>>>(totals, n_buckets, offsets);
    NAFP_LAUNCH_CHECK();
    if (key_bytes == 1) ivf_bucket_scatter_kernel<unsigned char><<<grid, 64, lds, st>>>((const unsigned char*)keys, n, n_buckets, batch, tc, offsets, ids, n_tiles, nbits);
    else                ivf_bucket_scatter_kernel<int><<<grid, 64, lds, st>>>((const int*)keys, n, n_buckets, batch, tc, offsets, ids, n_tiles, nbits);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int nafp_ivf_kmeans_update(const float* x, int64_t n, int dim, int batch, const int32_t* offsets, const int32_t* ids,
                                      int n_buckets, float* centroids, int32_t* counts, void* stream) {
    if (!x || !offsets || !ids || !centroids || !counts || n <= 0 || dim <= 0 || batch <= 0 || n_buckets <= 0) return NAFP_ERR_INVALID_ARG;
    if (dim % batch || n_buckets > IVF_MAX_BUCKETS || n >= ((int64_t)1 << 31)) return NAFP_ERR_UNSUPPORTED;
    ivf_kmeans_update_kernel<<<dim3((unsigned)n_buckets, (unsigned)batch), 64, 0, (hipStream_t)stream>>>(
        x, n, dim, dim / batch, offsets, ids, n_buckets, centroids, counts);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int nafp_ivf_residuals(const float* x, int64_t n, int dim, const int32_t* assign, const float* centroids, float* out,
                                  void* stream) {
    if (!x || !assign || !centroids || !out || n < 0) return NAFP_ERR_INVALID_ARG;
    if (!ivf_dim_ok(dim)) return NAFP_ERR_UNSUPPORTED;
    if (n == 0) return NAFP_OK;
    ivf_residual_kernel<<<(unsigned)((n * dim + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, n, dim, assign, centroids, out);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int nafp_ivf_pq_encode(const float* x, int64_t n, int dim, const int32_t* assign, const float* coarse,
                                  const float* pq_centroids, int M, uint8_t* codes, void* stream) {
    if (!x || !pq_centroids || !codes || n < 0 || (!assign) != (!coarse)) return NAFP_ERR_INVALID_ARG;
    if (!ivf_dim_ok(dim) || M != PQ_M || n >= ((int64_t)1 << 31)) return NAFP_ERR_UNSUPPORTED;
    if (n == 0) return NAFP_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)(dim / M));     // 64 / dsub sub-spaces per workgroup
    ivf_with_dsub(dim, [&](auto ds) { ivf_pq_encode_kernel<ds()><<<grid, 256, 0, st>>>(x, n, assign, coarse, pq_centroids, codes); });
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int nafp_ivf_probe(const float* query, int64_t n_query, const float* centroids, int nlist, int dim, int nprobe,
                              int32_t* probe, void* stream) {
    if (!query || !centroids || !probe || n_query < 0 || nlist <= 0 || nprobe <= 0) return NAFP_ERR_INVALID_ARG;
    if (!ivf_dim_ok(dim) || nprobe > 128 || nprobe > nlist || nlist > IVF_MAX_BUCKETS || n_query > (1 << 30)) return NAFP_ERR_UNSUPPORTED;
    if (n_query == 0) return NAFP_OK;
    const int lds = (dim + nlist) * 4;
    NAFP_HIP_CHECK(hipFuncSetAttribute((const void*)ivf_probe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    ivf_probe_kernel<<<(unsigned)n_query, 256, lds, (hipStream_t)stream>>>(query, centroids, nlist, dim, nprobe, probe);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int64_t nafp_ivf_flat_rows_bound(int64_t n, int nlist) {
    if (n < 0 || nlist <= 0) return -1;
    return n + 63ll * nlist;
}

extern "C" int nafp_ivf_flat_lists(const float* x, int64_t n, int dim, const int32_t* offsets, const int32_t* ids, int nlist,
                                   int32_t* row_offsets, float* rows, float* half_norms, int32_t* row_ids, void* stream) {
    if (!x || !offsets || !ids || !row_offsets || !rows || !half_norms || !row_ids || n <= 0 || nlist <= 0) return NAFP_ERR_INVALID_ARG;
    if (!ivf_dim_ok(dim) || nlist > IVF_MAX_BUCKETS || nafp_ivf_flat_rows_bound(n, nlist) >= ((int64_t)1 << 31)) return NAFP_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    ivf_padded_offsets_kernel<<<1, 64, 0, st>>>(offsets, nlist, row_offsets);
    NAFP_LAUNCH_CHECK();
    const int64_t bound = nafp_ivf_flat_rows_bound(n, nlist);
    ivf_flat_lists_kernel<<<(unsigned)((bound + 255) / 256), 256, 0, st>>>(x, dim, offsets, ids, nlist, row_offsets, bound, rows,
                                                                           half_norms, row_ids);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int nafp_ivf_pq_lists(const uint8_t* codes, int64_t n, int M, const int32_t* ids, uint8_t* codes_sorted, void* stream) {
    if (!codes || !ids || !codes_sorted || n < 0) return NAFP_ERR_INVALID_ARG;
    if (M != PQ_M || n >= ((int64_t)1 << 31)) return NAFP_ERR_UNSUPPORTED;
    if (n == 0) return NAFP_OK;
    ivf_gather_codes_kernel<<<(unsigned)((n * 4 + 255) / 256), 256, 0, (hipStream_t)stream>>>((const uint4*)codes, ids, n, (uint4*)codes_sorted);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

// wide: the IVFPQ-RR first stage (kind 1 only), k <= 128 kept as it is; otherwise k <= 32 in the two compiled sizes
static bool ivf_search_layout(int64_t n_query, int nlist, int nprobe, int k, int kind, IvfSearchLayout* L, bool wide = false) {
    if (n_query < 0 || n_query > (1 << 30) || nlist <= 0 || nlist > IVF_MAX_BUCKETS || nprobe <= 0 || nprobe > 128 || k <= 0 ||
        k > (wide ? WIDE_KMAX : 32) || (kind != 0 && kind != 1) || (wide && kind != 1))
        return false;
    L->np = std::min(nprobe, nlist);
    L->K = wide ? k : k <= 20 ? 20 : 32;
    L->n_pairs = n_query * L->np;
    if (L->n_pairs >= ((int64_t)1 << 31)) return false;
    L->parts = ivf_parts(L->n_pairs, L->np, L->K, kind);
    L->slotsK = (kind == 0 ? 2 : 1) * L->parts * L->K;
    L->bucket_ws = nafp_ivf_bucket_workspace_bytes(L->n_pairs, nlist, 1);
    int64_t at = 0;
    auto take = [&](int64_t bytes) { const int64_t o = at; at += align256(bytes); return o; };
    L->o_probe = take(L->n_pairs * 4);
    L->o_pair_off = take((int64_t)(nlist + 1) * 4);
    L->o_sorted = take(L->n_pairs * 4);
    L->o_qmap = take(L->n_pairs * 4);
    L->o_plist = take(L->n_pairs * 4);
    L->o_inv = take(L->n_pairs * 4);
    L->o_qblk = take((int64_t)(nlist + 1) * 4);
    L->o_pk = take(L->n_pairs * L->slotsK * 4);
    L->o_pi = take(L->n_pairs * L->slotsK * 4);
    L->o_bucket = take(L->bucket_ws);
    L->total = at + 256;
    return true;
}

extern "C" int64_t nafp_ivf_search_workspace_bytes(int64_t n_query, int nlist, int nprobe, int k, int kind) {
    IvfSearchLayout L;
    return ivf_search_layout(n_query, nlist, nprobe, k, kind, &L) ? L.total : -1;
}

// probe, group the (query, probe) pairs by list; returns the workspace base
static int ivf_search_front(const float* query, int64_t n_query, const float* centroids, int nlist, int dim, const IvfSearchLayout& L,
                            char* ws, hipStream_t st) {
    int rc = nafp_ivf_probe(query, n_query, centroids, nlist, dim, L.np, (int*)(ws + L.o_probe), st);
    if (rc != NAFP_OK) return rc;
    rc = nafp_ivf_bucket(ws + L.o_probe, 4, L.n_pairs, nlist, 1, (int*)(ws + L.o_pair_off), (int*)(ws + L.o_sorted), ws + L.o_bucket,
                         L.bucket_ws, st);
    if (rc != NAFP_OK) return rc;
    ivf_pairs_kernel<<<(unsigned)((L.n_pairs + 255) / 256), 256, 0, st>>>((const int*)(ws + L.o_sorted), (const int*)(ws + L.o_probe),
                                                                          L.n_pairs, L.np, (int*)(ws + L.o_qmap), (int*)(ws + L.o_plist),
                                                                          (int*)(ws + L.o_inv));
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

static int ivf_search_merge(const IvfSearchLayout& L, char* ws, int64_t n_query, const int32_t* row_ids, const int32_t* row_off,
                            const float* query, int dim, int mode, float* out_dist, int32_t* out_ids, int k, hipStream_t st) {
    const int lds = L.np * L.slotsK * 8;
    NAFP_HIP_CHECK(hipFuncSetAttribute((const void*)ivf_merge_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    ivf_merge_kernel<<<(unsigned)n_query, 64, lds, st>>>((const float*)(ws + L.o_pk), (const int*)(ws + L.o_pi), (const int*)(ws + L.o_inv),
                                                         (const int*)(ws + L.o_probe), L.np, L.slotsK, row_ids, row_off, query, dim, mode,
                                                         out_dist, out_ids, k);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int nafp_ivf_flat_search(const float* query, int64_t n_query, const float* centroids, int nlist, int dim, int nprobe,
                                    const float* rows, const float* half_norms, const int32_t* row_offsets, const int32_t* row_ids,
                                    int k, float* out_dist, int32_t* out_ids, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!query || !centroids || !rows || !half_norms || !row_offsets || !row_ids || !out_dist || !out_ids || !workspace || n_query < 0 ||
        nlist <= 0 || nprobe <= 0 || k <= 0)
        return NAFP_ERR_INVALID_ARG;
    IvfSearchLayout L;
    if (!ivf_dim_ok(dim) || !ivf_search_layout(n_query, nlist, nprobe, k, 0, &L)) return NAFP_ERR_UNSUPPORTED;
    if (n_query == 0) return NAFP_OK;
    if (workspace_bytes < L.total) return NAFP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    int rc = ivf_search_front(query, n_query, centroids, nlist, dim, L, ws, st);
    if (rc != NAFP_OK) return rc;
    ivf_qblock_prefix_kernel<<<1, 64, 0, st>>>((const int*)(ws + L.o_pair_off), nlist, (int*)(ws + L.o_qblk));
    NAFP_LAUNCH_CHECK();
    const unsigned grid_x = (unsigned)((L.n_pairs + 127) / 128 + nlist);        // >= the number of (list, query block) tasks
    rc = ivf_flat_scan_launch(dim, L.K, grid_x, L.parts, query, (const int*)(ws + L.o_qmap), (const int*)(ws + L.o_pair_off),
                              (const int*)(ws + L.o_qblk), nlist, rows, half_norms, row_offsets, (float*)(ws + L.o_pk),
                              (int*)(ws + L.o_pi), st);
    if (rc != NAFP_OK) return rc;
    return ivf_search_merge(L, ws, n_query, row_ids, row_offsets, query, dim, 0, out_dist, out_ids, k, st);
}

static bool ivf_lut_ok(int lut) { return lut == NAFP_IVF_LUT_F32 || lut == NAFP_IVF_LUT_F16; }

// The IVF-PQ search, k <= 32 through the two narrow scans or (wide) k <= 128 through the wide one: checks, layout, probe and
// pair grouping, the scan of the (pair, part) grid into the partial lists, the merge.
static int ivf_pq_search_run(bool wide, const float* query, int64_t n_query, const float* centroids, int nlist, int dim, int nprobe,
                             const float* pq_centroids, int M, const uint8_t* codes_sorted, const int32_t* offsets, const int32_t* ids,
                             int k, float* out_dist, int32_t* out_ids, int lut, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!query || !centroids || !pq_centroids || !codes_sorted || !offsets || !ids || !out_dist || !out_ids || !workspace ||
        n_query < 0 || nlist <= 0 || nprobe <= 0 || k <= 0)
        return NAFP_ERR_INVALID_ARG;
    IvfSearchLayout L;
    if (!ivf_dim_ok(dim) || M != PQ_M || !ivf_lut_ok(lut) || !ivf_search_layout(n_query, nlist, nprobe, k, 1, &L, wide)) return NAFP_ERR_UNSUPPORTED;
    if (n_query == 0) return NAFP_OK;
    if (workspace_bytes < L.total) return NAFP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    int rc = ivf_search_front(query, n_query, centroids, nlist, dim, L, ws, st);
    if (rc != NAFP_OK) return rc;
    const bool f32 = lut == NAFP_IVF_LUT_F32;
    hipError_t err = hipSuccess;
    // the wide scan takes K at run time (k_arg), the narrow ones have it compiled in
    auto scan = [&](auto kernel, int lds, auto... k_arg) {
        err = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (err != hipSuccess) return;
        kernel<<<dim3((unsigned)L.n_pairs, (unsigned)L.parts), 256, lds, st>>>(
            query, (const int*)(ws + L.o_qmap), (const int*)(ws + L.o_plist), centroids, pq_centroids, codes_sorted, offsets, ids, L.parts,
            k_arg..., (float*)(ws + L.o_pk), (int*)(ws + L.o_pi));
    };
    ivf_with_dsub(dim, [&](auto ds) {
        if (wide)
            ivf_with_either<0, 1>(f32, [&](auto lt) { scan(ivf_pq_scan_wide_kernel<ds(), lt()>, ivf_pq_scan_wide_lds_bytes(lt()), L.K); });
        else
            ivf_with_either<20, 32>(L.K == 20, [&](auto kk) {
                if (f32) scan(ivf_pq_scan_kernel<ds(), kk()>, ivf_pq_scan_lds_bytes());
                else     scan(ivf_pq_scan_f16_kernel<ds(), kk()>, ivf_pq_scan_f16_lds_bytes(kk()));
            });
    });
    NAFP_HIP_CHECK(err);
    NAFP_LAUNCH_CHECK();
    return ivf_search_merge(L, ws, n_query, nullptr, nullptr, query, dim, 1, out_dist, out_ids, k, st);
}

extern "C" int nafp_ivf_pq_search_ex(const float* query, int64_t n_query, const float* centroids, int nlist, int dim, int nprobe,
                                     const float* pq_centroids, int M, const uint8_t* codes_sorted, const int32_t* offsets,
                                     const int32_t* ids, int k, float* out_dist, int32_t* out_ids, int lut, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
    return ivf_pq_search_run(false, query, n_query, centroids, nlist, dim, nprobe, pq_centroids, M, codes_sorted, offsets, ids, k, out_dist,
                             out_ids, lut, workspace, workspace_bytes, stream);
}

extern "C" int nafp_ivf_pq_search(const float* query, int64_t n_query, const float* centroids, int nlist, int dim, int nprobe,
                                  const float* pq_centroids, int M, const uint8_t* codes_sorted, const int32_t* offsets,
                                  const int32_t* ids, int k, float* out_dist, int32_t* out_ids, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
    return nafp_ivf_pq_search_ex(query, n_query, centroids, nlist, dim, nprobe, pq_centroids, M, codes_sorted, offsets, ids, k, out_dist,
                                 out_ids, NAFP_IVF_LUT_F32, workspace, workspace_bytes, stream);
}

extern "C" int nafp_ivf_pq_adc_tables(const float* query, int64_t n_query, const int32_t* pair_query, const int32_t* pair_list,
                                      int64_t n_pairs, const float* centroids, int nlist, int dim, const float* pq_centroids, int M, int lut,
                                      void* out, void* stream) {
    if (!query || !pair_query || !pair_list || !centroids || !pq_centroids || !out || n_query < 0 || n_pairs < 0 || nlist <= 0)
        return NAFP_ERR_INVALID_ARG;
    if (!ivf_dim_ok(dim) || M != PQ_M || !ivf_lut_ok(lut) || nlist > IVF_MAX_BUCKETS || n_query > (1 << 30) || n_pairs >= ((int64_t)1 << 31))
        return NAFP_ERR_UNSUPPORTED;
    if (n_pairs == 0) return NAFP_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)n_pairs;
    ivf_with_dsub(dim, [&](auto ds) {
        ivf_with_either<0, 1>(lut == NAFP_IVF_LUT_F32, [&](auto lt) {
            ivf_pq_adc_tables_kernel<ds(), lt()><<<grid, 256, 0, st>>>(query, n_query, pair_query, pair_list, centroids, nlist, pq_centroids, out);
        });
    });
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

// ---- IVFPQ-RR --------------------------------------------------------------------------------------------------------
static bool ivf_refine_ok(int dim, int m_refine, int nbits_refine) { return ivf_dim_ok(dim) && m_refine == RF_M && nbits_refine == 4; }

extern "C" int nafp_ivf_pq_residuals(const float* x, int64_t n, int dim, const float* pq_centroids, int M, const uint8_t* codes, float* out,
                                     void* stream) {
    if (!x || !pq_centroids || !codes || !out || n < 0) return NAFP_ERR_INVALID_ARG;
    if (!ivf_dim_ok(dim) || M != PQ_M || n >= ((int64_t)1 << 31)) return NAFP_ERR_UNSUPPORTED;
    if (n * dim >= ((int64_t)1 << 32)) return NAFP_ERR_UNSUPPORTED;              // one thread per element, fewer than 2^32 per launch
    if (n == 0) return NAFP_OK;
    ivf_pq_residual2_kernel<<<(unsigned)((n * dim + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, n, dim, dim / M, pq_centroids, codes, out);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int nafp_ivf_refine_encode(const float* x, int64_t n, int dim, const float* refine_centroids, int M_refine, int nbits_refine,
                                      int packed, uint8_t* codes, void* stream) {
    if (!x || !refine_centroids || !codes || n < 0) return NAFP_ERR_INVALID_ARG;
    if (!ivf_refine_ok(dim, M_refine, nbits_refine) || (packed != 0 && packed != 1) || n >= ((int64_t)1 << 31)) return NAFP_ERR_UNSUPPORTED;
    if (n == 0) return NAFP_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)((n + 255) / 256);
    ivf_with_dsub(dim, [&](auto ds) { ivf_refine_encode_kernel<16 * ds()><<<grid, 256, 0, st>>>(x, n, refine_centroids, packed, codes); });   // DR = d / 4
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int64_t nafp_ivf_pq_wide_workspace_bytes(int64_t n_query, int nlist, int nprobe, int k1) {
    IvfSearchLayout L;
    return ivf_search_layout(n_query, nlist, nprobe, k1, 1, &L, true) ? L.total : -1;
}

extern "C" int nafp_ivf_pq_search_wide(const float* query, int64_t n_query, const float* centroids, int nlist, int dim, int nprobe,
                                       const float* pq_centroids, int M, const uint8_t* codes_sorted, const int32_t* offsets,
                                       const int32_t* ids, int k1, float* out_dist, int32_t* out_ids, int lut, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
    return ivf_pq_search_run(true, query, n_query, centroids, nlist, dim, nprobe, pq_centroids, M, codes_sorted, offsets, ids, k1, out_dist,
                             out_ids, lut, workspace, workspace_bytes, stream);
}

extern "C" int nafp_ivf_pqr_rerank(const float* query, int64_t n_query, int dim, const int32_t* cand_ids, int k1, const float* centroids,
                                   const int32_t* assign, const float* pq_centroids, int M, const uint8_t* codes,
                                   const float* refine_centroids, int M_refine, int nbits_refine, const uint8_t* refine_codes,
                                   int64_t n_rows, int k, float* out_dist, int32_t* out_ids, void* stream) {
    if (!query || !cand_ids || !centroids || !assign || !pq_centroids || !codes || !refine_centroids || !refine_codes || !out_dist ||
        !out_ids || n_query < 0 || n_rows < 0 || k1 <= 0 || k <= 0)
        return NAFP_ERR_INVALID_ARG;
    if (!ivf_refine_ok(dim, M_refine, nbits_refine) || M != PQ_M || k1 > WIDE_KMAX || k > 32 || k > k1 || n_query > (1 << 30) ||
        n_rows >= ((int64_t)1 << 31))
        return NAFP_ERR_UNSUPPORTED;
    if (n_query == 0) return NAFP_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)n_query;
    ivf_with_dsub(dim, [&](auto ds) {
        ivf_pqr_rerank_kernel<ds()><<<grid, WIDE_KMAX, 0, st>>>(query, cand_ids, k1, centroids, assign, pq_centroids, codes, refine_centroids,
                                                                refine_codes, n_rows, k, out_dist, out_ids);
    });
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int nafp_ivf_pqr_search(const float* query, int64_t n_query, const float* centroids, int nlist, int dim, int nprobe,
                                   const float* pq_centroids, int M, const uint8_t* codes_sorted, const int32_t* offsets, const int32_t* ids,
                                   const int32_t* assign, const uint8_t* codes, const float* refine_centroids, int M_refine, int nbits_refine,
                                   const uint8_t* refine_codes, int64_t n_rows, int k, int k_factor, float* out_dist, int32_t* out_ids,
                                   float* stage1_dist, int32_t* stage1_ids, int lut, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!stage1_dist || !stage1_ids || !assign || !codes || !refine_centroids || !refine_codes || !out_dist || !out_ids || k <= 0 ||
        k_factor <= 0 || n_rows < 0)
        return NAFP_ERR_INVALID_ARG;
    if (k > 32 || k_factor > 4 || !ivf_refine_ok(dim, M_refine, nbits_refine)) return NAFP_ERR_UNSUPPORTED;
    const int k1 = k * k_factor;
    int rc = nafp_ivf_pq_search_wide(query, n_query, centroids, nlist, dim, nprobe, pq_centroids, M, codes_sorted, offsets, ids, k1,
                                     stage1_dist, stage1_ids, lut, workspace, workspace_bytes, stream);
    if (rc != NAFP_OK) return rc;
    return nafp_ivf_pqr_rerank(query, n_query, dim, stage1_ids, k1, centroids, assign, pq_centroids, M, codes, refine_centroids, M_refine,
                               nbits_refine, refine_codes, n_rows, k, out_dist, out_ids, stream);
}
