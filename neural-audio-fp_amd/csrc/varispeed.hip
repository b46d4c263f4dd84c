// Varispeed: exact integer resampling of model-rate int16 mono PCM by an arbitrary Q24 step (sigma = step / 2^24 in 0.8 .. 1.25), gfx950.
//
// Sits behind the ingest of a launch and in front of nafp_melspec_forward_windows_i16: a recording played a few percent fast or
// slow (tempo and pitch together) is brought back to the library's speed before it is fingerprinted.  nafp_resample_* / nafp_ingest_*
// are polyphase filters for rational rate pairs with a small numerator; an arbitrary step has none, so this pass interpolates
// linearly, in integers, between the rows of a table of 512 phases.
//
// Contract (include/nafp.h has it in full): hq[p][t] = round(2^30 h(p / 512 + W - 1 - t)), p = 0 .. 512, t = 0 .. T - 1, T = 2 W;
//     P = n step,  pos = P >> 24,  frac = P & (2^24 - 1),  p = frac >> 15,  w = frac & 32767
//     c_t = (hq[p][t] (32768 - w) + hq[p + 1][t] w + 16384) >> 15
//     acc = sum_t c_t x[pos - W + 1 + t]           (int64, exact; samples outside the file are zero)
//     y[n] = clamp((acc + 2^29) >> 30, -32768, 32767)
// An output sample is a pure function of (file samples, output index, step): integer sums have no order, so the bytes do not depend
// on how the outputs are cut into pieces, blocks or launches.  No floating point on the device.
//
// One workgroup computes 256 consecutive outputs of one piece: it stages the input span of the block in LDS as int32 once (at most
// 255 * 1.25 + 2 * 43 + 2 samples), then every lane walks the T taps of its two adjacent table rows.  The table (513 rows of up to
// 88 int32: 176 KB) stays in global memory, where it is read at scattered phases out of L2; a row's taps are contiguous and padded
// to a multiple of 4, rows p and p + 1 adjacent, so a lane reads both with 16-byte loads.  The padding taps are zero: they add nothing.
#include <math.h>

#include "nafp_common.h"

struct nafp_varispeed {
    uint32_t step;
    int W, T, Tp;              // Tp: the device row stride, T rounded up to a multiple of 4
    int32_t* d_tab;            // [513][Tp]
};

namespace nafp {

double bessel_i0(double x);                             // resample.hip

constexpr int VS_BLOCK = 256;
constexpr int VS_PHASES = 512;
constexpr int VS_SPAN_CAP = 416;                        // >= (255 * 1.25 -> 319) + 1 + 2 * 43 + 3 padding taps

struct VsGeom { int W, T; };

static int vs_geometry(uint32_t step, VsGeom* g) {
    if (step < NAFP_VARISPEED_STEP_MIN || step > NAFP_VARISPEED_STEP_MAX) return NAFP_ERR_UNSUPPORTED;
    // W = ceil(32 / (2 fc)), 2 fc = 0.95 min(1, 2^24 / step), in integers: 640 max(step, 2^24) / (19 * 2^24)
    const int64_t m = step > (1u << 24) ? (int64_t)step : (int64_t)1 << 24, den = (int64_t)19 << 24;
    const int W = (int)((640 * m + den - 1) / den);
    *g = VsGeom{W, 2 * W};
    return NAFP_OK;
}

// hq[p][t]
struct VsDesign {
    VsGeom g; double two_fc, inv_i0;
    VsDesign(const VsGeom& g_, uint32_t step) : g(g_) {
        two_fc = step > (1u << 24) ? 0.95 * 16777216.0 / (double)step : 0.95;
        inv_i0 = 1.0 / bessel_i0(8.6);
    }
    int32_t hq(int p, int t) const {
        const double u = (double)p / 512.0 + (double)(g.W - 1 - t);            // exact; |u| <= W
        const double x = M_PI * (two_fc * u);
        const double sinc = u == 0.0 ? 1.0 : sin(x) / x;
        const double r = u / (double)g.W;
        const double w = bessel_i0(8.6 * sqrt(fmax(0.0, 1.0 - r * r))) * inv_i0;
        return (int32_t)llround(sinc * w * two_fc * 1073741824.0);
    }
};

// the table of a step in the device layout [phase][Tp], Tp = T rounded up to a multiple of 4, the padding taps zero
static std::vector<int32_t> vs_device_table(const VsGeom& g, uint32_t step) {
    const VsDesign d(g, step);
    const int Tp = (g.T + 3) & ~3;
    std::vector<int32_t> tab((size_t)(VS_PHASES + 1) * Tp, 0);
    for (int p = 0; p <= VS_PHASES; ++p)
        for (int t = 0; t < g.T; ++t) tab[(size_t)p * Tp + t] = d.hq(p, t);
    return tab;
}

// samples [first, last) of a file of n_in samples that the outputs [n0, n1) touch (first == last: none)
__host__ __device__ inline void vs_input_range(int64_t n0, int64_t n1, int64_t n_in, uint32_t step, int W, int64_t* first, int64_t* last) {
    int64_t lo = ((n0 * step) >> 24) - W + 1;
    if (lo < 0) lo = 0;
    int64_t hi = n1 > n0 ? (((n1 - 1) * step) >> 24) + W + 1 : 0;
    if (hi > n_in) hi = n_in;
    if (hi <= lo) { lo = lo < n_in ? lo : n_in; hi = lo; }
    *first = lo; *last = hi;
}

// 0: consistent; 1: the output range is outside the arena (nothing may be written); 2: anything else (its outputs are zeroed)
__host__ __device__ inline int vs_piece_fault(const nafp_varispeed_piece& pc, uint32_t step, int W, int64_t src_samples, int64_t out_samples) {
    if (pc.n_out < 0 || pc.out_off < 0 || pc.out_off > out_samples || pc.n_out > out_samples - pc.out_off) return 1;
    if (pc.n_in < 0 || pc.n_in >= VS_MAX_IN || pc.out0 < 0 || pc.out0 > 2 * VS_MAX_IN) return 2;
    if (pc.frame0 < 0 || pc.frame0 > pc.n_in || pc.n_frames < 0 || pc.n_frames > pc.n_in - pc.frame0) return 2;
    if (pc.src_off < 0 || pc.src_off > src_samples || pc.n_frames > src_samples - pc.src_off) return 2;
    if (pc.out0 + pc.n_out > vs_n_out(pc.n_in, step)) return 2;
    int64_t lo, hi;
    vs_input_range(pc.out0, pc.out0 + pc.n_out, pc.n_in, step, W, &lo, &hi);
    if (hi > lo && (pc.frame0 > lo || pc.frame0 + pc.n_frames < hi)) return 2;      // a needed sample is not present
    return 0;
}

__global__ __launch_bounds__(VS_BLOCK) void varispeed_i16_kernel(const int32_t* __restrict__ tab, uint32_t step, int W, int Tp,
                                                                 const int16_t* __restrict__ src, int64_t src_samples,
                                                                 const nafp_varispeed_piece* __restrict__ pieces,
                                                                 int16_t* __restrict__ out, int64_t out_samples) {
    // x[jlo .. jlo + span), then the Tp - 2 W samples the padding taps meet (real samples: their coefficients are zero).  Staged as
    // int32, not int16: 1.7 KB either way, and the tap loop then multiplies straight out of LDS without a sign extension per tap
    __shared__ __attribute__((aligned(16))) int32_t s_in[VS_SPAN_CAP];
    const nafp_varispeed_piece pc = pieces[blockIdx.y];
    const int tid = threadIdx.x;
    const int fault = vs_piece_fault(pc, step, W, src_samples, out_samples);
    if (fault == 1) return;
    for (int64_t b0 = (int64_t)blockIdx.x * VS_BLOCK; b0 < pc.n_out; b0 += (int64_t)gridDim.x * VS_BLOCK) {
        const int cnt = (int)(pc.n_out - b0 < VS_BLOCK ? pc.n_out - b0 : VS_BLOCK);
        int16_t* o = out + pc.out_off + b0;                                // [0, cnt) is inside the arena (fault != 1)
        const int64_t na = pc.out0 + b0;
        const int64_t pos_a = (na * step) >> 24, pos_b = ((na + cnt - 1) * step) >> 24;
        const int64_t jlo = pos_a - W + 1;
        const int64_t fill = pos_b - pos_a + Tp;                           // span = pos_b - pos_a + 2 W, + the Tp - 2 W padding taps
        if (fault != 0 || fill > VS_SPAN_CAP) {
            if (tid < cnt) o[tid] = 0;
            continue;
        }
        __syncthreads();                                                   // the previous block's reads of s_in
        for (int i = tid; i < (int)fill; i += VS_BLOCK) {
            const int64_t k = jlo + i - pc.frame0;                         // index into the samples present
            int32_t v = 0;
            if (k >= 0 && k < pc.n_frames) v = src[pc.src_off + k];        // inside [src_off, src_off + n_frames) <= src_samples
            s_in[i] = v;
        }
        __syncthreads();
        if (tid < cnt) {
            const int64_t P = (na + tid) * step;
            const int frac = (int)(P & 0xffffff);
            const int p = frac >> 15, w = frac & 32767;
            const int4* ra = (const int4*)(tab + (int64_t)p * Tp);         // row p; row p + 1 <= 512 follows it
            const int4* rb = (const int4*)(tab + (int64_t)(p + 1) * Tp);
            const int32_t* sp = s_in + (int)((P >> 24) - pos_a);           // sp[t], t < Tp: inside [0, fill)
            const int64_t wa = 32768 - w, wb = w;
            int64_t acc = 0;
#pragma unroll 2
            for (int t4 = 0; t4 < (Tp >> 2); ++t4) {
                const int4 a = ra[t4], b = rb[t4];
                const int32_t* x = sp + 4 * t4;
                acc += (int64_t)(int32_t)((a.x * wa + b.x * wb + 16384) >> 15) * x[0];
                acc += (int64_t)(int32_t)((a.y * wa + b.y * wb + 16384) >> 15) * x[1];
                acc += (int64_t)(int32_t)((a.z * wa + b.z * wb + 16384) >> 15) * x[2];
                acc += (int64_t)(int32_t)((a.w * wa + b.w * wb + 16384) >> 15) * x[3];
            }
            int64_t y = (acc + ((int64_t)1 << 29)) >> 30;
            y = y < -32768 ? -32768 : (y > 32767 ? 32767 : y);
            o[tid] = (int16_t)y;
        }
    }
}

// the set's tables and slot list on the current device, once
int aug_speedset_upload(nafp_aug_speedset* set) {
    if (set->d_slots) return NAFP_OK;
    hipError_t e = hipMalloc((void**)&set->d_tabs, set->tabs_host.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(set->d_tabs, set->tabs_host.data(), set->tabs_host.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    VsSlot* d_slots = nullptr;
    if (e == hipSuccess) {
        for (int k = 0; k < set->n_steps; ++k) set->slots[k].tab = set->d_tabs + set->tab_off[k];
        e = hipMalloc((void**)&d_slots, sizeof(set->slots));
    }
    if (e == hipSuccess) e = hipMemcpy(d_slots, set->slots, sizeof(set->slots), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        if (d_slots) (void)hipFree(d_slots);
        if (set->d_tabs) (void)hipFree(set->d_tabs);
        set->d_tabs = nullptr;
        return NAFP_ERR_HIP;
    }
    set->d_slots = d_slots;
    std::vector<int32_t>().swap(set->tabs_host);
    return NAFP_OK;
}

}  // namespace nafp

using namespace nafp;

extern "C" int nafp_varispeed_geometry(uint32_t step, int* W, int* T) {
    VsGeom g;
    const int st = vs_geometry(step, &g);
    if (st != NAFP_OK) return st;
    if (W) *W = g.W;
    if (T) *T = g.T;
    return NAFP_OK;
}

extern "C" int nafp_varispeed_table_host(uint32_t step, int32_t* table_host) {
    VsGeom g;
    const int st = vs_geometry(step, &g);
    if (st != NAFP_OK) return st;
    if (!table_host) return NAFP_ERR_INVALID_ARG;
    const VsDesign d(g, step);
    for (int p = 0; p <= VS_PHASES; ++p)
        for (int t = 0; t < g.T; ++t) table_host[(int64_t)p * g.T + t] = d.hq(p, t);
    return NAFP_OK;
}

extern "C" int64_t nafp_varispeed_n_out(int64_t n_in, uint32_t step) {
    VsGeom g;
    if (n_in < 0 || n_in >= VS_MAX_IN || vs_geometry(step, &g) != NAFP_OK) return -1;
    return vs_n_out(n_in, step);
}

extern "C" int nafp_varispeed_input_range(int64_t n0, int64_t n1, int64_t n_in, uint32_t step, int64_t* first, int64_t* last) {
    VsGeom g;
    const int st = vs_geometry(step, &g);
    if (st != NAFP_OK) return st;
    if (!first || !last || n0 < 0 || n1 < n0 || n_in < 0) return NAFP_ERR_INVALID_ARG;
    if (n_in >= VS_MAX_IN || n1 > 2 * VS_MAX_IN) return NAFP_ERR_UNSUPPORTED;
    vs_input_range(n0, n1, n_in, step, g.W, first, last);
    return NAFP_OK;
}

extern "C" int nafp_varispeed_check_pieces_host(uint32_t step, const nafp_varispeed_piece* pieces_host, int64_t n_pieces, int64_t src_samples,
                                                int64_t out_samples) {
    VsGeom g;
    const int st = vs_geometry(step, &g);
    if (st != NAFP_OK) return st;
    if (n_pieces < 0 || src_samples < 0 || out_samples < 0 || (n_pieces > 0 && !pieces_host)) return NAFP_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n_pieces; ++i) {
        if (pieces_host[i].n_in >= VS_MAX_IN) return NAFP_ERR_UNSUPPORTED;
        if (vs_piece_fault(pieces_host[i], step, g.W, src_samples, out_samples) != 0) return NAFP_ERR_INVALID_ARG;
    }
    return NAFP_OK;
}

extern "C" int nafp_varispeed_create(nafp_varispeed** plan, uint32_t step) {
    if (!plan) return NAFP_ERR_INVALID_ARG;
    *plan = nullptr;
    VsGeom g;
    const int st = vs_geometry(step, &g);
    if (st != NAFP_OK) return st;
    const int Tp = (g.T + 3) & ~3;
    const std::vector<int32_t> tab = vs_device_table(g, step);
    nafp_varispeed* h = new nafp_varispeed{step, g.W, g.T, Tp, nullptr};
    hipError_t e = hipMalloc((void**)&h->d_tab, tab.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(h->d_tab, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        if (h->d_tab) (void)hipFree(h->d_tab);
        delete h;
        return NAFP_ERR_HIP;
    }
    *plan = h;
    return NAFP_OK;
}

extern "C" int nafp_varispeed_destroy(nafp_varispeed* plan) {
    if (!plan) return NAFP_OK;
    if (plan->d_tab) (void)hipFree(plan->d_tab);
    delete plan;
    return NAFP_OK;
}

extern "C" int nafp_varispeed_i16(nafp_varispeed* plan, const int16_t* src, int64_t src_samples, const nafp_varispeed_piece* pieces_dev,
                                  int64_t n_pieces, int16_t* out, int64_t out_samples, void* stream) {
    if (!plan || !src || !out || n_pieces < 0 || src_samples < 0 || out_samples < 0 || (n_pieces > 0 && !pieces_dev))
        return NAFP_ERR_INVALID_ARG;
    if (n_pieces == 0 || out_samples == 0) return NAFP_OK;
    // blockIdx.y = piece; the blocks of a row stride over the piece's 256-output blocks, as nafp_resample_i16's do
    const int64_t blocks = (out_samples + VS_BLOCK - 1) / VS_BLOCK;
    for (int64_t p0 = 0; p0 < n_pieces; p0 += 32768) {
        const int64_t np = n_pieces - p0 < 32768 ? n_pieces - p0 : 32768;
        int64_t gx = 2 * ((blocks + n_pieces - 1) / n_pieces);
        gx = gx < 1 ? 1 : (gx > 8192 ? 8192 : gx);
        varispeed_i16_kernel<<<dim3((unsigned)gx, (unsigned)np), VS_BLOCK, 0, (hipStream_t)stream>>>(
            plan->d_tab, plan->step, plan->W, plan->Tp, src, src_samples, pieces_dev + p0, out, out_samples);
        NAFP_LAUNCH_CHECK();
    }
    return NAFP_OK;
}

extern "C" int nafp_aug_speedset_create(nafp_aug_speedset** set, const uint32_t* steps, int n_steps) {
    if (!set) return NAFP_ERR_INVALID_ARG;
    *set = nullptr;
    if (!steps || n_steps < 1 || n_steps > 32) return NAFP_ERR_INVALID_ARG;
    VsGeom g[32];
    for (int k = 0; k < n_steps; ++k) {
        const int st = vs_geometry(steps[k], &g[k]);
        if (st != NAFP_OK) return st;
    }
    nafp_aug_speedset* h = new nafp_aug_speedset();
    h->n_steps = n_steps;
    for (int k = 0; k < n_steps; ++k) {
        const std::vector<int32_t> tab = vs_device_table(g[k], steps[k]);
        h->tab_off[k] = (int64_t)h->tabs_host.size();                     // 513 Tp int32 each: every table starts 16-byte aligned
        h->tabs_host.insert(h->tabs_host.end(), tab.begin(), tab.end());
        h->slots[k] = VsSlot{nullptr, steps[k], g[k].W, (g[k].T + 3) & ~3, 0};
    }
    *set = h;
    return NAFP_OK;
}

extern "C" int nafp_aug_speedset_destroy(nafp_aug_speedset* set) {
    if (!set) return NAFP_OK;
    if (set->d_slots) (void)hipFree(set->d_slots);
    if (set->d_tabs) (void)hipFree(set->d_tabs);
    delete set;
    return NAFP_OK;
}
