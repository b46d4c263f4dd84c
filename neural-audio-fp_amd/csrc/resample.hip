// Exact integer resampling of int16 PCM (1 or 2 channels, any supported rate) to the model rate, gfx950.
//
// Sits between the PCM upload and nafp_melspec_forward_windows_i16: the reference accepts 8 kHz mono files only
// (model/utils/audio_utils.py:160-169 raises on any other rate) and leaves the conversion to an external tool.
//
// Contract (include/nafp.h has it in full): g = gcd(fs_in, fs_out), L = fs_out / g, M = fs_in / g; a Kaiser-windowed sinc
// hq[-half .. half] at the virtual rate fs_in * L, quantised to int32 with 30 fraction bits;
//     acc[n] = sum_j hq[n M - j L] * m[j]     (int64, exact; m = x or l + r; samples outside the file are zero)
//     y[n]   = clamp((acc[n] + 2^(s-1)) >> s, -32768, 32767),  s = 30 (mono) / 31 (stereo)
// An output sample is a pure function of (file samples, output index): integer sums have no order, so the bytes do not depend
// on how the outputs are cut into pieces, blocks or launches.  No floating point on the device.
//
// With c = n M + half, p = c mod L and jb = c div L the sum is  sum_t hq[p + t L - half] * m[jb - t],  t = 0 .. T-1: T taps of
// phase p.  One workgroup computes 256 consecutive outputs of one piece: it stages the (down-mixed) input span of the block in
// LDS as int32 once, then every lane walks its phase's taps.  The device table is [tap][phase]: the lanes of a wave sit at
// different phases of the SAME tap, so one step of a wave reads within one row of L int32 (L <= 320: at most 1280 B).
// The product is one v_mad_i64_i32 per tap.
#include <math.h>

#include "nafp_common.h"

struct nafp_resample {
    int fs_in, fs_out, L, M, half, T;
    int span_cap;              // LDS ints a block may need
    int32_t* d_tab;            // [T][L]
};

namespace nafp {

constexpr int RS_BLOCK = 256;
constexpr int64_t RS_MAX_INDEX = (int64_t)1 << 40;     // frames / outputs per file: n * M + half stays far inside int64

struct RsGeom { int L, M, half, T; };

static int rs_geometry(int fs_in, int fs_out, RsGeom* g) {
    if (fs_in <= 0 || fs_out <= 0) return NAFP_ERR_INVALID_ARG;
    int a = fs_in, b = fs_out;
    while (b) { const int r = a % b; a = b; b = r; }
    const int L = fs_out / a, M = fs_in / a;
    if (fs_in == fs_out) { *g = RsGeom{1, 1, 0, 1}; return NAFP_OK; }           // the channel average alone: hq = {2^30}
    if (fs_in < fs_out || L > 320 || fs_in > 192000) return NAFP_ERR_UNSUPPORTED;
    // half = ceil(32 fv / (2 fc)) with fc = 0.95 fs_out / 2, in integers: 32 fv / (0.95 fs_out) = 640 fv / (19 fs_out)
    const int64_t fv = (int64_t)fs_in * L, den = (int64_t)19 * fs_out;
    const int64_t half = (640 * fv + den - 1) / den;
    *g = RsGeom{L, M, (int)half, (int)((2 * half + 1 + L - 1) / L)};
    return NAFP_OK;
}

double bessel_i0(double x) {                         // (varispeed.hip uses it too) sum_k ((x/2)^k / k!)^2
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// hq[v], v in [-half, half] (0 outside)
struct RsDesign {
    RsGeom g; double r, gain, inv_i0;
    RsDesign(const RsGeom& g_, int fs_in, int fs_out) : g(g_) {
        r = 0.95 * (double)fs_out / ((double)fs_in * (double)g.L);       // 2 fc / fv
        gain = r * (double)g.L;
        inv_i0 = 1.0 / bessel_i0(8.6);
    }
    int32_t hq(int64_t v) const {
        if (v < -g.half || v > g.half) return 0;
        if (g.half == 0) return (int32_t)1 << 30;
        const double x = M_PI * (r * (double)v);
        const double sinc = v == 0 ? 1.0 : sin(x) / x;
        const double u = (double)v / (double)g.half;
        const double w = bessel_i0(8.6 * sqrt(fmax(0.0, 1.0 - u * u))) * inv_i0;
        return (int32_t)llround(sinc * w * gain * 1073741824.0);
    }
};

__host__ __device__ inline int64_t rs_floor_div(int64_t a, int64_t b) { int64_t q = a / b; if ((a % b != 0) && ((a < 0) != (b < 0))) --q; return q; }

// frames [first, last) of a file of n_in frames that the outputs [n0, n1) touch (first == last: none)
__host__ __device__ inline void rs_input_range(int64_t n0, int64_t n1, int64_t n_in, int L, int M, int half, int64_t* first, int64_t* last) {
    int64_t lo = -rs_floor_div(-(n0 * M - half), L);            // ceil
    if (lo < 0) lo = 0;
    int64_t hi = n1 > n0 ? rs_floor_div((n1 - 1) * M + half, L) + 1 : 0;
    if (hi > n_in) hi = n_in;
    if (hi <= lo) { lo = lo < n_in ? lo : n_in; hi = lo; }
    *first = lo; *last = hi;
}

// 0: consistent; 1: the output range is outside the arena (nothing may be written); 2: anything else (its outputs are zeroed)
__host__ __device__ inline int rs_piece_fault(const nafp_resample_piece& pc, int L, int M, int half, int64_t raw_samples, int64_t out_samples) {
    if (pc.n_out < 0 || pc.out_off < 0 || pc.out_off > out_samples || pc.n_out > out_samples - pc.out_off) return 1;
    if (pc.channels != 1 && pc.channels != 2) return 2;
    if (pc.n_in < 0 || pc.n_in > RS_MAX_INDEX || pc.out0 < 0 || pc.out0 > RS_MAX_INDEX) return 2;
    if (pc.frame0 < 0 || pc.frame0 > pc.n_in || pc.n_frames < 0 || pc.n_frames > pc.n_in - pc.frame0) return 2;
    if (pc.raw_off < 0 || pc.raw_off > raw_samples || pc.n_frames > (raw_samples - pc.raw_off) / pc.channels) return 2;
    const int64_t n_total = (pc.n_in * L + M - 1) / M;
    if (pc.out0 + pc.n_out > n_total) return 2;
    int64_t lo, hi;
    rs_input_range(pc.out0, pc.out0 + pc.n_out, pc.n_in, L, M, half, &lo, &hi);
    if (hi > lo && (pc.frame0 > lo || pc.frame0 + pc.n_frames < hi)) return 2;      // a needed frame was not uploaded
    return 0;
}

__global__ __launch_bounds__(RS_BLOCK) void resample_i16_kernel(const int32_t* __restrict__ tab, int L, int M, int half, int T, int span_cap,
                                                                const int16_t* __restrict__ raw, int64_t raw_samples,
                                                                const nafp_resample_piece* __restrict__ pieces,
                                                                int16_t* __restrict__ out, int64_t out_samples) {
    extern __shared__ __attribute__((aligned(16))) int32_t s_in[];         // m[jlo .. jlo + span)
    const nafp_resample_piece pc = pieces[blockIdx.y];
    const int tid = threadIdx.x;
    const int fault = rs_piece_fault(pc, L, M, half, raw_samples, out_samples);
    if (fault == 1) return;
    const int ch = pc.channels;
    const int shift = ch == 2 ? 31 : 30;
    for (int64_t b0 = (int64_t)blockIdx.x * RS_BLOCK; b0 < pc.n_out; b0 += (int64_t)gridDim.x * RS_BLOCK) {
        const int cnt = (int)(pc.n_out - b0 < RS_BLOCK ? pc.n_out - b0 : RS_BLOCK);
        int16_t* o = out + pc.out_off + b0;                                // [0, cnt) is inside the arena (fault != 1)
        const int64_t na = pc.out0 + b0;
        const int64_t jb_a = (na * M + half) / L, jb_b = ((na + cnt - 1) * M + half) / L;
        const int64_t jlo = jb_a - (T - 1);
        const int64_t span = jb_b - jlo + 1;
        if (fault != 0 || span > span_cap) {
            if (tid < cnt) o[tid] = 0;
            continue;
        }
        __syncthreads();                                                   // the previous block's reads of s_in
        for (int i = tid; i < (int)span; i += RS_BLOCK) {
            const int64_t k = jlo + i - pc.frame0;                         // index into the uploaded frames
            int32_t v = 0;
            if (k >= 0 && k < pc.n_frames) {                               // inside [raw_off, raw_off + n_frames * ch) <= raw_samples
                const int16_t* q = raw + pc.raw_off + k * ch;
                v = q[0];
                if (ch == 2) v += q[1];
            }
            s_in[i] = v;
        }
        __syncthreads();
        if (tid < cnt) {
            const int64_t c = (na + tid) * M + half;
            const int64_t jb = c / L;
            const int32_t* tp = tab + (int)(c - jb * L);                   // phase p; tp[t * L], t < T, stays inside [T][L]
            const int32_t* sp = s_in + (int)(jb - jlo);                    // sp[-t], t < T: [jb - jb_a, jb - jlo] inside [0, span)
            int64_t acc = 0;
#pragma unroll 4
            for (int t = 0; t < T; ++t) acc += (int64_t)tp[(int64_t)t * L] * (int64_t)sp[-t];
            int64_t y = (acc + ((int64_t)1 << (shift - 1))) >> shift;
            y = y < -32768 ? -32768 : (y > 32767 ? 32767 : y);
            o[tid] = (int16_t)y;
        }
    }
}

}  // namespace nafp

using namespace nafp;

extern "C" int nafp_resample_geometry(int fs_in, int fs_out, int* L, int* M, int* half, int* T) {
    RsGeom g;
    const int st = rs_geometry(fs_in, fs_out, &g);
    if (st != NAFP_OK) return st;
    if (L) *L = g.L;
    if (M) *M = g.M;
    if (half) *half = g.half;
    if (T) *T = g.T;
    return NAFP_OK;
}

extern "C" int nafp_resample_table_host(int fs_in, int fs_out, int32_t* table_host) {
    RsGeom g;
    const int st = rs_geometry(fs_in, fs_out, &g);
    if (st != NAFP_OK) return st;
    if (!table_host) return NAFP_ERR_INVALID_ARG;
    const RsDesign d(g, fs_in, fs_out);
    for (int p = 0; p < g.L; ++p)
        for (int t = 0; t < g.T; ++t) table_host[(int64_t)p * g.T + t] = d.hq((int64_t)p + (int64_t)t * g.L - g.half);
    return NAFP_OK;
}

extern "C" int64_t nafp_resample_n_out(int64_t n_in, int fs_in, int fs_out) {
    RsGeom g;
    if (n_in < 0 || n_in > RS_MAX_INDEX || rs_geometry(fs_in, fs_out, &g) != NAFP_OK) return -1;
    return (n_in * g.L + g.M - 1) / g.M;
}

extern "C" int nafp_resample_input_range(int64_t n0, int64_t n1, int64_t n_in, int fs_in, int fs_out, int64_t* first, int64_t* last) {
    RsGeom g;
    const int st = rs_geometry(fs_in, fs_out, &g);
    if (st != NAFP_OK) return st;
    if (!first || !last || n0 < 0 || n1 < n0 || n1 > RS_MAX_INDEX || n_in < 0 || n_in > RS_MAX_INDEX) return NAFP_ERR_INVALID_ARG;
    rs_input_range(n0, n1, n_in, g.L, g.M, g.half, first, last);
    return NAFP_OK;
}

extern "C" int nafp_resample_check_pieces_host(int fs_in, int fs_out, const nafp_resample_piece* pieces_host, int64_t n_pieces,
                                               int64_t raw_samples, int64_t out_samples) {
    RsGeom g;
    const int st = rs_geometry(fs_in, fs_out, &g);
    if (st != NAFP_OK) return st;
    if (n_pieces < 0 || raw_samples < 0 || out_samples < 0 || (n_pieces > 0 && !pieces_host)) return NAFP_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n_pieces; ++i) {
        if (pieces_host[i].channels != 1 && pieces_host[i].channels != 2) return NAFP_ERR_UNSUPPORTED;
        if (rs_piece_fault(pieces_host[i], g.L, g.M, g.half, raw_samples, out_samples) != 0) return NAFP_ERR_INVALID_ARG;
    }
    return NAFP_OK;
}

extern "C" int nafp_resample_create(nafp_resample** plan, int fs_in, int fs_out) {
    if (!plan) return NAFP_ERR_INVALID_ARG;
    *plan = nullptr;
    RsGeom g;
    const int st = rs_geometry(fs_in, fs_out, &g);
    if (st != NAFP_OK) return st;
    const RsDesign d(g, fs_in, fs_out);
    std::vector<int32_t> tab((size_t)g.T * g.L);                           // device layout [tap][phase]
    for (int t = 0; t < g.T; ++t)
        for (int p = 0; p < g.L; ++p) tab[(size_t)t * g.L + p] = d.hq((int64_t)p + (int64_t)t * g.L - g.half);
    nafp_resample* h = new nafp_resample{fs_in, fs_out, g.L, g.M, g.half, g.T, 0, nullptr};
    // jb of the last output of a block minus jb of its first <= ceil((RS_BLOCK - 1) M / L); + T taps below the first
    h->span_cap = (int)(((int64_t)(RS_BLOCK - 1) * g.M + g.L - 1) / g.L) + g.T + 1;
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

extern "C" int nafp_resample_destroy(nafp_resample* plan) {
    if (!plan) return NAFP_OK;
    if (plan->d_tab) (void)hipFree(plan->d_tab);
    delete plan;
    return NAFP_OK;
}

extern "C" int nafp_resample_i16(nafp_resample* plan, const int16_t* raw, int64_t raw_samples, const nafp_resample_piece* pieces_dev,
                                 int64_t n_pieces, int16_t* out, int64_t out_samples, void* stream) {
    if (!plan || !raw || !out || n_pieces < 0 || raw_samples < 0 || out_samples < 0 || (n_pieces > 0 && !pieces_dev))
        return NAFP_ERR_INVALID_ARG;
    if (n_pieces == 0 || out_samples == 0) return NAFP_OK;
    const int lds = plan->span_cap * (int)sizeof(int32_t);
    if (lds > 64 * 1024) return NAFP_ERR_UNSUPPORTED;                      // <= 31 KB for every supported ratio
    // blockIdx.y = piece; the blocks of a row stride over the piece's 256-output blocks.  The row is sized for twice the mean
    // piece, so that equal pieces take one step; the bytes written do not depend on it.
    const int64_t blocks = (out_samples + RS_BLOCK - 1) / RS_BLOCK;
    for (int64_t p0 = 0; p0 < n_pieces; p0 += 32768) {
        const int64_t np = n_pieces - p0 < 32768 ? n_pieces - p0 : 32768;
        int64_t gx = 2 * ((blocks + n_pieces - 1) / n_pieces);
        gx = gx < 1 ? 1 : (gx > 8192 ? 8192 : gx);
        resample_i16_kernel<<<dim3((unsigned)gx, (unsigned)np), RS_BLOCK, lds, (hipStream_t)stream>>>(
            plan->d_tab, plan->L, plan->M, plan->half, plan->T, plan->span_cap, raw, raw_samples, pieces_dev + p0, out, out_samples);
        NAFP_LAUNCH_CHECK();
    }
    return NAFP_OK;
}
