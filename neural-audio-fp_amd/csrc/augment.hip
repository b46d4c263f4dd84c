// Time-domain augmentation of a training batch on the device, gfx950.
//
// Replaces the host loops of the reference's training loader -- load_audio per segment,
// bg_mix_batch, ir_aug_batch (model/utils/audio_utils.py:28-137, 221-264) as called from
// genUnbalSequence.__getitem__ (model/utils/dataloader_keras.py:223-311) -- which SURVEY.md names the
// true bottleneck of reference training.  One workgroup per output row; the row lives in LDS.
//   x   = event window / 2^15                      (zero tail: load_audio's padding)
//   nz  = background window (+ speech window) / 2^15
//   mix : max|x| == 0 or max|nz| == 0 ? x + nz : 10^(snr/20) x / rms(x) + nz / rms(nz)
//         -> max-normalise -> * amp                 (background_mix, bg_mix_batch)
//   ir  : circular convolution of length T with the <= 600-tap impulse response, summed directly
//         (4 outputs x 4 taps per step from three aligned LDS float4 reads) == the reference's
//         ifft(fft(ir, T) * fft(x, T)) (ir_aug_batch), then max-normalise.
// Rows without noise / IR windows (the anchors) are plain int16 -> float conversions, so ONE launch
// produces the whole (anchors | replicas) batch that feeds the log-mel kernel.
#include <type_traits>

#include "nafp_common.h"

namespace nafp {

__device__ __forceinline__ float block_max(float v, float* red, int tid) {
    v = wave_max(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float block_sum(float v, float* red, int tid) {
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

constexpr int MAX_IR = 608;       // MAX_IR_LENGTH = 600 (dataloader_keras.py:8), padded to a multiple of 4 (+4 guard)

// What makes a speed entry inconsistent (nafp.h); the kernel and nafp_augment_speed_check_host share it.  0: consistent
__host__ __device__ inline int aug_speed_fault(const nafp_aug_speed& sp, int n_steps, int64_t pcm_samples) {
    if (sp.slot < 0 || sp.slot >= n_steps) return 1;
    if (sp.out0 < 0 || sp.out0 > 2 * VS_MAX_IN) return 1;                      // (out0 + T) step stays far inside int64
    if (sp.n_in < 0 || sp.n_in >= VS_MAX_IN) return 2;
    if (sp.file_off < 0 || sp.file_off > pcm_samples || sp.n_in > pcm_samples - sp.file_off) return 1;
    return 0;
}
// the widest input span of T consecutive outputs, with the padding taps: what must fit the 2 T int16 of the noise buffer
__host__ __device__ inline int64_t aug_speed_span_cap(int T) { return ((((int64_t)T - 1) * NAFP_VARISPEED_STEP_MAX) >> 24) + VS_MAX_TP + 1; }

struct AugSpeedArgs {
    const nafp_aug_speed* speeds;     // one per row
    const VsSlot* slots;
    int n_steps;
    int64_t pcm_samples;
};

// x[i] = y[out0 + i] / 2^15 of the varispeed contract (varispeed.hip) over the row's file, i < T.  s_in: 2 T int16 (the row's noise
// buffer, not written before the mix): the input span of the T outputs is staged there once, then every lane walks the Tp taps of
// its two adjacent table rows with 16-byte loads, as varispeed_i16_kernel does.  Integers only up to the final conversion.
__device__ __forceinline__ void speed_event(const int16_t* __restrict__ pcm, const AugSpeedArgs& sa, const nafp_aug_speed& sp, int T,
                                            float* x, int16_t* s_in, int tid) {
    const float sc = 1.f / 32768.f;
    int cnt = 0;                                                           // outputs of the window that exist
    uint32_t step = 0; int W = 0, Tp = 0; const int32_t* tab = nullptr;
    int64_t pos_a = 0, fill = 0;
    if (aug_speed_fault(sp, sa.n_steps, sa.pcm_samples) == 0) {
        const VsSlot s = sa.slots[sp.slot];
        step = s.step; W = s.W; Tp = s.Tp; tab = s.tab;
        const int64_t left = vs_n_out(sp.n_in, step) - sp.out0;
        cnt = left <= 0 ? 0 : (left < T ? (int)left : T);
        if (cnt > 0) {
            pos_a = (sp.out0 * step) >> 24;
            fill = (((sp.out0 + cnt - 1) * step) >> 24) - pos_a + Tp;      // span = pos_b - pos_a + 2 W, + the Tp - 2 W padding taps
            if (fill > 2 * (int64_t)T) cnt = 0;                            // (the launch refuses such a T)
        }
    }
    if (cnt > 0) {
        const int64_t jlo = pos_a - W + 1;
        const int16_t* pf = pcm + sp.file_off;                             // [0, n_in) is inside the arena (no fault)
        for (int i = tid; i < (int)fill; i += 256) {
            const int64_t j = jlo + i;
            s_in[i] = j >= 0 && j < sp.n_in ? pf[j] : (int16_t)0;          // outside the file: zero, never a neighbour's sample
        }
    }
    __syncthreads();
    for (int i = tid; i < T; i += 256) {
        float v = 0.f;
        if (i < cnt) {
            const int64_t P = (sp.out0 + i) * step;
            const int frac = (int)(P & 0xffffff);
            const int p = frac >> 15, w = frac & 32767;
            const int4* ra = (const int4*)(tab + (int64_t)p * Tp);         // row p; row p + 1 <= 512 follows it
            const int4* rb = (const int4*)(tab + (int64_t)(p + 1) * Tp);
            const int16_t* sp16 = s_in + (int)((P >> 24) - pos_a);         // sp16[t], t < Tp: inside [0, fill)
            const int64_t wa = 32768 - w, wb = w;
            int64_t acc = 0;
#pragma unroll 2
            for (int t4 = 0; t4 < (Tp >> 2); ++t4) {
                const int4 a = ra[t4], b = rb[t4];
                const int16_t* xs = sp16 + 4 * t4;
                acc += (int64_t)(int32_t)((a.x * wa + b.x * wb + 16384) >> 15) * xs[0];
                acc += (int64_t)(int32_t)((a.y * wa + b.y * wb + 16384) >> 15) * xs[1];
                acc += (int64_t)(int32_t)((a.z * wa + b.z * wb + 16384) >> 15) * xs[2];
                acc += (int64_t)(int32_t)((a.w * wa + b.w * wb + 16384) >> 15) * xs[3];
            }
            int64_t y = (acc + ((int64_t)1 << 29)) >> 30;
            y = y < -32768 ? -32768 : (y > 32767 ? 32767 : y);
            v = (float)(int16_t)y * sc;
        }
        x[i] = v;
    }
    __syncthreads();                                                       // the span is read; the mix may write the noise buffer
}

struct AugNoArgs {};

// One workgroup per row.  SPEED: rows whose speed entry has a slot other than -1 take their event from speed_event; that is compiled
// out of the plain instantiation, nafp_augment_rows's kernel.
template <bool SPEED>
__global__ __launch_bounds__(256) void augment_rows_kernel(const int16_t* __restrict__ pcm, const nafp_aug_row* __restrict__ rows,
                                                           float* __restrict__ out, int T,
                                                           std::conditional_t<SPEED, AugSpeedArgs, AugNoArgs> sa) {
    extern __shared__ __attribute__((aligned(16))) float smem[];      // x[T] | y[T] (a speed row's input span first) | ir[MAX_IR]
    __shared__ float red[4];
    float* x = smem; float* y = smem + T; float* ir = smem + 2 * T;
    const int tid = threadIdx.x;
    const nafp_aug_row r = rows[blockIdx.x];
    const float sc = 1.f / 32768.f;
    bool plain = true;
    if constexpr (SPEED) {
        const nafp_aug_speed sp = sa.speeds[blockIdx.x];
        if (sp.slot != -1) {                                               // uniform over the workgroup
            plain = false;
            speed_event(pcm, sa, sp, T, x, (int16_t*)y, tid);
        }
    }
    if (plain) {
        const int16_t* pe = pcm + r.ev_off;
        for (int i = tid; i < T; i += 256) x[i] = i < r.ev_valid ? (float)pe[i] * sc : 0.f;
    }
    float* cur = x;
    if (r.mix) {
        const int16_t* p1 = pcm + (r.nz_off >= 0 ? r.nz_off : 0);
        const int16_t* p2 = pcm + (r.nz2_off >= 0 ? r.nz2_off : 0);
        const int v1 = r.nz_off >= 0 ? r.nz_valid : 0, v2 = r.nz2_off >= 0 ? r.nz2_valid : 0;
        float xm = 0.f, nm = 0.f, xs = 0.f, ns = 0.f;
        for (int i = tid; i < T; i += 256) {
            const float n = (i < v1 ? (float)p1[i] * sc : 0.f) + (i < v2 ? (float)p2[i] * sc : 0.f);
            y[i] = n;
            const float xv = x[i];
            xm = fmaxf(xm, fabsf(xv)); nm = fmaxf(nm, fabsf(n));
            xs = fmaf(xv, xv, xs); ns = fmaf(n, n, ns);
        }
        xm = block_max(xm, red, tid); nm = block_max(nm, red, tid);
        xs = block_sum(xs, red, tid); ns = block_sum(ns, red, tid);
        float a = 1.f, b = 1.f;
        if (xm != 0.f && nm != 0.f) {
            a = exp10f(r.snr_db / 20.f) / sqrtf(xs / (float)T);
            b = 1.f / sqrtf(ns / (float)T);
        }
        float mm = 0.f;
        for (int i = tid; i < T; i += 256) { const float m = a * x[i] + b * y[i]; x[i] = m; mm = fmaxf(mm, fabsf(m)); }
        mm = block_max(mm, red, tid);
        const float g = (mm != 0.f ? 1.f / mm : 1.f) * r.amp;
        for (int i = tid; i < T; i += 256) x[i] *= g;
    }
    __syncthreads();
    if (r.ir_off >= 0 && r.ir_len > 0) {
        const int L = min(r.ir_len, MAX_IR - 8);
        const int L4 = (L + 3) & ~3;
        const int16_t* pi = pcm + r.ir_off;
        for (int i = tid; i < MAX_IR; i += 256) ir[i] = i < L ? (float)pi[i] * sc : 0.f;
        __syncthreads();
        // y[n] = sum_k ir[k] x[(n - k) mod T]; thread <-> 4 consecutive outputs, 4 taps per step.
        // T % 4 == 0, so (n0 - k) mod T stays 4-aligned and the two x reads are aligned float4.
        float ym = 0.f;
        for (int n0 = 4 * tid; n0 < T; n0 += 1024) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            int p = n0;                                   // (n0 - k) mod T for the current k
            for (int k = 0; k < L4; k += 4) {
                const float4 h = *(const float4*)(ir + k);
                const float4 hi = *(const float4*)(x + p);               // x[p .. p+3]   = x[n0-k+j]
                int pl = p - 4; if (pl < 0) pl += T;
                const float4 lo = *(const float4*)(x + pl);              // x[p-4 .. p-1]
                // output j uses x[p + j - t] for tap k + t
                acc.x = fmaf(h.x, hi.x, fmaf(h.y, lo.w, fmaf(h.z, lo.z, fmaf(h.w, lo.y, acc.x))));
                acc.y = fmaf(h.x, hi.y, fmaf(h.y, hi.x, fmaf(h.z, lo.w, fmaf(h.w, lo.z, acc.y))));
                acc.z = fmaf(h.x, hi.z, fmaf(h.y, hi.y, fmaf(h.z, hi.x, fmaf(h.w, lo.w, acc.z))));
                acc.w = fmaf(h.x, hi.w, fmaf(h.y, hi.z, fmaf(h.z, hi.y, fmaf(h.w, hi.x, acc.w))));
                p = pl;
            }
            *(float4*)(y + n0) = acc;
            ym = fmaxf(fmaxf(ym, fmaxf(fabsf(acc.x), fabsf(acc.y))), fmaxf(fabsf(acc.z), fabsf(acc.w)));
        }
        ym = block_max(ym, red, tid);
        const float g = ym != 0.f ? 1.f / ym : 1.f;
        for (int i = tid; i < T; i += 256) y[i] *= g;
        __syncthreads();
        cur = y;
    }
    float* o = out + (int64_t)blockIdx.x * T;
    for (int i = tid; i < T / 4; i += 256) ((float4*)o)[i] = ((const float4*)cur)[i];
}

}  // namespace nafp

using namespace nafp;

extern "C" int nafp_augment_rows(const int16_t* pcm, const nafp_aug_row* rows, int64_t n_rows, int seg_len, float* out,
                                 void* stream) {
    if (!pcm || !rows || !out || n_rows < 0 || seg_len <= 0) return NAFP_ERR_INVALID_ARG;
    if (seg_len % 4 != 0 || seg_len > 19000) return NAFP_ERR_UNSUPPORTED;        // x | y | ir must fit the 160 KB LDS
    if (n_rows == 0) return NAFP_OK;
    const int lds = (2 * seg_len + MAX_IR) * (int)sizeof(float);
    NAFP_HIP_CHECK(hipFuncSetAttribute((const void*)augment_rows_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    augment_rows_kernel<false><<<dim3((unsigned)n_rows), 256, lds, (hipStream_t)stream>>>(pcm, rows, out, seg_len, AugNoArgs{});
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}

extern "C" int nafp_augment_speed_check_host(const nafp_aug_speedset* set, const nafp_aug_row* rows_host, const nafp_aug_speed* speeds_host,
                                             int64_t n_rows, int64_t pcm_samples, int seg_len) {
    if (!set || n_rows < 0 || pcm_samples < 0 || seg_len <= 0 || (n_rows > 0 && (!rows_host || !speeds_host))) return NAFP_ERR_INVALID_ARG;
    if (seg_len % 4 != 0 || seg_len > 19000 || aug_speed_span_cap(seg_len) > 2 * (int64_t)seg_len) return NAFP_ERR_UNSUPPORTED;
    for (int64_t i = 0; i < n_rows; ++i) {
        if (speeds_host[i].slot == -1) continue;
        const int f = aug_speed_fault(speeds_host[i], set->n_steps, pcm_samples);
        if (f != 0) return f == 2 && speeds_host[i].n_in >= VS_MAX_IN ? NAFP_ERR_UNSUPPORTED : NAFP_ERR_INVALID_ARG;
    }
    return NAFP_OK;
}

extern "C" int nafp_augment_rows_speed(nafp_aug_speedset* set, const int16_t* pcm, int64_t pcm_samples, const nafp_aug_row* rows,
                                       const nafp_aug_speed* speeds, int64_t n_rows, int seg_len, float* out, void* stream) {
    if (!speeds) return nafp_augment_rows(pcm, rows, n_rows, seg_len, out, stream);
    if (!set || !pcm || !rows || !out || n_rows < 0 || seg_len <= 0 || pcm_samples < 0) return NAFP_ERR_INVALID_ARG;
    if (seg_len % 4 != 0 || seg_len > 19000 || aug_speed_span_cap(seg_len) > 2 * (int64_t)seg_len) return NAFP_ERR_UNSUPPORTED;
    if (n_rows == 0) return NAFP_OK;
    const int st = aug_speedset_upload(set);
    if (st != NAFP_OK) return st;
    const int lds = (2 * seg_len + MAX_IR) * (int)sizeof(float);              // as nafp_augment_rows: the span lives in y
    NAFP_HIP_CHECK(hipFuncSetAttribute((const void*)augment_rows_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    augment_rows_kernel<true><<<dim3((unsigned)n_rows), 256, lds, (hipStream_t)stream>>>(
        pcm, rows, out, seg_len, AugSpeedArgs{speeds, set->d_slots, set->n_steps, pcm_samples});
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}
