// General front end: the log-mel layer of melspec.hip for any power-of-two STFT window (128 ... 4096), any hop <= window, any
// mel bank of up to 512 filters of any width.  gfx950.  Reached only through nafp_melspec_create_ex, for the geometries the tuned
// kernel (melspec_r16_kernel: 1024 / 256, <= 8 taps) refuses -- or, with NAFP_MELSPEC_FORCE_GENERAL, for A/B runs against it.
//
// One 256-thread workgroup per (segment, chunk of 16 frames); beyond 65,535 chunks a workgroup takes several, 65,535 apart.  Two real frames are packed into one complex n_fft-point FFT
// (frame 2p -> re, frame 2p + 1 -> im), transformed in place in LDS by radix-4 decimation-in-frequency passes (one radix-2
// pass at the end when log2(n_fft) is odd), un-packed into two magnitude spectra, and the mel bank is applied as a sparse gather
// (first bin, tap count, weights per filter -- never a dense matrix).  A window of 1024 points or more is transformed by the
// whole workgroup, one pair at a time; smaller windows run 1024 / n_fft pairs side by side, 256 n_fft / 1024 threads each.
// The samples are read straight from global memory (a sample is reused by n_fft / hop frames; those reads hit the caches), so
// neither the segment length, the hop nor an odd window offset costs LDS or an alignment case.
//
// A segment's raw log-mel bytes are a pure function of its samples: frames are always paired (2p, 2p + 1) by their index in
// the segment (chunks start at even frames), every sum runs in one fixed order (taps ascending), and nothing is shared between
// segments but the order-independent (max, min) atomics of the group.
//
// Dynamic LDS, floats:  2 max(n_fft, 1024)  FFT buffers  +  1.5 n_fft  twiddles  +  2 fft_par (n_fft / 2 + 4)  magnitudes
//                       +  17 n_mels  tile.
//   n_fft  128 / 256 / 512 / 1024 / 2048 / 4096, 256 mels:  30,720 / 31,360 / 32,832 / 35,872 / 54,304 / 91,168 B
//   the largest corner (4096, 512 mels):  108,576 B  -- within a CU's 160 KB everywhere, above 64 KB only at 4096.
#include "melspec_plan.h"

#include <algorithm>
#include <cmath>

namespace nafp {

__device__ __forceinline__ float2 any_cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// where X[k] sits after the in-place passes: the base-4 digits of k reversed; with an odd log2 n the last (radix-2) pass leaves
// the top bit of k in bit 0 and the digit pairs one bit higher
__device__ __forceinline__ int any_digit_rev(int k, int log2n) {
    const unsigned r = __brev((unsigned)k) >> (32 - log2n);
    if (log2n & 1) {
        const unsigned h = r >> 1;
        return (int)((r & 1u) | ((((h & 0x55555555u) << 1) | ((h >> 1) & 0x55555555u)) << 1));
    }
    return (int)(((r & 0x55555555u) << 1) | ((r >> 1) & 0x55555555u));
}

template <typename T> __device__ __forceinline__ float any_pcm(T v);
template <> __device__ __forceinline__ float any_pcm<float>(float v) { return v; }
template <> __device__ __forceinline__ float any_pcm<int16_t>(int16_t v) { return (float)v * (1.0f / 32768.0f); }   // exact in f32

template <typename TIn>
__global__ __launch_bounds__(256) void melspec_any_kernel(
        const TIn* __restrict__ audio, const int64_t* __restrict__ seg_offset, const int* __restrict__ seg_valid,
        float* __restrict__ feat, float* __restrict__ group_stat,
        const float2* __restrict__ tw, const float* __restrict__ window,
        const int* __restrict__ mel_start, const int* __restrict__ mel_cnt, const int* __restrict__ mel_off,
        const float* __restrict__ mel_w,
        int seg_len, int n_frames, int n_mels, int group_size, int hop, int log2n, int fft_par) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t seg = blockIdx.x;
    const int N = 1 << log2n, nbin = (N >> 1) + 1, magld = (N >> 1) + 4;
    float2* fftbuf = (float2*)smem;                                  // [fft_par][N]
    float2* stw = fftbuf + fft_par * N;                              // [3 N / 4]
    float* mag = (float*)(stw + 3 * (N >> 2));                       // [2 fft_par][magld]
    float* tile = mag + 2 * fft_par * magld;                         // [n_mels][ANY_TILE_LD]
    for (int i = tid; i < 3 * (N >> 2); i += 256) stw[i] = tw[i];

    const TIn* a = audio + (seg_offset ? seg_offset[seg] : seg * seg_len);
    const int n_valid = seg_valid ? max(min(seg_valid[seg], seg_len), 0) : seg_len;
    const int tpf = 256 / fft_par;                                   // threads per FFT (a power of two, >= n_fft / 4 or 256)
    const int slot = tid / tpf, t = tid - slot * tpf;
    float2* z = fftbuf + slot * N;
    const int n_chunks = (n_frames + ANY_CHUNK_FRAMES - 1) / ANY_CHUNK_FRAMES;
    float* out_seg = feat + seg * (int64_t)n_mels * n_frames;
    float lmax = -INFINITY, lmin = INFINITY;
    __syncthreads();

    // grid y holds at most ANY_MAX_GRID_Y workgroups per segment: a longer segment's chunks are strided over them
    for (int chunk = blockIdx.y; chunk < n_chunks; chunk += gridDim.y) {
        const int chunk0 = chunk * ANY_CHUNK_FRAMES;
        const int chunk_frames = min(ANY_CHUNK_FRAMES, n_frames - chunk0);
        const int n_rounds = ((chunk_frames + 1) / 2 + fft_par - 1) / fft_par;
        for (int round = 0; round < n_rounds; ++round) {
            const int f0 = chunk0 + 2 * (round * fft_par + slot), f1 = f0 + 1;
            const bool live = f0 < chunk0 + chunk_frames;
            const bool has1 = f1 < n_frames;
            if (live) {
                // z[n] = w[n] (x_f0[n] + i x_f1[n]); frame f covers padded samples f hop ... f hop + N - 1, i.e. samples - N / 2
                const int s_base = f0 * hop - (N >> 1);
                for (int n = t; n < N; n += tpf) {
                    const int s0 = s_base + n, s1 = s0 + hop;
                    const float w = window[n];
                    const float x0 = (s0 >= 0 && s0 < n_valid) ? any_pcm<TIn>(a[s0]) : 0.f;
                    const float x1 = (has1 && s1 >= 0 && s1 < n_valid) ? any_pcm<TIn>(a[s1]) : 0.f;
                    z[n] = make_float2(w * x0, w * x1);
                }
            }
            __syncthreads();
            // radix-4 passes of span S = N / 4, N / 16, ... (down to 1, or to 2 when log2 N is odd); tmul = N / (4 S)
            int tmul = 1;
            for (int S = N >> 2; S >= 1; S >>= 2, tmul <<= 2) {
                if (live) {
                    for (int b = t; b < (N >> 2); b += tpf) {
                        const int off = b & (S - 1);
                        const int base = ((b - off) << 2) + off;
                        const float2 u0 = z[base], u1 = z[base + S], u2 = z[base + 2 * S], u3 = z[base + 3 * S];
                        const float2 t0 = make_float2(u0.x + u2.x, u0.y + u2.y);
                        const float2 t1 = make_float2(u0.x - u2.x, u0.y - u2.y);
                        const float2 t2 = make_float2(u1.x + u3.x, u1.y + u3.y);
                        const float2 t3 = make_float2(u1.y - u3.y, -(u1.x - u3.x));   // (u1 - u3) * (-i)
                        float2 y1 = make_float2(t1.x + t3.x, t1.y + t3.y);
                        float2 y2 = make_float2(t0.x - t2.x, t0.y - t2.y);
                        float2 y3 = make_float2(t1.x - t3.x, t1.y - t3.y);
                        if (S > 1) {
                            const int m = off * tmul;                                  // 3 m < 3 N / 4
                            y1 = any_cmul(y1, stw[m]); y2 = any_cmul(y2, stw[2 * m]); y3 = any_cmul(y3, stw[3 * m]);
                        }
                        z[base] = make_float2(t0.x + t2.x, t0.y + t2.y);
                        z[base + S] = y1; z[base + 2 * S] = y2; z[base + 3 * S] = y3;
                    }
                }
                __syncthreads();
            }
            if (log2n & 1) {
                if (live) {
                    for (int b = t; b < (N >> 1); b += tpf) {
                        const float2 u0 = z[2 * b], u1 = z[2 * b + 1];
                        z[2 * b] = make_float2(u0.x + u1.x, u0.y + u1.y);
                        z[2 * b + 1] = make_float2(u0.x - u1.x, u0.y - u1.y);
                    }
                }
                __syncthreads();
            }
            if (live) {
                // un-pack: X0[k] = (Z[k] + conj Z[N-k]) / 2, X1[k] = (Z[k] - conj Z[N-k]) / (2 i); keep |.| (kapre Magnitude = tf.abs)
                float* mag0 = mag + (2 * slot) * magld;
                float* mag1 = mag0 + magld;
                for (int k = t; k < nbin; k += tpf) {
                    const float2 zk = z[any_digit_rev(k, log2n)];
                    const float2 zc = z[any_digit_rev((N - k) & (N - 1), log2n)];
                    const float ar = 0.5f * (zk.x + zc.x), ai = 0.5f * (zk.y - zc.y);
                    const float br = 0.5f * (zk.y + zc.y), bi = -0.5f * (zk.x - zc.x);
                    mag0[k] = sqrtf(ar * ar + ai * ai);
                    mag1[k] = sqrtf(br * br + bi * bi);
                }
            }
            __syncthreads();
            // mel gather for the frames of this round: item = (frame e of the round, filter m), m fastest
            const int fr0 = chunk0 + 2 * round * fft_par;
            for (int idx = tid; idx < n_mels * 2 * fft_par; idx += 256) {
                const int e = idx / n_mels, m = idx - e * n_mels;
                const int f = fr0 + e;
                if (f < chunk0 + chunk_frames) {
                    const float* mm = mag + e * magld + mel_start[m];
                    const float* ww = mel_w + mel_off[m];
                    const int cnt = mel_cnt[m];
                    float acc = 0.f;
                    for (int j = 0; j < cnt; ++j) acc += ww[j] * mm[j];
                    const float v = logf(max_keep_nan(acc + 0.06f, 1e-10f)) / 2.302585092994046f;     // melspectrogram.py:104,107
                    tile[m * ANY_TILE_LD + (f - chunk0)] = v;
                    lmax = fmaxf(lmax, v);
                    lmin = fminf(lmin, v);
                }
            }
            __syncthreads();
        }
        // tile out: (n_mels, chunk_frames) -> feat[seg][m][chunk0 + t]
        for (int idx = tid; idx < n_mels * chunk_frames; idx += 256) {
            const int m = idx / chunk_frames, c = idx - m * chunk_frames;
            out_seg[(int64_t)m * n_frames + chunk0 + c] = tile[m * ANY_TILE_LD + c];
        }
        __syncthreads();
    }
    // group max / min (melspectrogram.py:108, 110): fmaxf / fminf drop a NaN, as the tuned kernel does
    lmax = wave_max(lmax);
    lmin = wave_min(lmin);
    float* red = tile;                       // >= 17 floats
    if (lane == 0) { red[wave] = lmax; red[4 + wave] = lmin; }
    __syncthreads();
    if (tid == 0) {
        const float mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        const float mn = fminf(fminf(red[4], red[5]), fminf(red[6], red[7]));
        const int64_t g = group_size > 0 ? seg / group_size : 0;
        atomic_max_float(group_stat + 2 * g, mx);
        atomic_min_float(group_stat + 2 * g + 1, mn);
    }
}

static int any_lds_bytes(int n_fft, int n_mels, int fft_par) {
    return (2 * fft_par * n_fft + 3 * (n_fft / 2) + 2 * fft_par * (n_fft / 2 + 4) + n_mels * ANY_TILE_LD) * (int)sizeof(float);
}

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the kernel on the current device, not to a plan: every create sets it to
// what the largest supported geometry needs (4096 / 512 mels), so no plan lowers it under another and every device is served
static int any_raise_lds_limit() {
    const int lds = any_lds_bytes(ANY_MAX_FFT, ANY_MAX_MELS, 1);
    NAFP_HIP_CHECK(hipFuncSetAttribute((const void*)melspec_any_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    NAFP_HIP_CHECK(hipFuncSetAttribute((const void*)melspec_any_kernel<int16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    return NAFP_OK;
}

template <typename TIn>
int launch_melspec_any(const nafp_melspec* p, const TIn* audio, const int64_t* seg_offset, const int* seg_valid, int64_t n_seg,
                       int group_size, float* feat, float* group_stat, hipStream_t st) {
    const int n_chunks = (p->n_frames + ANY_CHUNK_FRAMES - 1) / ANY_CHUNK_FRAMES;
    const dim3 grid((unsigned)n_seg, (unsigned)std::min(n_chunks, ANY_MAX_GRID_Y));     // the kernel strides the chunks over grid y
    melspec_any_kernel<TIn><<<grid, 256, (size_t)p->lds_bytes, st>>>(audio, seg_offset, seg_valid, feat, group_stat, p->d_twiddle,
                                                                     p->d_window, p->d_mel_start, p->d_mel_cnt, p->d_mel_off, p->d_mel_w,
                                                                     p->seg_len, p->n_frames, p->n_mels, group_size, p->hop, p->log2n,
                                                                     p->fft_par);
    NAFP_LAUNCH_CHECK();
    return NAFP_OK;
}
template int launch_melspec_any<float>(const nafp_melspec*, const float*, const int64_t*, const int*, int64_t, int, float*, float*,
                                       hipStream_t);
template int launch_melspec_any<int16_t>(const nafp_melspec*, const int16_t*, const int64_t*, const int*, int64_t, int, float*,
                                         float*, hipStream_t);

int melspec_host_plan(int fs, int seg_len, int n_fft, int hop, int n_mels, float f_min, float f_max, int flags,
                      MelspecHostPlan& out) {
    if (fs <= 0 || seg_len <= 0 || !(f_max > f_min)) return NAFP_ERR_INVALID_ARG;
    if (flags & ~(NAFP_MELSPEC_ANY_GEOMETRY | NAFP_MELSPEC_FORCE_GENERAL)) return NAFP_ERR_INVALID_ARG;
    const bool tuned_shape = n_fft == 1024 && hop == 256 && n_mels > 0 && n_mels <= 256 && (n_mels % 64) == 0 &&
                             seg_len <= MELSPEC_MAX_SEG;
    const bool general_shape = n_fft >= ANY_MIN_FFT && n_fft <= ANY_MAX_FFT && (n_fft & (n_fft - 1)) == 0 && hop >= 1 &&
                               hop <= n_fft && n_mels >= 1 && n_mels <= ANY_MAX_MELS && seg_len <= MELSPEC_MAX_SEG;
    if (!tuned_shape && !(flags && general_shape)) return NAFP_ERR_UNSUPPORTED;
    const int nbin = n_fft / 2 + 1;
    std::vector<float> fb;
    mel_bank_host(fs, n_fft, n_mels, f_min, f_max, fb);
    out.start.assign(n_mels, 0); out.cnt.assign(n_mels, 0); out.off.assign(n_mels, 0);
    out.w.clear();
    out.nnz = out.widest = out.empty = 0;
    for (int m = 0; m < n_mels; ++m) {
        int lo = -1, hi = -1;
        for (int k = 0; k < nbin; ++k)
            if (fb[(size_t)m * nbin + k] != 0.f) { if (lo < 0) lo = k; hi = k; ++out.nnz; }
        out.off[m] = (int)out.w.size();
        if (lo < 0) { ++out.empty; continue; }
        out.start[m] = lo; out.cnt[m] = hi - lo + 1;
        out.widest = std::max(out.widest, hi - lo + 1);
        out.w.insert(out.w.end(), fb.begin() + (size_t)m * nbin + lo, fb.begin() + (size_t)m * nbin + hi + 1);
    }
    const bool tuned_ok = tuned_shape && out.widest <= 8;
    if (tuned_ok && !(flags & NAFP_MELSPEC_FORCE_GENERAL)) out.kernel = 0;
    else if (flags && general_shape) out.kernel = 1;
    else return NAFP_ERR_UNSUPPORTED;
    out.n_frames = 1 + seg_len / hop;
    out.n_bins = nbin;
    out.log2n = 0;
    while ((1 << out.log2n) < n_fft) ++out.log2n;
    if (out.kernel == 0) {
        out.chunk_frames = melspec_tuned_chunk_frames();
        out.fft_par = 4;                                  // one frame pair per wave
        out.lds_bytes = melspec_tuned_lds_bytes(n_mels);
    } else {
        out.chunk_frames = ANY_CHUNK_FRAMES;
        out.fft_par = n_fft >= 1024 ? 1 : 1024 / n_fft;
        out.lds_bytes = any_lds_bytes(n_fft, n_mels, out.fft_par);
    }
    out.n_chunks = (out.n_frames + out.chunk_frames - 1) / out.chunk_frames;
    return NAFP_OK;
}

}  // namespace nafp

using namespace nafp;

extern "C" int nafp_melspec_plan_host(int fs, int seg_len, int n_fft, int hop, int n_mels, float f_min, float f_max, int flags,
                                      int64_t* record_host) {
    if (!record_host) return NAFP_ERR_INVALID_ARG;
    MelspecHostPlan hp;
    const int rc = melspec_host_plan(fs, seg_len, n_fft, hop, n_mels, f_min, f_max, flags, hp);
    if (rc != NAFP_OK) return rc;
    const int64_t rec[NAFP_MELSPEC_PLAN_FIELDS] = {hp.kernel, hp.n_frames, hp.n_bins, hp.nnz, hp.widest, hp.empty, hp.chunk_frames,
                                                   hp.lds_bytes, hp.n_chunks, hp.fft_par};
    std::copy(rec, rec + NAFP_MELSPEC_PLAN_FIELDS, record_host);
    return NAFP_OK;
}

extern "C" int nafp_melspec_create_ex(nafp_melspec** plan, int fs, int seg_len, int n_fft, int hop, int n_mels, float f_min,
                                      float f_max, int flags) {
    if (!plan) return NAFP_ERR_INVALID_ARG;
    MelspecHostPlan hp;
    const int rc = melspec_host_plan(fs, seg_len, n_fft, hop, n_mels, f_min, f_max, flags, hp);
    if (rc != NAFP_OK) return rc;                      // decided before any HIP call
    if (hp.kernel == 0) return nafp_melspec_create(plan, fs, seg_len, n_fft, hop, n_mels, f_min, f_max);
    const int n_tw = 3 * (n_fft / 4);
    std::vector<float2> tw(n_tw);
    std::vector<float> win(n_fft);
    for (int n = 0; n < n_tw; ++n) {
        const double a = -2.0 * M_PI * n / n_fft;
        tw[n] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    for (int n = 0; n < n_fft; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / n_fft));   // tf.signal.hann_window, periodic
    if (hp.w.empty()) hp.w.push_back(0.f);             // a bank of empty filters only: keep the allocation non-empty
    nafp_melspec* p = new nafp_melspec();
    p->fs = fs; p->seg_len = seg_len; p->n_fft = n_fft; p->hop = hop; p->n_mels = n_mels;
    p->f_min = f_min; p->f_max = f_max;
    p->n_frames = hp.n_frames;
    p->kind = 1; p->log2n = hp.log2n; p->fft_par = hp.fft_par; p->lds_bytes = hp.lds_bytes;
    auto fail = [&](hipError_t e) { g_last_hip_error = (int)e; nafp_melspec_destroy(p); return NAFP_ERR_HIP; };
    hipError_t e;
    if ((e = hipMalloc(&p->d_twiddle, sizeof(float2) * n_tw)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&p->d_window, sizeof(float) * n_fft)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&p->d_mel_start, sizeof(int) * n_mels)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&p->d_mel_cnt, sizeof(int) * n_mels)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&p->d_mel_off, sizeof(int) * n_mels)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&p->d_mel_w, sizeof(float) * hp.w.size())) != hipSuccess) return fail(e);
    if ((e = hipMemcpy(p->d_twiddle, tw.data(), sizeof(float2) * n_tw, hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    if ((e = hipMemcpy(p->d_window, win.data(), sizeof(float) * n_fft, hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    if ((e = hipMemcpy(p->d_mel_start, hp.start.data(), sizeof(int) * n_mels, hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    if ((e = hipMemcpy(p->d_mel_cnt, hp.cnt.data(), sizeof(int) * n_mels, hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    if ((e = hipMemcpy(p->d_mel_off, hp.off.data(), sizeof(int) * n_mels, hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    if ((e = hipMemcpy(p->d_mel_w, hp.w.data(), sizeof(float) * hp.w.size(), hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    if (any_raise_lds_limit() != NAFP_OK) { nafp_melspec_destroy(p); return NAFP_ERR_HIP; }
    *plan = p;
    return NAFP_OK;
}

extern "C" int nafp_melspec_kernel(const nafp_melspec* p) { return p ? p->kind : -1; }
