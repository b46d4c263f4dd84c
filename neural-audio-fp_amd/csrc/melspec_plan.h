// The front end's plan object and what melspec.hip (the tuned 1024 / 256 kernel, the layer's tail, the entry points) and
// melspec_any.hip (the general kernel and the host-side planning) share.
#pragma once
#include "nafp_common.h"

#include <vector>

struct nafp_melspec {
    int fs, seg_len, n_fft, hop, n_mels, n_frames;
    float f_min, f_max;
    float2* d_twiddle;     // tuned: 1024 of exp(-2 pi i n / 1024); general: 3 n_fft / 4 of exp(-2 pi i n / n_fft)
    float* d_window;       // n_fft, periodic Hann
    int* d_mel_start;      // n_mels: first bin of every filter
    float* d_mel_w;        // tuned: n_mels * 8; general: the non-zero runs of all filters, one after another
    // general kernel only (kind == 1; a plan of nafp_melspec_create has all of these zero)
    int kind;              // 0 tuned (melspec_r16_kernel), 1 general (melspec_any_kernel)
    int log2n, fft_par, lds_bytes;
    int* d_mel_cnt;        // n_mels: taps of every filter (0: an empty one)
    int* d_mel_off;        // n_mels: where its weights start in d_mel_w
};

namespace nafp {

constexpr int MELSPEC_MAX_SEG = 1 << 22;
constexpr int ANY_CHUNK_FRAMES = 16;         // frames per workgroup of the general kernel (even: frames are transformed in pairs)
constexpr int ANY_TILE_LD = ANY_CHUNK_FRAMES + 1;
constexpr int ANY_MAX_MELS = 512;
constexpr int ANY_MAX_GRID_Y = 65535;         // workgroups per segment at the most; a segment of more chunks strides them
constexpr int ANY_MIN_FFT = 128, ANY_MAX_FFT = 4096;

void mel_bank_host(int fs, int n_fft, int n_mels, double fmin, double fmax, std::vector<float>& out);
int melspec_tuned_lds_bytes(int n_mels);     // dynamic LDS of melspec_r16_kernel
int melspec_tuned_chunk_frames();

// What nafp_melspec_create_ex builds for a geometry, decided on the host without any HIP call.
struct MelspecHostPlan {
    int kernel;                    // 0 tuned, 1 general
    int n_frames, n_bins;
    int nnz, widest, empty;        // of the mel bank: non-zero weights, taps of the widest filter, all-zero filters
    int chunk_frames, n_chunks;    // frames per workgroup, chunks per segment (grid y, up to ANY_MAX_GRID_Y)
    int fft_par;                   // complex FFTs (= frame pairs) a workgroup transforms at a time
    int lds_bytes;
    int log2n;
    std::vector<int> start, cnt, off;     // general kernel: per filter
    std::vector<float> w;                 // general kernel: nnz-or-more weights (the runs first bin ... last bin of every filter)
};
int melspec_host_plan(int fs, int seg_len, int n_fft, int hop, int n_mels, float f_min, float f_max, int flags, MelspecHostPlan& out);

template <typename TIn>
int launch_melspec_any(const nafp_melspec* p, const TIn* audio, const int64_t* seg_offset, const int* seg_valid, int64_t n_seg,
                       int group_size, float* feat, float* group_stat, hipStream_t st);

}  // namespace nafp
