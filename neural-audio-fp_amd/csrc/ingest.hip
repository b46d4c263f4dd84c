// Ingest of sample data of any PCM or IEEE-float format -- little-endian as RIFF/WAVE holds it, or big-endian and signed 8-bit as
// AIFF / AIFF-C and AU do (NAFP_INGEST_BE, NAFP_INGEST_S8) -- 1 to 8 channels, at any supported rate -- up OR down -- to int16 mono at
// the model rate, gfx950.  The general sibling of resample.hip (16-bit, 1 or 2 channels, downsampling), which
// stays as it is; for the files both take, the bytes are the same.
//
// Contract (include/nafp.h has it in full): every sample is first DECODED to the canonical q, a signed integer at 2^-23 of
// full scale (|q| <= 2^23); the channels of a frame are summed, m[j] = sum_c q[j][c] (|m| <= 2^26); then, with
// g = gcd(fs_in, fs_out), L = fs_out / g, M = fs_in / g and the Kaiser-windowed sinc hq[-half .. half] designed for the LOWER
// of the two rates at the virtual rate fs_in * L (int32, 30 fraction bits),
//     acc[n] = sum_j hq[n M - j L] * m[j]                       (int64, exact: |acc| < 2^58)
//     y[n]   = clamp(floor((acc[n] + D / 2) / D), -32768, 32767),   D = channels * 2^38, floor division.
// An output sample is a pure function of (file bytes, output index).  The float formats are decoded in INTEGER arithmetic from
// their bit patterns (round to nearest even, clamp), so host and device cannot differ and no floating-point mode matters.
//
// The kernel is resample_i16_kernel's: one workgroup per 256 consecutive outputs of one piece, the block's input span decoded
// and down-mixed into LDS as int32 once, every lane walking the taps of its phase in the [tap][phase] table.  What differs: the
// raw arena is BYTES (a 24-bit 3-channel frame is 9 of them, at any alignment): a sample is loaded as one naturally aligned
// unit where the piece's first byte is aligned to the sample size and byte by byte otherwise, never wider than its alignment (a
// big-endian sample is that one load byte-swapped, or its bytes assembled the other way round: uniform per piece);
// the finish divides by D (a shift by 38 and one 32-bit floor division by the channel count, which is the same number);
// L goes up to 640.
#include <math.h>

#include "nafp_common.h"

struct nafp_ingest {
    int fs_in, fs_out, L, M, half, T;
    int span_cap;              // LDS ints a block may need
    int32_t* d_tab;            // [T][L]
};

namespace nafp {

constexpr int IG_BLOCK = 256;
constexpr int IG_MAX_L = 640;
constexpr int IG_MAX_RATE = 192000;
constexpr int IG_MAX_CHANNELS = 8;
constexpr int IG_LDS_BYTES = 64 * 1024;
constexpr int64_t IG_MAX_INDEX = (int64_t)1 << 40;     // frames / outputs per file: n * M + half stays far inside int64

struct IgGeom { int L, M, half, T, span_cap; };

static int ig_geometry(int fs_in, int fs_out, IgGeom* g) {
    if (fs_in <= 0 || fs_out <= 0) return NAFP_ERR_INVALID_ARG;
    if (fs_in > IG_MAX_RATE || fs_out > IG_MAX_RATE) return NAFP_ERR_UNSUPPORTED;
    if (fs_in == fs_out) { *g = IgGeom{1, 1, 0, 1, IG_BLOCK + 1}; return NAFP_OK; }   // the channel average alone: hq = {2^30}
    int a = fs_in, b = fs_out;
    while (b) { const int r = a % b; a = b; b = r; }
    const int L = fs_out / a, M = fs_in / a;
    if (L > IG_MAX_L) return NAFP_ERR_UNSUPPORTED;
    // half = ceil(32 fv / (2 fc)) with fc = 0.95 lo / 2 and lo the lower rate, in integers: 640 fv / (19 lo); fv <= 192000 * 640
    const int64_t lo = fs_in < fs_out ? fs_in : fs_out;
    const int64_t fv = (int64_t)fs_in * L, den = 19 * lo;
    const int64_t half = (640 * fv + den - 1) / den;
    const int64_t T = (2 * half + 1 + L - 1) / L;
    // jb of the last output of a block minus jb of its first <= ceil((IG_BLOCK - 1) M / L); + T taps below the first
    const int64_t span_cap = ((int64_t)(IG_BLOCK - 1) * M + L - 1) / L + T + 1;
    if (span_cap * (int64_t)sizeof(int32_t) > IG_LDS_BYTES) return NAFP_ERR_UNSUPPORTED;      // (this bounds T and half too)
    *g = IgGeom{L, M, (int)half, (int)T, (int)span_cap};
    return NAFP_OK;
}

static double ig_bessel_i0(double x) {                  // sum_k ((x/2)^k / k!)^2
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// hq[v], v in [-half, half] (0 outside).  For fs_in > fs_out every expression is resample.hip's, operand for operand.
struct IgDesign {
    IgGeom g; double r, gain, inv_i0;
    IgDesign(const IgGeom& g_, int fs_in, int fs_out) : g(g_) {
        const int lo = fs_in < fs_out ? fs_in : fs_out;
        r = 0.95 * (double)lo / ((double)fs_in * (double)g.L);           // 2 fc / fv
        gain = r * (double)g.L;
        inv_i0 = 1.0 / ig_bessel_i0(8.6);
    }
    int32_t hq(int64_t v) const {
        if (v < -g.half || v > g.half) return 0;
        if (g.half == 0) return (int32_t)1 << 30;
        const double x = M_PI * (r * (double)v);
        const double sinc = v == 0 ? 1.0 : sin(x) / x;
        const double u = (double)v / (double)g.half;
        const double w = ig_bessel_i0(8.6 * sqrt(fmax(0.0, 1.0 - u * u))) * inv_i0;
        return (int32_t)llround(sinc * w * gain * 1073741824.0);
    }
};

__host__ __device__ inline int64_t ig_floor_div(int64_t a, int64_t b) { int64_t q = a / b; if ((a % b != 0) && ((a < 0) != (b < 0))) --q; return q; }

// frames [first, last) of a file of n_in frames that the outputs [n0, n1) touch (first == last: none)
__host__ __device__ inline void ig_input_range(int64_t n0, int64_t n1, int64_t n_in, int L, int M, int half, int64_t* first, int64_t* last) {
    int64_t lo = -ig_floor_div(-(n0 * M - half), L);            // ceil
    if (lo < 0) lo = 0;
    int64_t hi = n1 > n0 ? ig_floor_div((n1 - 1) * M + half, L) + 1 : 0;
    if (hi > n_in) hi = n_in;
    if (hi <= lo) { lo = lo < n_in ? lo : n_in; hi = lo; }
    *first = lo; *last = hi;
}

// bytes of one sample of a format code; 0: not a format
__host__ __device__ inline int ig_sample_bytes(int format) {
    switch (format) {
        case NAFP_INGEST_U8: case NAFP_INGEST_S8: return 1;
        case NAFP_INGEST_S16: case NAFP_INGEST_S16 | NAFP_INGEST_BE: return 2;
        case NAFP_INGEST_S24: case NAFP_INGEST_S24 | NAFP_INGEST_BE: return 3;
        case NAFP_INGEST_S32: case NAFP_INGEST_S32 | NAFP_INGEST_BE: return 4;
        case NAFP_INGEST_F32: case NAFP_INGEST_F32 | NAFP_INGEST_BE: return 4;
        case NAFP_INGEST_F64: case NAFP_INGEST_F64 | NAFP_INGEST_BE: return 8;
    }
    return 0;
}

// the `bytes` low bytes of u in the opposite order
__host__ __device__ inline uint64_t ig_reverse(uint64_t u, int bytes) {
    uint64_t r = 0;
    for (int b = 0; b < bytes; ++b, u >>= 8) r = (r << 8) | (u & 0xff);
    return r;
}

// clamp(rint(x * 2^23), -2^23, 2^23 - 1) of the IEEE value with sign `neg`, biased exponent `e` (bias `bias`, all-ones `emax`) and
// `mbits` mantissa bits `man`, in integers: NaN -> 0, infinities clamp, zeros and denormals -> 0.
__host__ __device__ inline int32_t ig_float_q(bool neg, int e, uint64_t man, int bias, int emax, int mbits) {
    if (e == emax) return man ? 0 : (neg ? -8388608 : 8388607);
    if (e == 0) return 0;                                         // |x| < 2^-126: far below half a step
    if (e >= bias) return neg ? -8388608 : 8388607;               // |x| >= 1
    // |x| * 2^23 = sig * 2^(e - bias - mbits + 23), sig = 2^mbits | man, the exponent negative here
    const int s = bias + mbits - 23 - e;                          // >= mbits - 22 >= 1
    if (s > mbits + 2) return 0;                                  // below 1/4
    const uint64_t sig = ((uint64_t)1 << mbits) | man;
    uint64_t k = sig >> s;
    const uint64_t rem = sig & (((uint64_t)1 << s) - 1), tie = (uint64_t)1 << (s - 1);
    if (rem > tie || (rem == tie && (k & 1))) ++k;                // to nearest, ties to even
    if (neg) return -(int32_t)k;                                  // k <= 2^23
    return k > 8388607 ? 8388607 : (int32_t)k;
}

// the canonical sample from the little-endian value `u` of the bytes of a little-endian format code (or NAFP_INGEST_S8)
__host__ __device__ inline int32_t ig_decode_le(int format, uint64_t u) {
    switch (format) {
        case NAFP_INGEST_U8: return ((int32_t)(u & 0xff) - 128) * 65536;
        case NAFP_INGEST_S8: return (int32_t)(int8_t)(uint8_t)u * 65536;
        case NAFP_INGEST_S16: return (int32_t)(int16_t)(uint16_t)u * 256;
        case NAFP_INGEST_S24: return (int32_t)((uint32_t)u << 8) >> 8;
        case NAFP_INGEST_S32: {
            const int64_t v = ((int64_t)(int32_t)(uint32_t)u + 128) >> 8;
            return v > 8388607 ? 8388607 : (int32_t)v;
        }
        case NAFP_INGEST_F32: {
            const uint32_t b = (uint32_t)u;
            return ig_float_q((b >> 31) != 0, (int)((b >> 23) & 0xff), b & 0x7fffffu, 127, 255, 23);
        }
        case NAFP_INGEST_F64:
            return ig_float_q((u >> 63) != 0, (int)((u >> 52) & 0x7ff), u & (((uint64_t)1 << 52) - 1), 1023, 2047, 52);
    }
    return 0;
}

// the canonical sample from the value `u` of its ig_sample_bytes(format) bytes as the file holds them, first byte lowest: a
// NAFP_INGEST_BE format is the little-endian rule on the reversed bytes.  (The kernel reverses while it loads, ig_load, and calls
// ig_decode_le itself.)
__host__ __device__ inline int32_t ig_decode(int format, uint64_t u) {
    if (format & NAFP_INGEST_BE) return ig_decode_le(format & ~NAFP_INGEST_BE, ig_reverse(u, ig_sample_bytes(format)));
    return ig_decode_le(format, u);
}

// 0: consistent; 1: the output range is outside the arena (nothing may be written); 2: anything else (its outputs are zeroed)
__host__ __device__ inline int ig_piece_fault(const nafp_ingest_piece& pc, int L, int M, int half, int64_t raw_size, int64_t out_samples) {
    if (pc.n_out < 0 || pc.out_off < 0 || pc.out_off > out_samples || pc.n_out > out_samples - pc.out_off) return 1;
    const int bps = ig_sample_bytes(pc.format);
    if (bps == 0 || pc.channels < 1 || pc.channels > IG_MAX_CHANNELS) return 2;
    if (pc.n_in < 0 || pc.n_in > IG_MAX_INDEX || pc.out0 < 0 || pc.out0 > IG_MAX_INDEX) return 2;
    if (pc.frame0 < 0 || pc.frame0 > pc.n_in || pc.n_frames < 0 || pc.n_frames > pc.n_in - pc.frame0) return 2;
    if (pc.raw_off < 0 || pc.raw_off > raw_size || pc.n_frames > (raw_size - pc.raw_off) / (pc.channels * bps)) return 2;
    const int64_t n_total = (pc.n_in * L + M - 1) / M;
    if (pc.out0 + pc.n_out > n_total) return 2;
    int64_t lo, hi;
    ig_input_range(pc.out0, pc.out0 + pc.n_out, pc.n_in, L, M, half, &lo, &hi);
    if (hi > lo && (pc.frame0 > lo || pc.frame0 + pc.n_frames < hi)) return 2;      // a needed frame was not uploaded
    return 0;
}

// the little-endian value of the BPS bytes at p -- with BE of those bytes in the opposite order: a byte swap of the one load, or
// the bytes assembled the other way round; `aligned`: p is a multiple of BPS (never true for 3), so one load of that width is legal
template <int BPS, bool BE>
__device__ __forceinline__ uint64_t ig_load(const uint8_t* p, bool aligned) {
    if (BPS == 2 && aligned) return BE ? __builtin_bswap16(*(const uint16_t*)p) : *(const uint16_t*)p;
    if (BPS == 4 && aligned) return BE ? __builtin_bswap32(*(const uint32_t*)p) : *(const uint32_t*)p;
    if (BPS == 8 && aligned) return BE ? __builtin_bswap64(*(const uint64_t*)p) : *(const uint64_t*)p;
    uint64_t u = 0;
#pragma unroll
    for (int b = 0; b < BPS; ++b) u |= (uint64_t)p[b] << (8 * (BE ? BPS - 1 - b : b));
    return u;
}

// m of one frame: the sum of its channels' canonical samples; `format` is a little-endian code (BE: its bytes come reversed)
template <int BPS, bool BE>
__device__ __forceinline__ int32_t ig_frame(const uint8_t* p, int format, int ch, bool aligned) {
    int32_t v = 0;
    for (int c = 0; c < ch; ++c) v += ig_decode_le(format, ig_load<BPS, BE>(p + c * BPS, aligned));
    return v;
}

__global__ __launch_bounds__(IG_BLOCK) void ingest_i16_kernel(const int32_t* __restrict__ tab, int L, int M, int half, int T, int span_cap,
                                                              const uint8_t* __restrict__ raw, int64_t raw_size,
                                                              const nafp_ingest_piece* __restrict__ pieces,
                                                              int16_t* __restrict__ out, int64_t out_samples) {
    extern __shared__ __attribute__((aligned(16))) int32_t s_in[];         // m[jlo .. jlo + span)
    const nafp_ingest_piece pc = pieces[blockIdx.y];
    const int tid = threadIdx.x;
    const int fault = ig_piece_fault(pc, L, M, half, raw_size, out_samples);
    if (fault == 1) return;
    const int ch = pc.channels;
    const int bps = ig_sample_bytes(pc.format);                            // 0 only with fault == 2: nothing is read then
    const int path = (pc.format & NAFP_INGEST_BE) ? bps + 8 : bps;         // uniform over the piece: no wave diverges on it
    const int format = pc.format & ~NAFP_INGEST_BE;
    const int64_t frame_bytes = (int64_t)ch * bps;
    const uint8_t* base = raw + pc.raw_off;
    // the frame stride is a multiple of the sample size, so every sample of the piece is aligned as its first byte is
    const bool aligned = bps > 0 && bps != 3 && ((uintptr_t)base % (uintptr_t)bps) == 0;
    for (int64_t b0 = (int64_t)blockIdx.x * IG_BLOCK; b0 < pc.n_out; b0 += (int64_t)gridDim.x * IG_BLOCK) {
        const int cnt = (int)(pc.n_out - b0 < IG_BLOCK ? pc.n_out - b0 : IG_BLOCK);
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
        for (int i = tid; i < (int)span; i += IG_BLOCK) {
            const int64_t k = jlo + i - pc.frame0;                         // index into the uploaded frames
            int32_t v = 0;
            if (k >= 0 && k < pc.n_frames) {                               // inside [raw_off, raw_off + n_frames * frame_bytes) <= raw_size
                const uint8_t* p = base + k * frame_bytes;
                switch (path) {                                            // bps, + 8 for a big-endian piece
                    case 1: v = ig_frame<1, false>(p, format, ch, aligned); break;
                    case 2: v = ig_frame<2, false>(p, format, ch, aligned); break;
                    case 3: v = ig_frame<3, false>(p, format, ch, aligned); break;
                    case 4: v = ig_frame<4, false>(p, format, ch, aligned); break;
                    case 8: v = ig_frame<8, false>(p, format, ch, aligned); break;
                    case 10: v = ig_frame<2, true>(p, format, ch, aligned); break;
                    case 11: v = ig_frame<3, true>(p, format, ch, aligned); break;
                    case 12: v = ig_frame<4, true>(p, format, ch, aligned); break;
                    default: v = ig_frame<8, true>(p, format, ch, aligned); break;
                }
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
            // floor((acc + D / 2) / D), D = ch * 2^38: floor(floor(a / 2^38) / ch) is floor(a / (2^38 ch)) for a positive ch
            const int32_t w = (int32_t)((acc + ((int64_t)ch << 37)) >> 38);        // |.| < 2^21
            int32_t y = w / ch;
            if (w % ch != 0 && w < 0) --y;
            y = y < -32768 ? -32768 : (y > 32767 ? 32767 : y);
            o[tid] = (int16_t)y;
        }
    }
}

}  // namespace nafp

using namespace nafp;

extern "C" int nafp_ingest_geometry(int fs_in, int fs_out, int* L, int* M, int* half, int* T) {
    IgGeom g;
    const int st = ig_geometry(fs_in, fs_out, &g);
    if (st != NAFP_OK) return st;
    if (L) *L = g.L;
    if (M) *M = g.M;
    if (half) *half = g.half;
    if (T) *T = g.T;
    return NAFP_OK;
}

extern "C" int nafp_ingest_table_host(int fs_in, int fs_out, int32_t* table_host) {
    IgGeom g;
    const int st = ig_geometry(fs_in, fs_out, &g);
    if (st != NAFP_OK) return st;
    if (!table_host) return NAFP_ERR_INVALID_ARG;
    const IgDesign d(g, fs_in, fs_out);
    for (int p = 0; p < g.L; ++p)
        for (int t = 0; t < g.T; ++t) table_host[(int64_t)p * g.T + t] = d.hq((int64_t)p + (int64_t)t * g.L - g.half);
    return NAFP_OK;
}

extern "C" int64_t nafp_ingest_n_out(int64_t n_in, int fs_in, int fs_out) {
    IgGeom g;
    if (n_in < 0 || n_in > IG_MAX_INDEX || ig_geometry(fs_in, fs_out, &g) != NAFP_OK) return -1;
    return (n_in * g.L + g.M - 1) / g.M;
}

extern "C" int nafp_ingest_input_range(int64_t n0, int64_t n1, int64_t n_in, int fs_in, int fs_out, int64_t* first, int64_t* last) {
    IgGeom g;
    const int st = ig_geometry(fs_in, fs_out, &g);
    if (st != NAFP_OK) return st;
    if (!first || !last || n0 < 0 || n1 < n0 || n1 > IG_MAX_INDEX || n_in < 0 || n_in > IG_MAX_INDEX) return NAFP_ERR_INVALID_ARG;
    ig_input_range(n0, n1, n_in, g.L, g.M, g.half, first, last);
    return NAFP_OK;
}

extern "C" int nafp_ingest_decode_host(int format, const void* bytes, int64_t n_samples, int32_t* q_out) {
    const int bps = ig_sample_bytes(format);
    if (bps == 0) return NAFP_ERR_UNSUPPORTED;
    if (n_samples < 0 || (n_samples > 0 && (!bytes || !q_out))) return NAFP_ERR_INVALID_ARG;
    const uint8_t* p = (const uint8_t*)bytes;
    for (int64_t i = 0; i < n_samples; ++i, p += bps) {
        uint64_t u = 0;
        for (int b = 0; b < bps; ++b) u |= (uint64_t)p[b] << (8 * b);
        q_out[i] = ig_decode(format, u);
    }
    return NAFP_OK;
}

extern "C" int nafp_ingest_check_pieces_host(int fs_in, int fs_out, const nafp_ingest_piece* pieces_host, int64_t n_pieces,
                                             int64_t raw_size, int64_t out_samples) {
    IgGeom g;
    const int st = ig_geometry(fs_in, fs_out, &g);
    if (st != NAFP_OK) return st;
    if (n_pieces < 0 || raw_size < 0 || out_samples < 0 || (n_pieces > 0 && !pieces_host)) return NAFP_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n_pieces; ++i) {
        const nafp_ingest_piece& pc = pieces_host[i];
        if (ig_sample_bytes(pc.format) == 0 || pc.channels < 1 || pc.channels > IG_MAX_CHANNELS) return NAFP_ERR_UNSUPPORTED;
        if (ig_piece_fault(pc, g.L, g.M, g.half, raw_size, out_samples) != 0) return NAFP_ERR_INVALID_ARG;
    }
    return NAFP_OK;
}

extern "C" int nafp_ingest_create(nafp_ingest** plan, int fs_in, int fs_out) {
    if (!plan) return NAFP_ERR_INVALID_ARG;
    *plan = nullptr;
    IgGeom g;
    const int st = ig_geometry(fs_in, fs_out, &g);                          // refuses a block span beyond 64 KB of LDS too
    if (st != NAFP_OK) return st;
    const IgDesign d(g, fs_in, fs_out);
    std::vector<int32_t> tab((size_t)g.T * g.L);                           // device layout [tap][phase]
    for (int t = 0; t < g.T; ++t)
        for (int p = 0; p < g.L; ++p) tab[(size_t)t * g.L + p] = d.hq((int64_t)p + (int64_t)t * g.L - g.half);
    nafp_ingest* h = new nafp_ingest{fs_in, fs_out, g.L, g.M, g.half, g.T, g.span_cap, nullptr};
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

extern "C" int nafp_ingest_destroy(nafp_ingest* plan) {
    if (!plan) return NAFP_OK;
    if (plan->d_tab) (void)hipFree(plan->d_tab);
    delete plan;
    return NAFP_OK;
}

extern "C" int nafp_ingest_i16(nafp_ingest* plan, const uint8_t* raw_bytes, int64_t raw_size, const nafp_ingest_piece* pieces_dev,
                               int64_t n_pieces, int16_t* out, int64_t out_samples, void* stream) {
    if (!plan || !raw_bytes || !out || n_pieces < 0 || raw_size < 0 || out_samples < 0 || (n_pieces > 0 && !pieces_dev))
        return NAFP_ERR_INVALID_ARG;
    if (n_pieces == 0 || out_samples == 0) return NAFP_OK;
    const int lds = plan->span_cap * (int)sizeof(int32_t);                 // <= 64 KB (ig_geometry)
    // blockIdx.y = piece; the blocks of a row stride over the piece's 256-output blocks.  The row is sized for twice the mean
    // piece, so that equal pieces take one step; the bytes written do not depend on it.
    const int64_t blocks = (out_samples + IG_BLOCK - 1) / IG_BLOCK;
    for (int64_t p0 = 0; p0 < n_pieces; p0 += 32768) {
        const int64_t np = n_pieces - p0 < 32768 ? n_pieces - p0 : 32768;
        int64_t gx = 2 * ((blocks + n_pieces - 1) / n_pieces);
        gx = gx < 1 ? 1 : (gx > 8192 ? 8192 : gx);
        ingest_i16_kernel<<<dim3((unsigned)gx, (unsigned)np), IG_BLOCK, lds, (hipStream_t)stream>>>(
            plan->d_tab, plan->L, plan->M, plan->half, plan->T, plan->span_cap, raw_bytes, raw_size, pieces_dev + p0, out, out_samples);
        NAFP_LAUNCH_CHECK();
    }
    return NAFP_OK;
}
