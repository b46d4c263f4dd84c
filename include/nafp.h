/*
 * nafp.h -- C ABI of libnafp.so: the MI355X (gfx950) hot path of neural audio
 * fingerprinting: 1-s segment -> log-mel -> conv encoder -> 128-d fingerprint
 * (generate), the contrastive train step around it (batch assembly + time-domain
 * augmentation, spec-augment, NT-Xent / online-triplet loss, the encoder's backward
 * pass, Adam / LAMB), and the exact search that consumes the fingerprints.
 *
 * The reference (mimbres/neural-audio-fp) is pure Python on TensorFlow; it has no
 * FFI of its own.  Each entry point below replaces the device work behind one
 * Python-level operator of the reference, cited as file:line of the reference
 * checkout.  INTEGRATION.md shows the ctypes stub a maintainer of the reference
 * would add to route those operators here.
 *
 * Conventions
 *   - every function returns an int status (NAFP_OK == 0); no C++ exception
 *     crosses this boundary;
 *   - all data pointers are CALLER-OWNED DEVICE pointers unless the name ends in
 *     `_host`; the library allocates only what hangs off an opaque handle
 *     (tables, packed weights) and frees it in the matching *_destroy;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *     all work is enqueued asynchronously on it;
 *   - a handle is re-entrant across handles, not thread-safe per handle (the
 *     reference drives the device from one host thread: generate.py:176-181).
 */
#ifndef NAFP_H
#define NAFP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NAFP_ABI_VERSION 1

enum {
    NAFP_OK = 0,
    NAFP_ERR_INVALID_ARG = 1,
    NAFP_ERR_UNSUPPORTED = 2,   /* geometry the kernels are not built for */
    NAFP_ERR_HIP = 3,           /* a HIP runtime call failed; see nafp_last_hip_error */
    NAFP_ERR_WORKSPACE = 4,     /* caller workspace too small */
    NAFP_ERR_NO_WEIGHTS = 5     /* encoder forward before set_weights */
};

typedef struct nafp_melspec nafp_melspec;
typedef struct nafp_encoder nafp_encoder;

int nafp_abi_version(void);
const char* nafp_status_string(int status);
/* hipError_t (as int) of the most recent failing HIP call on this thread. */
int nafp_last_hip_error(void);
/* CRC-32C (Castagnoli) of n host bytes, continuing from `crc` (0 to start): the checksum TensorFlow's TensorBundle
 * stores per tensor and per index block; used by the reader of the reference's checkpoints (model/generate.py:26-52). */
uint32_t nafp_crc32c_host(const void* data_host, int64_t n, uint32_t crc);

/* ------------------------------------------------------------------------
 * Front end: Melspec_layer (model/fp/melspec/melspectrogram.py:10-112)
 * ---------------------------------------------------------------------- */

/* Host-side Slaney mel filter bank, float32, row-major (n_mels, n_fft/2+1).
 * Replaces librosa.filters.mel reached via kapre ApplyFilterbank
 * (melspectrogram.py:93-98).  No GPU needed. */
int nafp_mel_filterbank_host(int fs, int n_fft, int n_mels, float f_min, float f_max,
                             float* out_host);

/* Plan for get_melspec_layer(cfg) (melspectrogram.py:115-141).  seg_len = FS*DUR.
 * Supported: n_fft == 1024, hop == 256, n_mels % 64 == 0 && n_mels <= 256,
 * every mel filter <= 8 taps wide. */
int nafp_melspec_create(nafp_melspec** plan, int fs, int seg_len, int n_fft, int hop,
                        int n_mels, float f_min, float f_max);
/* The same plan for ANY geometry of the front end's config keys (MODEL.FS, STFT_WIN, STFT_HOP, N_MELS, F_MIN, F_MAX, DUR), which
 * the reference hands to kapre and librosa unrestricted (melspectrogram.py:115-141).  flags:
 *   0                            exactly nafp_melspec_create
 *   NAFP_MELSPEC_ANY_GEOMETRY    a geometry nafp_melspec_create refuses is served by the general kernel (csrc/melspec_any.hip);
 *                                one it serves keeps the tuned kernel
 *   NAFP_MELSPEC_FORCE_GENERAL   the general kernel for those as well (tests, A/B runs)
 * General kernel: n_fft a power of two in 128 ... 4096, 1 <= hop <= n_fft (any value: no divisor of n_fft, no power of two needed),
 * 1 <= n_mels <= 512, seg_len <= 2^22 (shorter than n_fft included), any fs and f_min < f_max, filters of any width; an all-zero
 * filter yields log10(0.06).  Everything else is NAFP_ERR_UNSUPPORTED (bad pointers / sizes / flag bits NAFP_ERR_INVALID_ARG), decided
 * before any HIP call.  Either kind of plan goes to every nafp_melspec_* entry point below and has the same contract: float32 or
 * int16 input with the same bytes out, windows, NAFP_MELSPEC_DEFER, a segment's raw log-mel a pure function of its samples.
 *
 * nafp_melspec_plan_host: host only (works in a process without a GPU), what create_ex would build.  Same status as create_ex;
 * record_host receives NAFP_MELSPEC_PLAN_FIELDS values:
 *   [0] kernel: 0 tuned (melspec_r16_kernel), 1 general (melspec_any_kernel)   [1] n_frames = 1 + seg_len / hop   [2] bins = n_fft / 2 + 1
 *   [3] non-zero weights of the mel bank   [4] taps of its widest filter   [5] its all-zero filters   [6] frames per workgroup
 *   [7] dynamic LDS bytes per workgroup   [8] chunks of [6] frames per segment (grid y; above 65,535 a workgroup takes several)   [9] frame pairs a workgroup transforms at a time.
 * tests/test_melspec_any_host.py holds the records.  nafp_melspec_kernel: [0] of a built plan. */
#define NAFP_MELSPEC_ANY_GEOMETRY 1
#define NAFP_MELSPEC_FORCE_GENERAL 2
#define NAFP_MELSPEC_PLAN_FIELDS 10
int nafp_melspec_create_ex(nafp_melspec** plan, int fs, int seg_len, int n_fft, int hop, int n_mels,
                           float f_min, float f_max, int flags);
int nafp_melspec_plan_host(int fs, int seg_len, int n_fft, int hop, int n_mels, float f_min, float f_max,
                           int flags, int64_t* record_host);
int nafp_melspec_kernel(const nafp_melspec* plan);
int nafp_melspec_destroy(nafp_melspec* plan);
int nafp_melspec_n_frames(const nafp_melspec* plan);   /* 1 + seg_len/hop   (32)  */
int nafp_melspec_n_mels(const nafp_melspec* plan);

/* Melspec_layer.call (melspectrogram.py:102-112).
 *   audio      (n_seg, seg_len) float32 or int16 PCM (int16 is scaled by 2^-15 as
 *              load_audio does, model/utils/audio_utils.py:245-246)
 *   group_size the reference subtracts the max over the WHOLE device batch
 *              (melspectrogram.py:108); consecutive runs of group_size segments
 *              (last ragged) form one such batch.  <= 0 means one group.
 *   segment_norm  bit 0: FEAT == 'melspec_maxnorm' (melspectrogram.py:110-111);
 *              bit 1 (NAFP_MELSPEC_DEFER): stop before melspectrogram.py:108 -- feat is the raw log10 mel and
 *              group_stat the (max, min) per group; nafp_encoder_forward_raw finishes the layer inside its first
 *              conv (one kernel and one round trip of the feature tensor through HBM fewer; same result)
 *   feat       out, (n_seg, n_mels, n_frames) float32 == the reference's
 *              (B, n_mels, n_frames, 1)
 *   group_stat scratch, 2*ceil(n_seg/group_size) floats (raw max / min per group)
 */
#define NAFP_MELSPEC_DEFER 2
int nafp_melspec_forward_f32(nafp_melspec* plan, const float* audio, int64_t n_seg,
                             int group_size, int segment_norm, float* feat,
                             float* group_stat, void* stream);
int nafp_melspec_forward_i16(nafp_melspec* plan, const int16_t* audio, int64_t n_seg,
                             int group_size, int segment_norm, float* feat,
                             float* group_stat, void* stream);

/* Finish a deferred call in place: feat <- max(feat - group max, -80) [, segment normalisation]
 * (melspectrogram.py:108-111), for consumers other than nafp_encoder_forward_raw. */
int nafp_melspec_finish(nafp_melspec* plan, float* feat, const float* group_stat, int64_t n_seg, int group_size,
                        int segment_norm, void* stream);

/* The same layer fed by WINDOWS of one int16 PCM arena instead of a materialised (n_seg, seg_len)
 * array: segment i starts at sample seg_offset[i] of `pcm` and has seg_valid[i] (<= seg_len) real
 * samples, the rest being the zero tail.  Replaces the segment assembly of the reference's loader
 * (get_fns_seg_list + load_audio per segment, model/utils/audio_utils.py:140-264; np.vstack per
 * batch, model/utils/dataloader_keras.py:389-397): whole files are uploaded once and the 50 %
 * overlap between consecutive segments (HOP = 0.5 s) is never duplicated.  All device pointers. */
int nafp_melspec_forward_windows_i16(nafp_melspec* plan, const int16_t* pcm, const int64_t* seg_offset,
                                     const int32_t* seg_valid, int64_t n_seg, int group_size,
                                     int segment_norm, float* feat, float* group_stat, void* stream);

/* ------------------------------------------------------------------------
 * Ingest at any sample rate (csrc/resample.hip; numpy restatement tests/_resample_ref.py).  The reference raises on
 * anything but FS-rate mono files (model/utils/audio_utils.py:160-169) and leaves the conversion to an external tool;
 * this resampler sits between the PCM upload and nafp_melspec_forward_windows_i16.  EXACT INTEGER ARITHMETIC: an output
 * sample is a pure function of (file samples, output index), whatever shares its piece, block or launch.
 *
 * Ratio: g = gcd(fs_in, fs_out), L = fs_out / g, M = fs_in / g.  Supported: fs_in > fs_out with L <= 320 and
 * fs_in <= 192000 (11025 .. 192000 -> 8000 among them); fs_in == fs_out (L = M = 1, half = 0, T = 1: the filter is the
 * single tap 2^30, i.e. the identity for 1 channel and (l + r + 1) >> 1 for 2).  1 or 2 channels, 16-bit PCM.
 * Filter: Kaiser-windowed sinc designed in float64 at the virtual rate fv = fs_in * L, cut-off fc = 0.95 fs_out / 2,
 * half = ceil(32 fv / (2 fc)) = ceil(640 fv / (19 fs_out)) (32 zero crossings a side),
 *   h[v]  = sinc(2 fc v / fv) * I0(8.6 sqrt(1 - (v / half)^2)) / I0(8.6) * (2 fc / fv) * L,   v in [-half, half]
 *   hq[v] = round(h[v] * 2^30) as int32,   T = ceil((2 half + 1) / L) taps per phase.
 * Output: n_out = ceil(n_in * L / M); m[j] = x[j] (1 channel) or l[j] + r[j] (2 channels); samples outside the file are zero;
 *   acc[n] = sum_j hq[n M - j L] * m[j]  over |n M - j L| <= half   (exact in int64: sum |hq| / 2^30 <= 2.23 per phase)
 *   y[n]   = clamp((acc[n] + 2^(s-1)) >> s, -32768, 32767),  s = 30 (1 channel) / 31 (2 channels), arithmetic shift.
 * Status: a ratio outside the list NAFP_ERR_UNSUPPORTED, null pointers / negative sizes NAFP_ERR_INVALID_ARG, all before
 * any GPU call.
 * ---------------------------------------------------------------------- */
typedef struct nafp_resample nafp_resample;

/* A run of consecutive output samples of one file.  The raw frames uploaded for it are only what its outputs need
 * (nafp_resample_input_range); a frame outside them but inside the file is a caller error and is never read. */
typedef struct nafp_resample_piece {
    int64_t raw_off;     /* int16 index in the raw arena of the first uploaded frame (interleaved l, r for 2 channels) */
    int64_t frame0;      /* which frame of the file that is */
    int64_t n_frames;    /* frames uploaded */
    int64_t n_in;        /* frames of the whole file */
    int64_t out0;        /* index in the file's resampled stream of the first output */
    int64_t out_off;     /* int16 index in the output arena of that output */
    int32_t n_out;       /* outputs */
    int32_t channels;    /* 1 or 2 */
} nafp_resample_piece;

/* Host only. */
int nafp_resample_geometry(int fs_in, int fs_out, int* L, int* M, int* half, int* T);
/* Host only: the canonical table (L, T) int32, [phase p][tap t] = hq[p + t L - half], zero where out of range.  Output n
 * has phase p = (n M + half) mod L and, with jb = (n M + half) div L, is sum_t table[p][t] * m[jb - t].  (The device
 * layout is the library's own.) */
int nafp_resample_table_host(int fs_in, int fs_out, int32_t* table_host);
int64_t nafp_resample_n_out(int64_t n_in, int fs_in, int fs_out);          /* -1: unsupported ratio / negative n_in */
/* Host only: the frames [*first, *last) of a file of n_in frames that the outputs [n0, n1) read (first == last: none). */
int nafp_resample_input_range(int64_t n0, int64_t n1, int64_t n_in, int fs_in, int fs_out, int64_t* first,
                              int64_t* last);
/* Host only: the checks the kernel makes per piece, on a host copy of the list, before it is uploaded: indices inside
 * raw_samples / out_samples, the outputs inside the file's n_out, every frame they read uploaded.  NAFP_ERR_INVALID_ARG
 * for an inconsistent piece, NAFP_ERR_UNSUPPORTED for a channel count other than 1 or 2. */
int nafp_resample_check_pieces_host(int fs_in, int fs_out, const nafp_resample_piece* pieces_host, int64_t n_pieces,
                                    int64_t raw_samples, int64_t out_samples);
/* The plan owns the device table. */
int nafp_resample_create(nafp_resample** plan, int fs_in, int fs_out);
int nafp_resample_destroy(nafp_resample* plan);
/* raw (raw_samples int16) -> out (out_samples int16) for the n_pieces pieces of pieces_dev, all device pointers.  Every
 * index derived from a piece is checked on the device against raw_samples / out_samples: an inconsistent piece is
 * skipped, its outputs zeroed (nothing is written for one whose output range leaves the arena).  Int16 outside the
 * pieces' output ranges is not touched. */
int nafp_resample_i16(nafp_resample* plan, const int16_t* raw, int64_t raw_samples,
                      const nafp_resample_piece* pieces_dev, int64_t n_pieces, int16_t* out, int64_t out_samples,
                      void* stream);

/* ------------------------------------------------------------------------
 * Ingest of any PCM / IEEE-float WAV, 1 to 8 channels, at any supported rate in EITHER direction (csrc/ingest.hip; numpy
 * restatement tests/_ingest_ref.py).  The general sibling of nafp_resample_*, which is unchanged;
 * for 16-bit files with 1 or 2 channels at a higher rate the two write the same bytes.  EXACT INTEGER ARITHMETIC: an output
 * sample is a pure function of (file bytes, output index), whatever shares its piece, block or launch.
 *
 * Canonical sample q: a signed integer at 2^-23 of full scale, |q| <= 2^23, from the little-endian sample as the file holds it
 * (for WAVE_FORMAT_EXTENSIBLE the container of block_align / channels bytes: samples are MSB-justified in it):
 *   NAFP_INGEST_U8   unsigned 8-bit PCM       q = (u - 128) << 16
 *   NAFP_INGEST_S16  16-bit PCM               q = x << 8
 *   NAFP_INGEST_S24  24-bit PCM, 3 bytes      q = x (sign-extended)
 *   NAFP_INGEST_S32  32-bit PCM               q = min((x + 128) >> 8, 2^23 - 1), arithmetic shift, the sum formed in 64 bits
 *   NAFP_INGEST_F32 / NAFP_INGEST_F64  IEEE   NaN -> 0; otherwise q = clamp(rint(x * 2^23), -2^23, 2^23 - 1), ties to even, the
 *                                             clamp applied before the conversion to integer (infinities clamp, denormals give
 *                                             0); computed from the bit pattern in integers on host and device alike
 *   NAFP_INGEST_S8   signed 8-bit PCM         q = x << 16   (AIFF and AU hold 8-bit samples signed)
 *   NAFP_INGEST_BE   a flag on S16, S24, S32, F32 and F64 only (the codes 18 .. 22): the sample's bytes stand in the opposite
 *                    order, as AIFF / AIFF-C and AU hold them; q is the little-endian rule applied to the reversed bytes.
 * Every other value -- 0, 7, 9 .. 17, 23 and above, the flag on U8 or S8 -- is NAFP_ERR_UNSUPPORTED from every entry point.
 * Down-mix: m[j] = sum_c q[j][c] over the C = 1..8 channels of frame j, equal weights; the division by C is part of the
 * final rounding.
 * Ratio: g = gcd(fs_in, fs_out), L = fs_out / g, M = fs_in / g.  Supported: both rates <= 192000 and L <= 640, in either
 * direction (11025 -> 16000 is L = 640, M = 441), provided the input span of a 256-output block,
 * ceil(255 M / L) + T + 1 int32, fits 64 KB of LDS (otherwise NAFP_ERR_UNSUPPORTED from every entry point, plan creation
 * included); fs_in == fs_out is the identity geometry L = M = 1, half = 0, T = 1, the single tap 2^30.
 * Filter: nafp_resample_*'s design with the LOWER of the two rates in the place of fs_out: lo = min(fs_in, fs_out),
 * fv = fs_in * L, fc = 0.95 lo / 2, half = ceil(640 fv / (19 lo)),
 *   h[v]  = sinc(2 fc v / fv) * I0(8.6 sqrt(1 - (v / half)^2)) / I0(8.6) * (2 fc / fv) * L,   v in [-half, half]
 *   hq[v] = round(h[v] * 2^30) as int32,   T = ceil((2 half + 1) / L) taps per phase.
 * For fs_in > fs_out this is nafp_resample_table_host's table bit for bit.  Per phase sum |hq| / 2^30 < 2.5.
 * Output: n_out = ceil(n_in * L / M); samples outside the file are zero;
 *   acc[n] = sum_j hq[n M - j L] * m[j]  over |n M - j L| <= half     (exact in int64: |acc| <= 2^23 * 8 * 2.5 * 2^30 < 2^58)
 *   y[n]   = clamp(floor((acc[n] + D / 2) / D), -32768, 32767),   D = C * 2^38, floor division.
 * Status: a ratio, format or channel count outside the list NAFP_ERR_UNSUPPORTED, null pointers / negative sizes / an
 * inconsistent piece NAFP_ERR_INVALID_ARG, all before any GPU call.
 * ---------------------------------------------------------------------- */
typedef struct nafp_ingest nafp_ingest;

#define NAFP_INGEST_U8 1
#define NAFP_INGEST_S16 2
#define NAFP_INGEST_S24 3
#define NAFP_INGEST_S32 4
#define NAFP_INGEST_F32 5
#define NAFP_INGEST_F64 6
#define NAFP_INGEST_S8 8
#define NAFP_INGEST_BE 16 /* a flag: NAFP_INGEST_S16 .. NAFP_INGEST_F64 | NAFP_INGEST_BE, the codes 18 .. 22 */

/* A run of consecutive output samples of one file: nafp_resample_piece with a BYTE offset into a uint8 arena (any
 * alignment), a format code and 1..8 channels.  64 bytes. */
typedef struct nafp_ingest_piece {
    int64_t raw_off;     /* byte index in the raw arena of the first uploaded frame (frames interleaved as in the file) */
    int64_t frame0;      /* which frame of the file that is */
    int64_t n_frames;    /* frames uploaded */
    int64_t n_in;        /* frames of the whole file */
    int64_t out0;        /* index in the file's output stream of the first output */
    int64_t out_off;     /* int16 index in the output arena of that output */
    int32_t n_out;       /* outputs */
    int32_t channels;    /* 1 .. 8 */
    int32_t format;      /* NAFP_INGEST_* */
    int32_t reserved;
} nafp_ingest_piece;

/* Host only. */
int nafp_ingest_geometry(int fs_in, int fs_out, int* L, int* M, int* half, int* T);
/* Host only: the canonical table (L, T) int32, [phase p][tap t] = hq[p + t L - half], as nafp_resample_table_host. */
int nafp_ingest_table_host(int fs_in, int fs_out, int32_t* table_host);
int64_t nafp_ingest_n_out(int64_t n_in, int fs_in, int fs_out);            /* -1: unsupported ratio / negative n_in */
/* Host only: the frames [*first, *last) of a file of n_in frames that the outputs [n0, n1) read (first == last: none). */
int nafp_ingest_input_range(int64_t n0, int64_t n1, int64_t n_in, int fs_in, int fs_out, int64_t* first, int64_t* last);
/* Host only: q of n_samples consecutive samples of `format` at `bytes` (any alignment) -- the function the kernel decodes
 * with, compiled for the host. */
int nafp_ingest_decode_host(int format, const void* bytes, int64_t n_samples, int32_t* q_out);
/* Host only: the checks the kernel makes per piece.  NAFP_ERR_INVALID_ARG for an inconsistent piece, NAFP_ERR_UNSUPPORTED
 * for a format code or a channel count outside the contract. */
int nafp_ingest_check_pieces_host(int fs_in, int fs_out, const nafp_ingest_piece* pieces_host, int64_t n_pieces,
                                  int64_t raw_size, int64_t out_samples);
/* The plan owns the device table. */
int nafp_ingest_create(nafp_ingest** plan, int fs_in, int fs_out);
int nafp_ingest_destroy(nafp_ingest* plan);
/* raw_bytes (raw_size bytes) -> out (out_samples int16) for the n_pieces pieces of pieces_dev, all device pointers.  Every
 * index derived from a piece is checked on the device against raw_size / out_samples: an inconsistent piece is skipped, its
 * outputs zeroed (nothing is written for one whose output range leaves the arena).  No byte outside the two arenas is read
 * or written whatever a piece says; int16 outside the pieces' output ranges is not touched. */
int nafp_ingest_i16(nafp_ingest* plan, const uint8_t* raw_bytes, int64_t raw_size, const nafp_ingest_piece* pieces_dev,
                    int64_t n_pieces, int16_t* out, int64_t out_samples, void* stream);

/* ------------------------------------------------------------------------
 * Varispeed: model-rate 16-bit mono PCM -> model-rate 16-bit mono PCM played `sigma` times as fast, tempo and pitch together
 * (csrc/varispeed.hip; numpy restatement tests/_varispeed_ref.py).  Undoes the speed change of a
 * recording before it is fingerprinted; runs after the ingest of its launch.  EXACT INTEGER ARITHMETIC: an output sample is a
 * pure function of (the file's model-rate samples, the output index, the step), whatever shares its piece, block or launch.
 *
 * Step: an unsigned Q24 count of input samples per output sample, sigma = step / 2^24.  Supported: NAFP_VARISPEED_STEP_MIN <=
 * step <= NAFP_VARISPEED_STEP_MAX (sigma 0.8 .. 1.25).  A recording played s times too fast is undone by step =
 * round(2^24 / s); the speed reported back is 2^24 / step.
 * Filter: Kaiser-windowed sinc, beta 8.6, 32 zero crossings a side, as the resampler's, in float64:
 *   fc = 0.475 * min(1, 1 / sigma) cycles per input sample,  W = ceil(32 / (2 fc)) (34 for sigma <= 1, up to 43),  T = 2 W taps,
 *   h(u) = 2 fc sinc(2 fc u) * I0(8.6 sqrt(1 - (u / W)^2)) / I0(8.6)  for |u| <= W, else 0.
 * Table: hq[p][t] = round(2^30 h(p / 512 + W - 1 - t)) as int32, p = 0 .. 512 (513 rows: p + 1 always exists), t = 0 .. T - 1.
 * Output n (n_in < 2^31):  P = n * step (int64),  pos = P >> 24,  frac = P & (2^24 - 1),  p = frac >> 15,  w = frac & 32767,
 *   c_t  = (hq[p][t] * (32768 - w) + hq[p + 1][t] * w + 16384) >> 15
 *   acc  = sum_t c_t * x[pos - W + 1 + t]      (int64; samples outside [0, n_in) are zero)
 *   y[n] = clamp((acc + 2^29) >> 30, -32768, 32767),  arithmetic shifts;   n_out = ceil(n_in * 2^24 / step).
 * Status: a step outside the range or n_in >= 2^31 NAFP_ERR_UNSUPPORTED, null pointers / negative sizes / an inconsistent
 * piece NAFP_ERR_INVALID_ARG, all before any GPU call.
 * ---------------------------------------------------------------------- */
typedef struct nafp_varispeed nafp_varispeed;

#define NAFP_VARISPEED_STEP_MIN 13421773u
#define NAFP_VARISPEED_STEP_MAX 20971520u

/* A run of consecutive output samples of one file, with the meanings of nafp_resample_piece: the model-rate samples present
 * for it are only what its outputs need (nafp_varispeed_input_range).  56 bytes. */
typedef struct nafp_varispeed_piece {
    int64_t src_off;     /* int16 index in the source arena of the first sample present */
    int64_t frame0;      /* which model-rate sample of the file that is */
    int64_t n_frames;    /* samples present */
    int64_t n_in;        /* model-rate samples of the whole file */
    int64_t out0;        /* index in the file's stretched stream of the first output */
    int64_t out_off;     /* int16 index in the output arena of that output */
    int32_t n_out;       /* outputs */
    int32_t reserved;
} nafp_varispeed_piece;

/* Host only. */
int nafp_varispeed_geometry(uint32_t step, int* W, int* T);
/* Host only: the table (513, T) int32, [phase p][tap t], as defined above. */
int nafp_varispeed_table_host(uint32_t step, int32_t* table_host);
int64_t nafp_varispeed_n_out(int64_t n_in, uint32_t step);                 /* -1: unsupported step / n_in outside [0, 2^31) */
/* Host only: the samples [*first, *last) of a file of n_in samples that the outputs [n0, n1) read (first == last: none). */
int nafp_varispeed_input_range(int64_t n0, int64_t n1, int64_t n_in, uint32_t step, int64_t* first, int64_t* last);
/* Host only: the checks the kernel makes per piece, on a host copy of the list, before it is uploaded: indices inside
 * src_samples / out_samples, the outputs inside the file's n_out, every sample they read present. */
int nafp_varispeed_check_pieces_host(uint32_t step, const nafp_varispeed_piece* pieces_host, int64_t n_pieces,
                                     int64_t src_samples, int64_t out_samples);
/* The plan owns the device table. */
int nafp_varispeed_create(nafp_varispeed** plan, uint32_t step);
int nafp_varispeed_destroy(nafp_varispeed* plan);
/* src (src_samples int16) -> out (out_samples int16) for the n_pieces pieces of pieces_dev, all device pointers.  Every index
 * derived from a piece is checked on the device against src_samples / out_samples: an inconsistent piece is skipped, its
 * outputs zeroed (nothing is written for one whose output range leaves the arena).  Int16 outside the pieces' output ranges
 * is not touched. */
int nafp_varispeed_i16(nafp_varispeed* plan, const int16_t* src, int64_t src_samples, const nafp_varispeed_piece* pieces_dev,
                       int64_t n_pieces, int16_t* out, int64_t out_samples, void* stream);

/* ------------------------------------------------------------------------
 * Block codecs in RIFF/WAVE: G.711 A-law and mu-law, IMA ADPCM and MS ADPCM at 4 bits, and Apple's IMA4 packets of AIFF-C
 * (csrc/codec.hip, the arithmetic in csrc/codec_decode.h; numpy restatements tests/_codec_ref.py and tests/_aiff_ref.py;
 * DESIGN.md sections 4.10.2 and 4.10.5).  A PRE-PASS of nafp_ingest_*, which is
 * unchanged: whole blocks are decoded to interleaved 16-bit PCM in a device arena, which nafp_ingest_i16 then reads as
 * NAFP_INGEST_S16.  A "block" is block_align bytes and yields spb (samples per block) frames of C = channels interleaved int16.
 * ALL ARITHMETIC IS int32 AND EXACT: a decoded sample is a pure function of (its block's bytes, its place in the block),
 * whatever shares its piece, workgroup or launch.  For all codecs block_align <= 4096.
 *
 * G.711 -- C = 1..8, block_align = C, spb = 1; per byte:
 *   mu-law: u = ~byte & 0xff;  t = (((u & 15) << 3) + 0x84) << ((u & 0x70) >> 4);  x = (u & 0x80) ? 0x84 - t : t - 0x84
 *   A-law:  a = byte ^ 0x55;  t = (a & 15) << 4;  seg = (a & 0x70) >> 4;
 *           seg 0: t += 8;  seg 1: t += 0x108;  otherwise t = (t + 0x108) << (seg - 1);  x = (a & 0x80) ? t : -t
 *   (|x| <= 32124 for mu-law, <= 32256 for A-law.)
 * IMA ADPCM, 4 bits -- C = 1 or 2; block_align - 4 C = 4 C G with G >= 1, spb = 8 G + 1.
 *   Layout: per channel a 4-byte header (int16 predictor, uint8 step index, one ignored byte); the predictor is frame 0.  Then
 *   G groups; group g holds, for each channel in order, 4 bytes = the 8 nibbles of frames 1 + 8 g .. 8 + 8 g, bytes ascending,
 *   LOW nibble first.  The header's step index is clamped to 0..88.  Per nibble n:
 *     s = STEP[idx];  d = s >> 3;  d += s >> 2 if n & 1;  d += s >> 1 if n & 2;  d += s if n & 4;
 *     pred = clamp16(n & 8 ? pred - d : pred + d);  idx = clamp(idx + IDX[n], 0, 88)
 *   STEP: the standard 89 entries (7, 8, 9, ... 29794, 32767); IDX = {-1, -1, -1, -1, 2, 4, 6, 8} for n & 7.
 * MS ADPCM, 4 bits -- C = 1 or 2; block_align > 7 C, spb = 2 + 2 (block_align - 7 C) / C.
 *   Layout: C bytes bPredictor, C x int16 iDelta, C x int16 iSamp1, C x int16 iSamp2; frame 0 is iSamp2, frame 1 is iSamp1.
 *   Body nibbles HIGH nibble first, round-robin over the channels: nibble k is frame 2 + k / C, channel k % C.
 *   Coefficients (c1, c2): (256,0) (512,-256) (0,0) (192,64) (240,0) (460,-208) (392,-232); a bPredictor above 6 uses pair 6.
 *   Per nibble n, s = n - 16 if n >= 8 else n:
 *     pred = (samp1 c1 + samp2 c2) / 256, C division TRUNCATING TOWARD ZERO (the Microsoft text; a shift differs by one LSB on
 *     negative sums);  x = clamp16(pred + s delta);  samp2 = samp1;  samp1 = x;
 *     delta = clamp((ADAPT[n] delta) >> 8, 16, 2796202), arithmetic shift (2796202 = INT_MAX / 768: every product fits int32);
 *   ADAPT = {230,230,230,230,307,409,512,614,768,614,512,409,307,230,230,230}.  The header's iDelta, sign-extended, is used as
 *   it stands for the first nibble.
 * Apple IMA4 (the `ima4` compression of AIFF-C; NAFP_CODEC_QT_IMA4) -- C = 1 or 2; block_align = 34 C, spb = 64.
 *   Layout: one 34-byte packet per channel, channel c's at bytes [34 c, 34 c + 34).  A packet is a BIG-endian uint16 h --
 *   predictor = (int16)(h & 0xFF80), step index = min(h & 0x7F, 88) -- and 32 bytes of two nibbles each, LOW nibble first, every
 *   nibble through the IMA recurrence above.  The 64 predictor values AFTER each nibble are frames 0 .. 63 of the channel; the
 *   header's predictor itself is not a sample.  The decode is STATELESS PER PACKET, as the contract of this section requires: no
 *   state is carried from the packet before (decoders that carry it when it agrees with the header to within the 7 dropped
 *   bits, or that form the step product by a multiplication, differ in the low bits).
 * Status: a codec, channel count or block_align outside the lists NAFP_ERR_UNSUPPORTED, null pointers / negative sizes / an
 * inconsistent piece NAFP_ERR_INVALID_ARG, all before any GPU call.
 * ---------------------------------------------------------------------- */
#define NAFP_CODEC_ALAW 1
#define NAFP_CODEC_ULAW 2
#define NAFP_CODEC_IMA4 3
#define NAFP_CODEC_MS4 4
#define NAFP_CODEC_QT_IMA4 6 /* 5 is not a codec */

/* A run of whole blocks of one file.  40 bytes. */
typedef struct nafp_codec_piece {
    int64_t raw_off;      /* byte index in the raw arena of the first block (any alignment) */
    int64_t n_blocks;     /* whole blocks */
    int64_t out_off;      /* int16 index in the output arena of frame 0, channel 0 of the first block (any parity) */
    int32_t codec;        /* NAFP_CODEC_* */
    int32_t channels;
    int32_t block_align;
    int32_t spb;          /* nafp_codec_samples_per_block(codec, channels, block_align) */
} nafp_codec_piece;

/* Host only: frames per block, or -1 for anything outside the lists above. */
int nafp_codec_samples_per_block(int codec, int channels, int block_align);
/* Host only: how many blocks one workgroup of the kernel takes at a time (G.711: the frames one workgroup step covers), -1 as
 * above.  The bytes written do not depend on it; tests cut pieces around it. */
int nafp_codec_blocks_per_group(int codec, int channels, int block_align);
/* Host only: n_blocks blocks at `bytes` -> n_blocks * spb * channels int16 -- the function the kernel decodes with, compiled
 * for the host. */
int nafp_codec_decode_host(int codec, int channels, int block_align, const void* bytes, int64_t n_blocks, int16_t* out);
/* Host only: the checks the kernel makes per piece. */
int nafp_codec_check_pieces_host(const nafp_codec_piece* pieces_host, int64_t n_pieces, int64_t raw_size, int64_t out_samples);
/* raw_bytes (raw_size bytes) -> out (out_samples int16) for the n_pieces pieces of pieces_dev, all device pointers.  Every
 * index derived from a piece is checked on the device against raw_size / out_samples.  The output range of a piece is the one
 * it states: n_blocks * spb * channels int16 at out_off.  A piece whose range is not a range of the arena (or whose n_blocks,
 * spb or channels cannot state one: negative, spb > 8185, channels outside 1..8) writes nothing; any other inconsistent piece
 * (codec, channels, block_align or spb outside the lists or not matching, raw range outside the arena) is skipped and its range
 * zeroed.  No byte outside the two arenas is read or written whatever a piece says; int16 outside the pieces' output ranges
 * is not touched. */
int nafp_codec_decode_i16(const uint8_t* raw_bytes, int64_t raw_size, const nafp_codec_piece* pieces_dev, int64_t n_pieces,
                          int16_t* out, int64_t out_samples, void* stream);

/* ------------------------------------------------------------------------
 * FLAC (csrc/flac.hip, the arithmetic in csrc/flac_decode.h; numpy / Python restatement tests/_flac_ref.py; DESIGN.md section
 * 4.10.3).  A PRE-PASS of nafp_ingest_*, which is unchanged: whole frames are decoded to interleaved little-endian PCM of the
 * file's own channel count and rate in a device BYTE arena.  A sample v of bps <= 16 bits becomes an s16 container holding
 * v << (16 - bps), one of 17 .. 24 bits a 3-byte s24 container holding v << (24 - bps) -- the bytes of the MSB-justified PCM WAV of
 * the same samples -- which nafp_ingest_i16 then reads as NAFP_INGEST_S16 / NAFP_INGEST_S24.
 * Taken: native FLAC streams (an ID3v2 tag before `fLaC` is skipped), 1 .. 8 channels, 8 / 12 / 16 / 20 / 24 bits, block sizes up
 * to 16384 in fixed- or variable-blocksize streams, constant / verbatim / fixed (order 0 .. 4) / LPC (order 1 .. 32, precision
 * 1 .. 15, shift 0 .. 15) subframes, both Rice methods with escape partitions, wasted bits, all four channel assignments.
 * ALL ARITHMETIC IS INTEGER AND EXACT: a prediction is sum_j coef[j] * s[i - 1 - j] in int64, shifted right arithmetically by
 * `shift`, plus the residual, truncated to int32; fixed predictors are the same form with coefficients (1) (2,-1) (3,-3,1)
 * (4,-6,4,-1); a side channel carries bps + 1 bits.  A decoded frame is a pure function of (its bytes, its record), whatever
 * shares its launch.
 * CORRUPT INPUT: every bit read is bounded by the frame's stated length, every unary run, Rice parameter, raw-bit count, LPC
 * order (<= block size), partition order (block size divisible by 2^order, first partition >= predictor order), reserved code and
 * write index is checked.  A frame that fails a check or its CRC-16 (polynomial 0x8005, initial 0) has its WHOLE output range
 * zeroed and a non-zero status; a frame whose header disagrees with its record (the file's STREAMINFO) in block size, channels,
 * depth or rate fails too; a record that states no range of the scratch arena writes nothing.  Other frames are unaffected.
 * Status of the functions: null pointers / negative sizes / an inconsistent record NAFP_ERR_INVALID_ARG, before any GPU call.
 * ---------------------------------------------------------------------- */
/* per-frame status (int32): 0 = decoded */
#define NAFP_FLAC_BAD_RECORD 1        /* raw range outside the arena, depth / rate outside the contract: range zeroed */
#define NAFP_FLAC_BAD_HEADER 2        /* no sync, a reserved bit or code, a bad coded number or CRC-8 */
#define NAFP_FLAC_HEADER_MISMATCH 3   /* block size, channels, depth or rate differ from the record */
#define NAFP_FLAC_TRUNCATED 4         /* the frame's bytes end before the frame does */
#define NAFP_FLAC_BAD_SUBFRAME 5      /* reserved type, wasted bits >= width, order > block size, precision 16, negative shift */
#define NAFP_FLAC_BAD_RESIDUAL 6      /* reserved method, partition order, over-long unary run */
#define NAFP_FLAC_BAD_CRC16 7
#define NAFP_FLAC_NO_RANGE 8          /* the record states no range of the scratch arena: nothing written */
/* nafp_flac_info.refusal: 0 = taken */
#define NAFP_FLAC_REFUSE_OGG 1
#define NAFP_FLAC_REFUSE_MARKER 2      /* no `fLaC` */
#define NAFP_FLAC_REFUSE_STREAMINFO 3  /* the first metadata block is not a 34-byte STREAMINFO */
#define NAFP_FLAC_REFUSE_DEPTH 4       /* not 8 / 12 / 16 / 20 / 24 bits */
#define NAFP_FLAC_REFUSE_BLOCK 5       /* maximum block size above 16384 */

/* 72 bytes. */
typedef struct nafp_flac_info {
    int64_t total_samples;    /* STREAMINFO's count of frames of audio, 0 = unknown */
    int64_t audio_off;        /* byte offset behind the last metadata block */
    int64_t n_indexed;        /* nafp_flac_index_host: frames in the index (may exceed the caller's cap) */
    int64_t indexed_samples;  /* nafp_flac_index_host: sum of their block sizes */
    int32_t rate, channels, bps, min_block, max_block, refusal;
    uint8_t md5[16];
} nafp_flac_info;

/* One frame of the index.  32 bytes. */
typedef struct nafp_flac_index_entry {
    int64_t offset;        /* byte offset of the sync code in the file */
    int64_t first_sample;  /* as coded: frame number x STREAMINFO block size, or the sample number */
    int64_t n_bytes;       /* up to the next indexed frame, or the end of the file */
    int32_t block_size;
    int32_t reserved;
} nafp_flac_index_entry;

/* One frame of a launch, uploaded by the host.  40 bytes. */
typedef struct nafp_flac_frame {
    int64_t raw_off;       /* byte index in the raw arena of the frame's sync code (any alignment) */
    int64_t scratch_off;   /* byte index in the scratch arena of sample 0, channel 0 (any alignment) */
    int32_t n_bytes;       /* bytes the frame may read */
    int32_t block_size;    /* 1 .. 16384 */
    int32_t channels;      /* 1 .. 8, STREAMINFO's */
    int32_t bps;           /* 8 / 12 / 16 / 20 / 24, STREAMINFO's */
    int32_t rate;          /* STREAMINFO's */
    int32_t reserved;
} nafp_flac_frame;

/* Host only: STREAMINFO of the stream at bytes[0, n_bytes).  NAFP_OK with info->refusal set for a stream that is not taken. */
int nafp_flac_streaminfo_host(const void* bytes, int64_t n_bytes, nafp_flac_info* info);
/* Host only: STREAMINFO and the frame index of a whole stream, one pass.  Candidates are found by the sync pattern and kept when
 * their header parses (reserved bits and codes, coded number, CRC-8) and CONTINUES THE CHAIN: fixed-blocksize stream -- frame number
 * = predecessor's + 1, first sample = number x STREAMINFO block size, only the last frame shorter; variable-blocksize stream -- coded
 * sample number = predecessor's first sample + block size.  The chain starts at the first valid header behind the metadata, whatever
 * its number.  A candidate that breaks continuity is dropped.  A FALSE candidate that keeps continuity by chance is not recognised
 * here: it is caught by the frame's CRC-16 on the device and counts as a failed frame.  A last frame the file cuts short is left
 * out.  At most `cap` entries are written to frames_out (may be NULL with cap 0); info->n_indexed counts all. */
int nafp_flac_index_host(const void* bytes, int64_t n_bytes, nafp_flac_info* info, nafp_flac_index_entry* frames_out, int64_t cap);
/* Host only: what nafp_flac_decode writes, from the function the kernels decode with, compiled for the host: the same scratch
 * bytes, the same status per frame (status_out may be NULL). */
int nafp_flac_decode_host(const void* raw, int64_t raw_size, const nafp_flac_frame* frames_host, int64_t n_frames, void* scratch,
                          int64_t scratch_size, int32_t* status_out);
/* Host only: the checks the kernels make per record; NAFP_ERR_INVALID_ARG for one that would not decode (status 1 or 8). */
int nafp_flac_check_frames_host(const nafp_flac_frame* frames_host, int64_t n_frames, int64_t raw_size, int64_t scratch_size);
/* raw (raw_size bytes) -> scratch (scratch_size bytes) for the n_frames records of frames_dev, all device pointers; status_dev:
 * int32 per frame, may be NULL.  Every index derived from a record or from the stream is checked on the device.  No byte outside
 * the two arenas is read or written whatever a record or a frame says; bytes outside the records' output ranges are not touched.
 * An int32 workspace of scratch_size / 2 + 1 elements is taken from the stream-ordered allocator for the duration of the call. */
int nafp_flac_decode(const uint8_t* raw, int64_t raw_size, const nafp_flac_frame* frames_dev, int64_t n_frames, uint8_t* scratch,
                     int64_t scratch_size, int32_t* status_dev, void* stream);

/* ------------------------------------------------------------------------
 * Encoder: FingerPrinter (model/fp/nnfp.py:159-231)
 * ---------------------------------------------------------------------- */

/* get_fingerprinter(cfg) (nnfp.py:234-258): 8 ConvLayer blocks with the channel
 * and stride tables of nnfp.py:193-197 on an (in_f, in_t, 1) input, DivEncLayer
 * with q = emb_sz slices, unit_dim [32,1].  (256,32,1) is the deployed shape. */
int nafp_encoder_create(nafp_encoder** enc, int in_f, int in_t, int emb_sz);
int nafp_encoder_destroy(nafp_encoder* enc);

/* The same with the normalisation of the ConvLayers chosen (config MODEL.BN -> ConvLayer(norm=...), nnfp.py:63-71, 250):
 *   NAFP_NORM_LAYER2D  'layer_norm2d' (the default and what nafp_encoder_create builds): LayerNormalization(axis=(1,2,3)),
 *                      folded into the GEMM epilogues;
 *   NAFP_NORM_LAYER1D  'layer_norm1d': LayerNormalization(axis=-1), statistics over the channels of one position; one extra
 *                      elementwise pass per layer and direction;
 *   NAFP_NORM_BATCH    'batch_norm' (or any other string): BatchNormalization(axis=-1) AS THE REFERENCE CALLS IT -- `m_fp(feat)`
 *                      without a `training` argument in train_step, val_step and generate (trainer.py:44, 60; generate.py:88),
 *                      i.e. always in inference mode: the per-channel affine map of the moving statistics (never updated:
 *                      keras initialises them to 0 / 1; a checkpoint may hold others), trainable gamma / beta.  Folded exactly
 *                      into the same epilogues.
 * With the alternates the tensors 4j+2 / 4j+3 are gamma / beta of shape (C); NAFP_NORM_BATCH appends, behind tensor 67, the
 * NON-trainable moving statistics: 68+2j moving_mean (C), 69+2j moving_variance (C), j = 0..15.  The gradient list of
 * nafp_encoder_backward covers the trainable tensors 0..67 only (nafp_encoder_n_trainable).  NAFP_OPT_FUSE_CONV0,
 * and NAFP_OPT_FUSED_LN_BWD are ignored by the alternates. */
#define NAFP_NORM_LAYER2D 0
#define NAFP_NORM_LAYER1D 1
#define NAFP_NORM_BATCH 2
int nafp_encoder_create_ex(nafp_encoder** enc, int in_f, int in_t, int emb_sz, int norm);
int nafp_encoder_norm(const nafp_encoder* enc);            /* NAFP_NORM_* of the handle */
int nafp_encoder_n_trainable(const nafp_encoder* enc);     /* 68: the tensors nafp_encoder_backward writes gradients for */

/* Parameter tensors, in this fixed order (n = nafp_encoder_n_tensors):
 *   for j in 0..15 (even = conv 1x3, odd = conv 3x1; nnfp.py:48-79):
 *     4j+0 kernel (kh,kw,Cin,Cout)   4j+1 bias (Cout)
 *     4j+2 LN gamma (F,T,C)          4j+3 LN beta (F,T,C)      [(C) each with NAFP_NORM_LAYER1D / NAFP_NORM_BATCH]
 *   64 div.w1 (Q,S,32)   65 div.b1 (Q,32)   66 div.w2 (Q,32,1)   67 div.b2 (Q,1)
 * i.e. the keras variable shapes, C-order float32. */
int nafp_encoder_n_tensors(const nafp_encoder* enc);
int64_t nafp_encoder_tensor_numel(const nafp_encoder* enc, int index);
/* writes up to 4 dims, returns rank (or -1) */
int nafp_encoder_tensor_shape(const nafp_encoder* enc, int index, int64_t dims_out[4]);
int64_t nafp_encoder_flat_dim(const nafp_encoder* enc);    /* F'*T'*C of front_conv (1024) */

/* Copy/pack weights from caller device tensors (array of n device pointers, the
 * array itself in host memory).  May be called again after every optimizer step.
 * Ordering: the call may be given a stream of its own.  Every later pass of this handle on a
 * DIFFERENT stream (forward*, div_enc, forward_train, backward) waits on the device for what it
 * reads of this call's output -- the training forward starts its first conv as soon as the plain
 * copies are done, its second behind layer 1's share (formed first) and only its third behind the
 * whole re-pack --, so the caller does not order them.  What the caller still orders: this call behind the passes enqueued EARLIER on
 * other streams (they read the blob it overwrites), and behind whatever produced `tensors`. */
int nafp_encoder_set_weights(nafp_encoder* enc, const float* const* tensors_host_array,
                             void* stream);

int64_t nafp_encoder_workspace_bytes(const nafp_encoder* enc, int64_t n_seg);

/* m_fp(feat) (nnfp.py:223-231).  feat (n_seg, in_f, in_t) float32.
 *   out_flat  optional (n_seg, flat_dim): front_conv output (nnfp.py:225), may be NULL
 *   out_emb   optional (n_seg, emb_sz): l2_normalize(div_enc(.)) if l2norm != 0,
 *             else div_enc(.) (use_L2layer, nnfp.py:228-231), may be NULL
 * LAUNCH-SIZE INDEPENDENCE AND WHAT IT COSTS SMALL LAUNCHES.  Every launch is planned -- tile shape, split-K factor, which finish runs --
 * as if it held 640 segments (environment NAFP_PLAN_B; the generate / bench launch size), whatever n_seg is, and only the grids follow
 * n_seg: the bytes of a segment's fingerprint do not depend on what shares its launch, at any n_seg (a launch with more split-K tiles
 * than arrival counters, n_seg > ~4096, runs those layers as several sample ranges).  The price is paid by very small launches
 * (n_seg = 1 .. 8, query-time latency): they no longer get the deeper split-K a plan for their own size would choose and leave most
 * of the chip idle in the mid layers.  NAFP_PLAN_B=0 plans per launch again (fastest single-segment latency, fingerprints then differ
 * in their last bits between launch sizes); a deployment that serves single queries next to a database built at 640 per launch
 * should keep the default.   */
int nafp_encoder_forward(nafp_encoder* enc, const float* feat, int64_t n_seg,
                         void* workspace, int64_t workspace_bytes,
                         float* out_flat, float* out_emb, int l2norm, void* stream);

/* m_fp(m_pre(X)) with the tail of the log-mel layer (x - reduce_max(x), clamp at -80, optional segment
 * normalisation: melspectrogram.py:108-111) applied by the first conv as it loads: raw_feat / group_stat are what
 * nafp_melspec_forward_* leave with NAFP_MELSPEC_DEFER, group_size the same grouping.  Bit-identical to
 * nafp_encoder_forward on the finished features. */
int nafp_encoder_forward_raw(nafp_encoder* enc, const float* raw_feat, const float* group_stat, int group_size,
                             int segment_norm, int64_t n_seg, void* workspace, int64_t workspace_bytes,
                             float* out_flat, float* out_emb, int l2norm, void* stream);

/* DIAGNOSTIC, for tests that compare two forms of the first conv bit for bit (the forward reuses z0's buffer two layers later); not
 * part of the inference interface.  The first conv (b0.conv1x3) of nafp_encoder_forward / _forward_raw alone, in the form the handle's
 * options select (group_stat may be NULL: finished features): z0 (n_seg, in_f, t_out, c0) = gamma0 . ELU(conv + bias),
 * nafp_encoder_conv0_numel floats per segment, and the layer's LayerNorm statistics as the next conv reads them, two 64-bit
 * fixed-point sums per segment (stats_out: 2 * n_seg, zeroed by the call on `stream`).  As in the forward, a handle created with
 * another normalisation than layer_norm2d drops finite partial sums beyond the fixed-point range instead of poisoning the sample. */
int64_t nafp_encoder_conv0_numel(const nafp_encoder* enc);
int nafp_encoder_conv0(nafp_encoder* enc, const float* feat, const float* group_stat, int group_size, int segment_norm,
                       int64_t n_seg, float* z0_out, long long* stats_out, void* stream);

/* Per-kernel timing of nafp_encoder_forward with HIP events recorded on the
 * caller's stream (bench.py's roofline leg).  enable(max_forwards > 0) allocates a
 * ring of event sets, one per forward call; enable(0) turns it off.  read() waits
 * for slot `slot` (0 = the first forward after enable) and writes 17 durations in
 * milliseconds: [0] conv0, [1..15] the implicit-GEMM convs, [16] the tail. */
#define NAFP_ENCODER_PROFILE_KERNELS 17
int nafp_encoder_profile_enable(nafp_encoder* enc, int max_forwards);
int nafp_encoder_profile_count(const nafp_encoder* enc);   /* forwards recorded so far */
/* Stamp granularity of the forwards that follow.
 *   0 (default): conv0, every GEMM conv, tail.  The GEMM convs are stamped on their own dispatch packets -- start of the
 *      first kernel, end of the last (a split-K finish kernel included): hipExtLaunchKernel, nothing is put into the queue --,
 *      conv0 and the tail between recorded events.  (Stamping every launch is still not free: the per-conv figures sum to
 *      about 10 % more than the span mode 2 measures for the same launches.)
 *   1: conv0 | the 15 GEMM convs as one span | tail, between recorded events (an event recorded between two kernels costs
 *      the GPU about 20 us of un-overlapped dispatch set-up).
 *   2: only the span of the 15 GEMM convs, from the dispatch packets of conv1 and of the last GEMM-conv kernel: no queue
 *      entry at all -- what a timed region uses.  profile_read returns the span in slot 1, zeros elsewhere. */
int nafp_encoder_profile_coarse(nafp_encoder* enc, int coarse);
int nafp_encoder_profile_read(nafp_encoder* enc, int slot, float* ms_out_host);
/* Diagnostic, process-wide: while `dev_buf` is non-null every forward GEMM-conv launch (full mode) whose conv has
 * (cin, cout, output positions per segment) as given stamps the shader clock at the phase boundaries of each tile:
 * 8 u64 per wave, 8 wave slots per workgroup, workgroups in launch order -- [hw_id | xcc_id << 32, entry, geometry done,
 * first operands landed, K-loop done, after the barrier behind it, epilogue stores issued, end].  `capacity_u64` bounds
 * the buffer (launches needing more are not recorded).  nafp_conv_timeline_grid returns {grid x, y, z, tile rows, tile
 * columns} of the last recorded launch.  tools/conv_timeline.py turns the stamps into per-phase times and per-CU overlap. */
int nafp_conv_timeline(void* dev_buf, int64_t capacity_u64, int cin, int cout, int positions);
int nafp_conv_timeline_grid(int* out5_host);
/* Diagnostic, host only (works in a process without a GPU): what the launcher of the GEMM convs will do with conv `layer`
 * (1 ... 15) of an encoder on (in_f, in_t) features for a launch of `n_seg` segments -- tile, split-K factor and finish, kernel, grid
 * and its mapping -- under the NAFP_* knobs of this process.  plan_b: the planning batch of the inference forward (0: the launch's own
 * size, as training); flags: the facts of the call, NAFP_PLAN_* or-ed, the arithmetic (0 f32, 1 bf16x3, 2 bf16x6) in bits 8-9;
 * slab_floats: the split-K workspace the caller has (0: none).  record_host receives NAFP_CONV_PLAN_FIELDS values:
 *   [0] kernel (row of the launcher's table; its symbol goes to kernel_name_host, if given) [1] tile rows [2] tile columns
 *   [3] LDS ring depth [4] dynamic LDS bytes [5-7] grid x, y, z [8] positions and [9] samples per tile [10] sample groups
 *   [11] position blocks [12] K-steps the split policy counts [13] split-K factor [14] finish: 0 none, 1 finish kernel, 2 in-kernel
 *   (FULL), 3 in-kernel (PLAIN) [15] float4 per workgroup of the FULL finish kernel [16] grid of the finish kernel [17] kernel mode:
 *   0 FULL, 1 PLAIN, 2 split-K part [18] epilogue: 0 inference, 1 training, 2 generic statistics, 3 plain / part, 4 / 5 in-kernel
 *   finish FULL / PLAIN [19] arithmetic [20-22] class order of the positions: kind, size and parity of class 0 [23] option bits
 *   (1 | 2 wave priority, 4 3-D grid, 8 XCD-aware 1-D grid, 16 ... row-fastest) [24] items per XCD group [25] items in full blocks
 *   of 8 groups [26] log2 of the column tiles [27] samples per launch when the launch runs as several over sample ranges (grid x
 *   then follows each range; 0: one launch) [28] ablation bits [29] the workspace (floats) the sizing wants for this layer at n_seg
 *   (with NAFP_PLAN_SIZE_DGRAD: for its transposed conv as well).
 * Returns NAFP_ERR_UNSUPPORTED for a shape the launcher refuses ([29] is still set).  tests/test_conv_plan_host.py holds the plans. */
#define NAFP_CONV_PLAN_FIELDS 30
#define NAFP_PLAN_PLAIN 1
#define NAFP_PLAN_DGRAD 2
#define NAFP_PLAN_V_OUT 4
#define NAFP_PLAN_TICKETS 8
#define NAFP_PLAN_SPLIT_WEIGHTS 16
#define NAFP_PLAN_FUSE0 32
#define NAFP_PLAN_SIZE_DGRAD 64
int nafp_conv_plan(int in_f, int in_t, int layer, int64_t n_seg, int64_t plan_b, int flags, int64_t slab_floats,
                   int64_t* record_host, char* kernel_name_host, int name_capacity);

/* Training (model/trainer.py:41-47: emb = m_fp(feat) under tf.GradientTape, then
 * tape.gradient(loss, m_fp.trainable_variables)).  forward_train is nafp_encoder_forward that
 * keeps every activation in `workspace`; backward consumes the SAME workspace (untouched in
 * between) and d_emb = dL/d(out_emb), and writes the 68 parameter gradients in the keras shapes
 * and order of the parameter tensors (grads_host_array: host array of device pointers; the
 * gradients are overwritten, not accumulated).  `feat` is the same (n_seg, in_f, in_t) input. */
int64_t nafp_encoder_train_workspace_bytes(const nafp_encoder* enc, int64_t n_seg);
int nafp_encoder_forward_train(nafp_encoder* enc, const float* feat, int64_t n_seg, void* workspace,
                               int64_t workspace_bytes, float* out_emb, int l2norm, void* stream);
int nafp_encoder_backward(nafp_encoder* enc, const float* feat, const float* d_emb, int64_t n_seg,
                          void* workspace, int64_t workspace_bytes, float* const* grads_host_array,
                          int l2norm, void* stream);

/* Overlap of the data-parallel gradient reduction with the backward pass.  The backward pass finishes the
 * parameter gradients last layer first; it records one event per GROUP of tensors, in completion order:
 *   group 0 = tensors 48..67 (convs 12-15 and the divide-and-encode tensors: 65 % of all parameters),
 *   group 1 = 32..47, group 2 = 16..31, group 3 = 0..15.
 * nafp_encoder_grad_group_wait makes `stream` (the communication stream) wait, on the device, until group
 * `group` of the most recent nafp_encoder_backward call is complete; the host does not block. */
#define NAFP_GRAD_GROUPS 4
int nafp_encoder_grad_group_range(const nafp_encoder* enc, int group, int* first_tensor, int* last_tensor);
int nafp_encoder_grad_group_wait(nafp_encoder* enc, int group, void* stream);

/* Execution options of an encoder handle (results are identical either way, except NAFP_OPT_BF16X3).
 *   NAFP_OPT_FUSE_CONV0  0 (default): b0.conv1x3 writes its activation, b0.conv3x1 reads it back.
 *                        1: only conv0's LayerNorm statistics are computed up front and conv1
 *                           re-generates its input tiles in-kernel from the log-mel features.
 *   NAFP_OPT_FUSED_LN_BWD  training: the LayerNorm + ELU backward of a layer runs in the epilogue of the transposed conv
 *                        that produces its gradient (one read of the stored pre-activation, one write, instead of a
 *                        separate pass that re-reads and re-writes the gradient).  0 (default): never -- measured slower
 *                        than the separate pass; 1: for the layers of >= 32768 elements per sample at
 *                        batches >= 64; 2: wherever the geometry permits.
 *   NAFP_OPT_BWD_OVERLAP  training: weight gradients of nafp_encoder_backward on a second stream owned by the handle; `stream` is
 *                        made to wait for them before the last event of the call, so callers see the same ordering as with 0.
 *                        2 (default): those of the SMALL layers (fewer than 16 output positions), next to the LayerNorm backward
 *                        and transposed conv of the layer below; 1: every layer's (measured slower); 0: everything on
 *                        `stream`.
 *   (5, NAFP_OPT_SMALLNET: retired in round 6 -- the small layers as one persistent launch measured slower than the per-layer launches
 *                        at every setting, docs/DESIGN_HISTORY.md; the number stays reserved, setting it is accepted and ignored.) */
#define NAFP_OPT_FUSE_CONV0 1
#define NAFP_OPT_FUSED_LN_BWD 2
#define NAFP_OPT_BWD_OVERLAP 4
#define NAFP_OPT_SMALLNET 5           /* retired, ignored */
/* (6 is a test hook of tests/test_gpu_train_dp.py -- it delays the handle's weight-gradient stream -- and is refused unless the process
 * runs with NAFP_TEST_HOOKS=1 in its environment; not part of the interface.) */
/* EXPERIMENTAL, changes the arithmetic (the only option that does): the unsplit GEMM convs of nafp_encoder_forward form their
 * products on the bf16 matrix pipe from f32 operands split into hi + lo bf16 halves (hi*hi + hi*lo + lo*hi, f32
 * accumulation).  Fingerprints move at the 1e-6 level against the f32 path.  Off by default; bench.py reports it as a
 * separate object with its measured error, never as the headline value.
 * value 2: the EXACT 3-way split x = h + m + l (three bf16 terms hold a float32's 24 significant bits) with the six products of
 * relative weight >= 2^-16 (hh, hm, mh, hl, mm, lh; the dropped ml + lm + ll < 2^-25 of |a||b|): float32-equivalent arithmetic on
 * the bf16 matrix pipe -- its error against the float64 oracle equals the f32 path's own (tests/test_gpu_parity_forward.py).
 * Value 2 also covers the TRAIN step: nafp_encoder_forward_train, the transposed convs and the weight gradients of
 * nafp_encoder_backward run on the same arithmetic (the flipped kernels are split alongside in nafp_encoder_set_weights; LayerNorm
 * backward, loss and optimizer stay f32): gradients within the f32 path's tolerances
 * (tests/test_gpu_backward.py, tests/test_gpu_configs.py), the step 84 -> 69 ms at BSZ 5120, 11.9 -> 9.7 ms at 640 (bench.py
 * `train_x6_experimental`).
 * CAUTION for kernels of OTHER libraries (values 1 and 2): on gfx950 a packed-f32 vector instruction that carries an op_sel modifier
 * (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 ... op_sel:[..]; compilers emit them for complex arithmetic -- rocFFT's kernels hold
 * them) returns wrong values in a wave that shares a compute unit with waves issuing the 128-bit-operand matrix instructions
 * (v_mfma_f32_32x32x16_bf16, what this option runs on) next to vector work.  Found in round 6; tools/probes/pk_opsel_hazard_probe.hip
 * reproduces it without this library, profiles/r06_experiments.md section 5 has the matrix of instructions.  EVERY kernel of this
 * library is compiled without packed-f32 instructions (build.py NO_PACKED_F32; tests/test_abi.py disassembles the library and holds
 * it), so the library's own kernels -- front end, other forwards, training -- overlap such a forward freely and stay run-to-run
 * bit-identical (tests/test_gpu_generate.py, tools/x6_determinism_check*.py).  A foreign kernel holding such instructions must not
 * run on the device while a forward with this option is in flight.  The fp32 path (f32 matrix instructions) does not disturb anything. */
#define NAFP_OPT_BF16X3 3
/* NAFP_OPT_NONMATRIX: a mask of NAFP_NONMATRIX_* bits, one per leaner form of a part of the forward pass OUTSIDE the GEMM K-loops.  Every
 * bit leaves every byte of every result and of the per-layer statistics as it is (tests/test_gpu_nonmatrix_equal.py compares both
 * forms in one process); the default is NAFP_NONMATRIX_DEFAULT, 0 selects the earlier forms.
 *   CONV0        b0.conv1x3 as straight-line code: counted waits instead of a full drain per batch of positions, inputs staged with
 *                their zero padding, no per-position division (conv0_lean_kernel, conv.hip).
 *                Taken at the default 16 rows per workgroup only: with the A/B knob NAFP_CONV0_ROWS at another value, and in the
 *                training forward, conv0_kernel runs whatever this bit says (same bytes).
 *   KEEP_OWN     the two-part split-K launches that finish in-kernel: the last arriver adds the other part to the accumulators it
 *                still holds instead of storing its own part and reading both back (conv_gemm_body, EPI 4).
 * The process-wide default can be set with the environment variable NAFP_NONMATRIX (a mask, read when a handle is created). */
#define NAFP_OPT_NONMATRIX 8
#define NAFP_NONMATRIX_CONV0 1
#define NAFP_NONMATRIX_KEEP_OWN 2
#define NAFP_NONMATRIX_ALL 3
#define NAFP_NONMATRIX_DEFAULT NAFP_NONMATRIX_ALL
/* Options are host-side state of the handle: set them while no pass of the handle is being enqueued from another thread; passes already
 * enqueued keep what they were launched with.  (NAFP_OPT_BF16X3 = 2 allocates its split weights, 1.5 x the packed conv kernels, on first use.) */
int nafp_encoder_set_option(nafp_encoder* enc, int option, int value);

/* m_fp.div_enc(x) alone (nnfp.py:141-156; called separately at trainer.py:73-76). */
int nafp_encoder_div_enc(nafp_encoder* enc, const float* flat, int64_t n_seg,
                         float* out_emb, int l2norm, void* stream);

/* tf.math.l2_normalize(x, axis=1) of a (n_rows, dim) array: x * rsqrt(max(sum x^2, 1e-12)), as test_step
 * applies it to front_conv's and div_enc's outputs (trainer.py:74, 76).  out may alias x. */
int nafp_l2_normalize_rows(const float* x, int64_t n_rows, int dim, float* out, void* stream);

/* Send buffer of the embedding-gradient reduce-scatter (the backward of the all-gather at model/fp/NTxent_loss_tpu.py:57-87,
 * neural-audio-fp_amd/model/trainer.py scatter_embedding_gradients), packed in ONE launch:
 *   send[r, 0 : n_anchors*d]            = d_a_all[r*n_anchors : (r+1)*n_anchors, :]      r = destination rank
 *   send[r, n_anchors*d : 2*n_anchors*d] = d_b_all[r*n_anchors : (r+1)*n_anchors, :]
 *   send[r, 2*n_anchors*d : +4]          = loss_sum[0] * loss_scale                      (the loss rides in a 4-float tail)
 * d_a_all, d_b_all (world*n_anchors, d); send (world, 2*n_anchors*d + 4); all device pointers. */
int nafp_pack_embedding_grads(const float* d_a_all, const float* d_b_all, const float* loss_sum, float loss_scale,
                              int64_t world, int64_t n_anchors, int dim, float* send, void* stream);

/* ------------------------------------------------------------------------
 * NT-Xent loss (model/fp/NTxent_loss_single_gpu.py:52-82; sharded form
 * model/fp/NTxent_loss_tpu.py:90-137)
 * ---------------------------------------------------------------------- */

int64_t nafp_ntxent_workspace_bytes(int64_t n_local, int64_t n_global);

/* Rows of this rank: emb_org_local/emb_rep_local (n_local, d); columns: the
 * (all-gathered) emb_org_all/emb_rep_all (n_global, d); this rank's rows sit at
 * [rank_offset, rank_offset+n_local) of the global arrays.  Single device:
 * local == all, rank_offset = 0.
 *   loss_sum  out, 1 float: sum over local rows of (CE_a + CE_b); the caller
 *             divides by n_global for the reference's mean (and all-reduces)
 *   sim_mtx   optional (n_local, 2*n_global-1): [ab | aa without its diagonal]
 *             as compute_loss returns it; NULL to skip
 *   d_org_all/d_rep_all optional (n_global, d): gradient of (loss_sum/n_global)
 *             w.r.t. the global arrays contributed by this rank's rows AND
 *             columns restricted to local rows (sum over ranks = full gradient);
 *             NULL to skip.  d (MODEL.EMB_SZ, nnfp.py:250) is 64, 128 or 256. */
int nafp_ntxent_forward(const float* emb_org_local, const float* emb_rep_local,
                        const float* emb_org_all, const float* emb_rep_all,
                        int64_t n_local, int64_t n_global, int64_t rank_offset, int d,
                        float tau, float* loss_sum, float* sim_mtx,
                        float* d_org_all, float* d_rep_all,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Spec-augment (train step only): SpecNCutout with uniform_mask=True
 * (model/fp/specaug_chain/layers/ncutout_tarray.py:214-268)
 * ---------------------------------------------------------------------- */

/* A hole: frequency rows [f0, f1] x frames [t0, t1], INCLUSIVE on both ends
 * (generate_single_mask, ncutout_tarray.py:117-128). */
typedef struct { int f0, f1, t0, t1; } nafp_rect;

/* In place on feat (n_seg, F, T): elements inside any of the <= 8 holes become fill_value for the
 * samples whose `active` flag is set (active == NULL: every sample).  T % 4 == 0. */
int nafp_specaug_apply(float* feat, int64_t n_seg, int F, int T, const nafp_rect* rects_host,
                       int n_rects, const unsigned char* active, float fill_value, void* stream);

/* The same with the fill value read from device memory (hole_fill = 'min' fills with reduce_mean(x),
 * ncutout_tarray.py:203-204: nafp_specaug_mean leaves that mean on the device, no host round trip). */
int nafp_specaug_apply_fill_dev(float* feat, int64_t n_seg, int F, int T, const nafp_rect* rects_host,
                                int n_rects, const unsigned char* active, const float* fill_value_dev,
                                void* stream);
/* mean_out[0] = mean of the n floats of feat (16-byte aligned), summed in double in a fixed order. */
int64_t nafp_specaug_mean_workspace_bytes(void);
int nafp_specaug_mean(const float* feat, int64_t n, float* mean_out, void* workspace, int64_t workspace_bytes,
                      void* stream);

/* The general form of the masking: SpecNCutout with uniform_mask=False (a rectangle set and an activation draw per sample and
 * hole, ncutout_tarray.py:131-186, 270-276) and / or a filler TENSOR (hole_fill = 'random' | [min_mag, max_mag], :106-115,
 * 200-211: the layer's noise tensor, drawn once, scaled to the batch's value range on every call).
 *   rects_dev   (n_sets, n_rects, 4) int32 in device memory: f0, f1, t0, t1, inclusive; n_sets == 1 (one set for the batch) or
 *               n_seg (one per sample); n_rects <= 32
 *   active_dev  (n_seg, n_rects) bytes or NULL (every hole of every sample)
 *   filler      (n_fill_seg, F, T) floats, 16-byte aligned, or NULL (reads as 1); sample b uses row b % n_fill_seg
 *   scale_offset_dev  2 floats in device memory: a hole element becomes filler * scale + offset
 * nafp_specaug_range leaves {max - min, min} of feat on the device (the 'random' filler's scale and offset, :207-208); it takes
 * the workspace of nafp_specaug_mean. */
int nafp_specaug_apply_ex(float* feat, int64_t n_seg, int F, int T, const int32_t* rects_dev, int n_rects, int64_t n_sets,
                          const unsigned char* active_dev, const float* filler, int64_t n_fill_seg,
                          const float* scale_offset_dev, void* stream);
int nafp_specaug_range(const float* feat, int64_t n, float* scale_offset_out, void* workspace, int64_t workspace_bytes,
                       void* stream);

/* ------------------------------------------------------------------------
 * Optimizer steps of the train step (model/trainer.py:47-48, 119-140)
 * ---------------------------------------------------------------------- */

/* One parameter tensor with its gradient and moment slots (all device pointers, float32).
 * var_len = length of ONE keras variable inside the tensor: numel for the conv / LN tensors;
 * the stacked divide-and-encode tensors hold 128 variables each (var_len = numel / 128), and
 * LAMB takes its trust ratio per variable, as the reference does over its 576 variables.
 * nafp_adam_step and nafp_lamb_step check the WHOLE table before their first launch: a refused step leaves every tensor untouched. */
typedef struct {
    float* param; const float* grad; float* m; float* v;
    int64_t numel; int64_t var_len;
} nafp_opt_tensor;

/* tf.keras.experimental.CosineDecay(lr0, decay_steps, alpha) at `step` (trainer.py:119-124). */
float nafp_cosine_decay_lr_host(float lr0, int64_t step, int64_t decay_steps, float alpha);
/* tf.keras.experimental.CosineDecayRestarts(lr0, first_decay_steps, t_mul, m_mul, alpha) at `step`
 * (LR_SCHEDULE 'COS-RESTART', trainer.py:125-131). */
float nafp_cosine_decay_restarts_lr_host(float lr0, int64_t step, int64_t first_decay_steps, float t_mul,
                                         float m_mul, float alpha);

/* tf.keras.optimizers.Adam.apply_gradients (trainer.py:138): step is 1-based (iterations + 1);
 * keras defaults beta1 0.9, beta2 0.999, eps 1e-7. */
int nafp_adam_step(const nafp_opt_tensor* tensors_host, int n, float lr, float beta1, float beta2,
                   float eps, int64_t step, void* stream);

/* LAMB._resource_apply_dense (model/fp/lamb_optimizer.py:123-158): defaults beta1 0.9, beta2 0.999,
 * eps 1e-6, weight_decay 1e-6, decay and layer adaptation on every variable. */
int64_t nafp_lamb_workspace_bytes(const nafp_opt_tensor* tensors_host, int n);
int nafp_lamb_step(const nafp_opt_tensor* tensors_host, int n, float lr, float beta1, float beta2,
                   float eps, float weight_decay, int64_t step, void* workspace,
                   int64_t workspace_bytes, void* stream);

/* Online triplet loss of the now-playing baseline: OnlineTripletLoss.compute_loss with use_anc_as_pos = True
 * (model/fp/online_triplet_loss.py:199-239; masks :98-121; distances :185-196).  mode 0 = 'semi-hard'
 * (training, trainer.py:160-164), 1 = 'all' (validation, :165-169), 2 = 'all-balanced' (:215-222), 3 = 'hardest'
 * (:223-227, with the reference's min over the MASKED matrix, i.e. hardest negative = 0).  n_pos = n_anchor * n_pos_per_anchor,
 * replicas in anchor order.  loss_out (1); pairwise_dist (n_anchor, n_pos + n_anchor) or NULL; d_anchor /
 * d_pos: gradients of the loss (both or neither).  All device pointers. */
int64_t nafp_triplet_workspace_bytes(int64_t n_anchor, int64_t n_pos);
int nafp_triplet_forward(const float* emb_anchor, const float* emb_pos, int64_t n_anchor, int64_t n_pos, int dim,
                         int mode, float margin, float* loss_out, float* pairwise_dist, float* d_anchor,
                         float* d_pos, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training batch assembly + time-domain augmentation on the device.  Replaces, per output row, the host
 * work of genUnbalSequence.__getitem__ (model/utils/dataloader_keras.py:223-311): load_audio
 * (model/utils/audio_utils.py:221-264), bg_mix_batch (:82-117, background_mix :28-72) and
 * ir_aug_batch (:120-137).  All windows index ONE int16 PCM arena; the random draws (offsets, SNR,
 * amplitude ratio) are made by the caller, as the reference makes them on the host.
 * ------------------------------------------------------------------------------------------- */
typedef struct nafp_aug_row {
    int64_t ev_off;      /* event window: first sample in the arena                                   */
    int64_t nz_off;      /* background window (same length), or -1                                    */
    int64_t nz2_off;     /* second noise window added to the first (speech), or -1                    */
    int64_t ir_off;      /* impulse response, or -1                                                   */
    int32_t ev_valid;    /* real samples of the event window (<= seg_len; the tail is zero)           */
    int32_t nz_valid, nz2_valid;
    int32_t ir_len;      /* taps used (<= 600 = MAX_IR_LENGTH, dataloader_keras.py:8)                 */
    float snr_db;        /* bg_mix_batch's uniform draw in snr_range (audio_utils.py:92-95)           */
    float amp;           /* its log-uniform amplitude ratio in (0.1, 1) (audio_utils.py:98-99)        */
    int32_t mix;         /* 1: run bg_mix_batch's arithmetic for this row (replicas with BG/speech)   */
    int32_t reserved;
} nafp_aug_row;

/* out (n_rows, seg_len) float32; rows is a DEVICE array.  A row with mix = 0 and ir_off = -1 is the
 * plain window / 2^15 (the anchors).  seg_len % 4 == 0. */
int nafp_augment_rows(const int16_t* pcm, const nafp_aug_row* rows, int64_t n_rows, int seg_len, float* out,
                      void* stream);

/* Speed augmentation: replicas played at another speed (tempo and pitch together), inside the same launch.
 *
 * A SPEED ROW is a row whose event window is not pcm[ev_off .. ev_off + ev_valid) (both fields are ignored for it) but seg_len
 * consecutive outputs of the varispeed contract above (nafp_varispeed_i16: table of 513 phases, integer interpolation, int64
 * sum, round, clamp to int16) applied to the row's file:
 *   file  = the samples [file_off, file_off + n_in) of the arena; everything outside it counts as zero, so a neighbouring
 *           file's samples never enter;
 *   y[n]  = output n of that contract at the step steps[slot], for n in [out0, out0 + seg_len);  y[n] = 0 for
 *           n >= nafp_varispeed_n_out(n_in, step);
 *   x[i]  = y[out0 + i] / 2^15,  then the rest of the row's chain unchanged: mix, max-normalise, amp, IR, max-normalise.
 * Integer arithmetic only up to x[]: a speed row's bytes are those of nafp_augment_rows on a window that holds
 * nafp_varispeed_i16's outputs, whatever else shares the launch.
 * Step: the Q24 count of input samples per output sample.  A replica played s times too fast has step = round(2^24 s); such
 * audio is what `identify --speeds s` undoes.  (The filter at step 2^24 is a 0.95-Nyquist low-pass, not the identity: callers
 * that mean "no speed change" use slot -1.)
 * One entry per row, parallel to the nafp_aug_row table.  32 bytes. */
typedef struct nafp_aug_speed {
    int64_t file_off;    /* first sample of the row's file in the arena                                */
    int64_t n_in;        /* samples of the file (< 2^31)                                               */
    int64_t out0;        /* index in the file's stretched stream of the row's first output (>= 0)      */
    int32_t slot;        /* index into the step set, or -1: the row is exactly as nafp_augment_rows treats it */
    int32_t reserved;
} nafp_aug_speed;

typedef struct nafp_aug_speedset nafp_aug_speedset;

/* 1 .. 32 steps, each within NAFP_VARISPEED_STEP_MIN .. NAFP_VARISPEED_STEP_MAX (otherwise NAFP_ERR_UNSUPPORTED; no steps, more
 * than 32 or null pointers NAFP_ERR_INVALID_ARG).  The set owns the tables of its steps: designed here on the host, as
 * nafp_varispeed_create designs them, and uploaded in that kernel's device layout by the set's first launch on the device that
 * is current then (so a set can be created, and tables checked against it, without a GPU). */
int nafp_aug_speedset_create(nafp_aug_speedset** set, const uint32_t* steps, int n_steps);
int nafp_aug_speedset_destroy(nafp_aug_speedset* set);
/* Host only: the checks the kernel makes per row, on host copies of both tables, before they are uploaded.  A seg_len the speed
 * path cannot hold (below) or an n_in >= 2^31 NAFP_ERR_UNSUPPORTED; a slot outside [-1, n_steps), a negative out0 (or one
 * beyond 2^32), a file range outside [0, pcm_samples) NAFP_ERR_INVALID_ARG.  Rows with slot -1 are not looked at. */
int nafp_augment_speed_check_host(const nafp_aug_speedset* set, const nafp_aug_row* rows_host, const nafp_aug_speed* speeds_host,
                                  int64_t n_rows, int64_t pcm_samples, int seg_len);
/* nafp_augment_rows with speed rows.  speeds: DEVICE array of n_rows entries, or NULL.  speeds == NULL (set may be NULL then)
 * or every slot -1 gives nafp_augment_rows's bytes; rows with slot -1 take its path.  The input span of a speed row is staged
 * in the row's noise buffer as int16, so the launch uses the dynamic LDS of nafp_augment_rows; with speeds != NULL a seg_len
 * whose widest span ((seg_len - 1) * 1.25 + 89 samples) exceeds 2 * seg_len int16, i.e. seg_len < 116, is
 * NAFP_ERR_UNSUPPORTED before any launch.  Every index derived from a speed entry is checked on the device against
 * pcm_samples: an inconsistent entry (as nafp_augment_speed_check_host refuses it) gives a zero event for that row and no
 * access outside the arena. */
int nafp_augment_rows_speed(nafp_aug_speedset* set, const int16_t* pcm, int64_t pcm_samples, const nafp_aug_row* rows,
                            const nafp_aug_speed* speeds, int64_t n_rows, int seg_len, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Search / evaluation over resident fingerprints (consumer of the generate path's output).
 * Replaces faiss.IndexFlatL2 as eval/eval_faiss.py uses it with index_type 'L2'
 * (eval/utils/get_index_faiss.py:57-62; index.add at eval_faiss.py:145-146; index.search at :209)
 * and the sequence-score loop of eval_faiss.py:221-230.  The index is the caller's device array
 * [dummy_db ; db] (n_index x dim float32, dim 64 or 128); nothing is trained or quantised.
 * ------------------------------------------------------------------------------------------- */

/* floats of the auxiliary array (|x|^2/2 per row, padded) nafp_search_index_prepare fills */
int64_t nafp_search_index_aux_floats(int64_t n_index);
int nafp_search_index_prepare(const float* index, int64_t n_index, int dim, float* aux, void* stream);

int64_t nafp_search_workspace_bytes(int64_t n_query, int64_t n_index, int k);
/* out_dist / out_ids (n_query, k): the k smallest squared L2 distances and their row ids, nearest
 * first; fewer than k rows: id -1, distance +inf.  k <= 32.
 * Order: by the float32 key q.x - |x|^2/2, descending, then by id, ascending (equal rows: smaller id first).
 * The distance written is max(|q|^2 - 2 key, 0) in float32 and is non-decreasing along a row; two distinct
 * keys can round to the same distance, so equal written distances are not always in id order.
 * An index row with a NaN or an infinite element is never returned and does not disturb the other rows; a
 * query row with a NaN gets k times id -1, +inf, and does not disturb the other queries. */
int nafp_search_topk_l2(const float* query, int64_t n_query, const float* index, const float* aux,
                        int64_t n_index, int dim, int k, float* out_dist, int32_t* out_ids,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* nafp_search_topk_l2 with a row range left out per query: excl (n_query, 2) int32, a DEVICE array of pairs (lo, hi); query q
 * gets the result nafp_search_topk_l2 would give on the index rows outside [lo_q, hi_q), with the ids of the whole index.  A
 * self-join of a library (every row a query, its own track excluded) is the use: the exclusion happens inside the selection,
 * before a row enters a list of k, so the k survivors are kept however many excluded rows are nearer.
 *   - unchanged from nafp_search_topk_l2: the float32 key q.x - |x|^2/2 and the order (key descending, then id ascending), the
 *     distance written, the padding (id -1, distance +inf) when fewer than k rows survive, the NaN / Inf rules, k <= 32;
 *   - lo and hi are clipped to [0, n_index] when they are loaded, each by comparisons (no difference is formed, so nothing
 *     overflows): ANY int32 pair is legal, lo > hi, negative values, INT32_MIN / INT32_MAX included.  A pair with lo >= hi
 *     after clipping excludes nothing; (INT32_MIN, INT32_MAX) excludes every row.  excl is only ever compared with row
 *     numbers: it is never an address or an index into `index`;
 *   - with every range empty out_dist and out_ids equal nafp_search_topk_l2's byte for byte;
 *   - bit-identical from run to run; a query's row does not depend on what shares the launch;
 *   - workspace: nafp_search_workspace_bytes(n_query, n_index, k), the same split plan and the same merge.
 * Status, before any GPU call, as nafp_search_topk_l2: NAFP_ERR_INVALID_ARG for a null pointer (excl included), n_query < 0,
 * n_index <= 0 or k <= 0; NAFP_ERR_UNSUPPORTED for dim outside 64 / 128 / 256, k > 32, n_index >= 2^31 or n_query > 2^30;
 * n_query == 0 returns NAFP_OK without a launch; NAFP_ERR_WORKSPACE for a workspace that is too small. */
int nafp_search_topk_l2_excl(const float* query, int64_t n_query, const float* index, const float* aux,
                             int64_t n_index, int dim, int k, const int32_t* excl, float* out_dist, int32_t* out_ids,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* out_scores[t, s] = mean_{i < min(task_len[t], n_index - c)} query[task_q0[t] + i] . index[c + i]
 * for the candidate sequence start c = cand[t, s] (>= 0; -1 -> -inf): np.mean(np.diag(np.dot(q,
 * index[c:c+l].T))) of eval_faiss.py:224-230.  All device pointers. */
int nafp_search_seq_scores(const float* query, const float* index, int64_t n_index, int dim,
                           const int32_t* task_q0, const int32_t* task_len, int64_t n_tasks,
                           const int32_t* cand, int n_slots, float* out_scores, void* stream);

/* Sequence matching in one launch: from the top-k ids of the segment search to the ranked predictions
 * (the candidate / unique / score / argsort part of the loop, eval_faiss.py:213-232).  One task t = one
 * query sequence: rows task_q0[t] .. of `query`, topk_ids (n_query, k) = the search result per query row
 * (-1 = none).  All device pointers; no workspace.
 *   - effective length  len_t = min(task_len[t], max_len, n_query - task_q0[t]); a task with task_q0[t]
 *     outside [0, n_query) or len_t <= 0 has no candidates;
 *   - candidates of t: the DISTINCT values c = topk_ids[task_q0[t] + i, j] - i over i < len_t, j < k with
 *     0 <= topk_ids[..] < n_index and c >= 0.  Entries of topk_ids outside [0, n_index) are treated as
 *     absent (this is also what keeps every read inside `index`);
 *   - score(c) = mean_{i < min(len_t, n_index - c)} query[task_q0[t] + i] . index[c + i], the fp32
 *     arithmetic of nafp_search_seq_scores in the same order: the same bits;
 *   - a candidate whose score is NaN or -inf is dropped;
 *   - out_ids / out_scores (n_tasks, n_out): the n_out best candidates, score descending, equal scores:
 *     smaller id first; padding id -1, score -inf.  out_n_cand (n_tasks,) or NULL: the number of distinct
 *     candidates that were not dropped;
 *   - bit-identical from run to run; a task's rows do not depend on what else is in the launch.
 * Status, before any GPU call: NAFP_ERR_INVALID_ARG for a null pointer (out_n_cand excepted) or a negative
 * size; NAFP_ERR_UNSUPPORTED for dim outside 64 / 128 / 256, k outside 1..32, max_len < 1,
 * k * max_len > 2048, n_out outside 1..32, n_index >= 2^31 (n_query, n_tasks likewise); n_tasks == 0
 * returns NAFP_OK without a launch. */
int nafp_search_seq_match(const float* query, int64_t n_query, const float* index, int64_t n_index, int dim,
                          const int32_t* topk_ids, int k, const int32_t* task_q0, const int32_t* task_len,
                          int64_t n_tasks, int max_len, int n_out, int32_t* out_ids, float* out_scores,
                          int32_t* out_n_cand, void* stream);

/* Identification: the track-aware sequence matcher.  `index` is the row array of a library of tracks laid end to end,
 * track_first (n_tracks + 1, strictly increasing, [0] == 0, [n_tracks] == n_index) the first row of each track.  One task t =
 * one analysis window of one recording: rows task_q0[t] .. of `query`, topk_ids (n_query, k) = the segment search result
 * per query row.  All array arguments are device pointers; no workspace.  Unlike nafp_search_seq_match, an alignment may be
 * negative or lie before its track (a recording that starts before the track does), a window is scored only where it
 * overlaps its track (never against the next track's rows), votes are counted, and a task may have 8192 slots.
 *   - len_t = min(task_len[t], max_len, n_query - task_q0[t]); a task with task_q0[t] outside [0, n_query) or len_t <= 0
 *     has no candidates;
 *   - candidates: every slot (i < len_t, j < k) with id = topk_ids[task_q0[t] + i, j] in [0, n_index) gives the pair
 *     (tr, a): tr the track with first[tr] <= id < first[tr + 1], a = id - i the alignment, the index row segment 0 of the
 *     window falls on (any sign).  A candidate is a DISTINCT pair; the same a through two tracks is two candidates;
 *   - votes v(tr, a): the number of slots that gave the pair;
 *   - overlap: i0 = max(0, first[tr] - a), i1 = min(len_t, first[tr + 1] - a), n_ov = i1 - i0 (>= 1).  A candidate with
 *     n_ov < min(min_overlap, len_t) or v < min_votes is dropped;
 *   - shortlist: the n_short best of the rest by votes descending, track ascending, a ascending; out_n_cand[t] (or NULL)
 *     counts the rest BEFORE this cut;
 *   - score of a shortlisted candidate = mean_{i0 <= i < i1} query[task_q0[t] + i] . index[a + i]: the bits of
 *     nafp_search_seq_scores for task_q0 = task_q0[t] + i0, task_len = n_ov, cand = a + i0 (the one summation order of the
 *     sequence score).  A NaN or -inf score drops the candidate;
 *   - out_track / out_align / out_score / out_votes / out_overlap (n_tasks, n_out): the n_out best by score descending,
 *     track ascending, a ascending; padding track -1, align 0, score -inf, votes 0, overlap 0;
 *   - bit-identical from run to run; a task's rows do not depend on what else is in the launch.
 * The kernel reads only rows [0, n_index) of `index` whatever track_first holds; nafp_search_identify_check_tracks_host
 * (host pointer) is the check of the table: NAFP_ERR_INVALID_ARG unless it is as stated above.
 * Status, before any GPU call: NAFP_ERR_INVALID_ARG for a null pointer (out_n_cand excepted) or a negative size;
 * NAFP_ERR_UNSUPPORTED for dim outside 64 / 128 / 256, k outside 1..32, max_len < 1, k * max_len > 8192, n_short outside
 * 1..256, n_out outside 1..32 or above n_short, min_overlap < 1, min_votes < 1, n_index > 2^31 - 2^14, n_tracks outside
 * 1..2^24 (n_query, n_tasks >= 2^31 likewise); n_tasks == 0 returns NAFP_OK without a launch. */
int nafp_search_identify(const float* query, int64_t n_query, const float* index, int64_t n_index, int dim,
                         const int32_t* topk_ids, int k,
                         const int32_t* task_q0, const int32_t* task_len, int64_t n_tasks, int max_len,
                         const int32_t* track_first, int n_tracks,
                         int min_overlap, int min_votes, int n_short, int n_out,
                         int32_t* out_track, int32_t* out_align, float* out_score,
                         int32_t* out_votes, int32_t* out_overlap, int32_t* out_n_cand, void* stream);
int nafp_search_identify_check_tracks_host(const int32_t* track_first_host, int n_tracks, int64_t n_index);

/* Identification under tempo hypotheses: nafp_search_identify along slanted lines, for a recording that was time-stretched
 * (tempo changed, pitch kept).  Under a tempo ratio rho, query segment i of a window falls on library row a + round(i * rho),
 * not a + i; every hypothesis is matched in this one launch on the same fingerprints.  The arguments are those of
 * nafp_search_identify plus rho_host (n_rho values, a HOST pointer: they travel in the kernel arguments) and out_rho.
 *   - hypothesis r < n_rho is rho_host[r], 16.16 fixed point, the library rows advanced per query segment;
 *     off_r(i) = (i * rho_host[r] + 32768) >> 16 (i < 8192, rho <= 81920: 32 bits hold it), non-decreasing in i;
 *   - len_t as in nafp_search_identify;
 *   - candidates: every slot (i < len_t, j < k) with id = topk_ids[task_q0[t] + i, j] in [0, n_index) gives, for EVERY r, the
 *     triple (tr, r, a): tr the track of id, a = id - off_r(i) (any sign).  A candidate is a DISTINCT triple; its votes are
 *     the number of slots that gave it;
 *   - overlap: i0 = the smallest i with a + off_r(i) >= first[tr], i1 = the smallest i with a + off_r(i) >= first[tr + 1],
 *     both clipped to [0, len_t], the track clipped to [0, n_index); n_ov = i1 - i0.  A candidate with
 *     n_ov < min(min_overlap, len_t), n_ov == 0 or votes < min_votes is dropped;
 *   - shortlist: the n_short best of the rest by votes descending, then tr, r, a ascending; out_n_cand[t] (or NULL) counts
 *     the rest BEFORE this cut;
 *   - score of a shortlisted candidate = mean_{i0 <= i < i1} query[task_q0[t] + i] . index[a + off_r(i)], in the one summation
 *     order of the sequence score: the bits of nafp_search_seq_scores on the rows index[a + off_r(i)] gathered into an array
 *     of their own.  A NaN or -inf score drops the candidate;
 *   - out_track / out_align / out_score / out_votes / out_overlap / out_rho (n_tasks, n_out): the n_out best by score
 *     descending, then tr, r, a ascending (of two hypotheses that give the same rows, the one first in rho_host); padding
 *     track -1, align 0, rho -1, score -inf, votes 0, overlap 0.  out_rho holds r, the place in rho_host;
 *   - every index row read lies inside its track and inside [0, n_index), whatever topk_ids or track_first hold;
 *   - bit-identical from run to run; a task's rows do not depend on what else is in the launch;
 *   - with rho_host = {65536} every array equals nafp_search_identify's byte for byte (out_rho 0, padding -1).
 * Status, before any GPU call: NAFP_ERR_INVALID_ARG for a null pointer (out_n_cand excepted) or a negative size;
 * NAFP_ERR_UNSUPPORTED for n_rho outside 1..16, a rho outside 52429..81920 (0.8 .. 1.25), k * max_len * n_rho > 8192 and
 * every limit of nafp_search_identify; n_tasks == 0 returns NAFP_OK without a launch. */
int nafp_search_identify_tempo(const float* query, int64_t n_query, const float* index, int64_t n_index, int dim,
                               const int32_t* topk_ids, int k,
                               const int32_t* task_q0, const int32_t* task_len, int64_t n_tasks, int max_len,
                               const int32_t* track_first, int n_tracks,
                               const int32_t* rho_host, int n_rho,
                               int min_overlap, int min_votes, int n_short, int n_out,
                               int32_t* out_track, int32_t* out_align, float* out_score,
                               int32_t* out_votes, int32_t* out_overlap, int32_t* out_n_cand, int32_t* out_rho, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Approximate indexes: IVF-Flat and IVF-PQ (faiss IndexIVFFlat / IndexIVFPQ as
 * eval/utils/get_index_faiss.py:64-80 builds them; opt-in from eval_faiss.py).  Building blocks of
 * training and add (bucketing, k-means update, PQ encoding) and the two searches.  dim 64 / 128 / 256;
 * PQ: M = 64 sub-quantizers of 256 codewords (pq_centroids (M, 256, dim / M) float32), codes (n, M) uint8.
 * Ties everywhere: the smaller id (list, code, row) first; for nafp_ivf_flat_search a tie is a tie of the float32 key
 * q.x - |x|^2/2, as in nafp_search_topk_l2: the distances written are non-decreasing, and two distinct keys that round to
 * the same distance keep their key order.  All pointers are device pointers; results
 * are bit-identical from run to run and do not depend on how rows or queries are batched.
 * Status: NAFP_ERR_INVALID_ARG for a null pointer or a negative size, NAFP_ERR_UNSUPPORTED for a dim
 * outside 64 / 128 / 256, k > 32 (k1 > 128 for the wide first stage of IVFPQ-RR), nprobe > 128, M != 64, n_buckets / nlist > 16384 or an unknown lut;
 * checked before any GPU call.  The *_workspace_bytes queries return -1 for such arguments.
 * ------------------------------------------------------------------------------------------- */

/* Stable counting sort of `batch` key arrays: key (b, i) = keys[i * batch + b] (int32 or uint8 by
 * key_bytes), 0 <= key < n_buckets (others are dropped).  offsets (batch, n_buckets + 1): bucket starts;
 * ids (batch, n): item ids i grouped by key, ascending inside a bucket. */
int64_t nafp_ivf_bucket_workspace_bytes(int64_t n, int n_buckets, int batch);
int nafp_ivf_bucket(const void* keys, int key_bytes, int64_t n, int n_buckets, int batch, int32_t* offsets,
                    int32_t* ids, void* workspace, int64_t workspace_bytes, void* stream);

/* k-means update on bucketed points: sort b (of batch) covers coordinates [b * dim / batch, (b + 1) *
 * dim / batch) of the rows x (n, dim); centroids (batch, n_buckets, dim / batch) of non-empty buckets
 * become the mean of their points (summed in id order, in double); empty ones are left as they are.
 * counts (batch, n_buckets) receives the bucket sizes. */
int nafp_ivf_kmeans_update(const float* x, int64_t n, int dim, int batch, const int32_t* offsets,
                           const int32_t* ids, int n_buckets, float* centroids, int32_t* counts, void* stream);

/* out (n, dim) = x - centroids[assign] */
int nafp_ivf_residuals(const float* x, int64_t n, int dim, const int32_t* assign, const float* centroids,
                       float* out, void* stream);

/* codes (n, M): per sub-space the nearest codeword of x - coarse[assign] (assign and coarse both NULL:
 * of x itself). */
int nafp_ivf_pq_encode(const float* x, int64_t n, int dim, const int32_t* assign, const float* coarse,
                       const float* pq_centroids, int M, uint8_t* codes, void* stream);

/* probe (n_query, nprobe): the nprobe nearest of nlist centroids per query, nearest first (nprobe <= nlist). */
int nafp_ivf_probe(const float* query, int64_t n_query, const float* centroids, int nlist, int dim, int nprobe,
                   int32_t* probe, void* stream);

/* IVF-Flat list storage: rows (bound, dim), half_norms (bound), row_ids (bound) with bound =
 * nafp_ivf_flat_rows_bound(n, nlist); list l holds rows [row_offsets[l], row_offsets[l + 1]) (nlist + 1
 * entries), padded to whole 64-row tiles (row id -1).  offsets / ids: nafp_ivf_bucket of the rows' lists. */
int64_t nafp_ivf_flat_rows_bound(int64_t n, int nlist);
int nafp_ivf_flat_lists(const float* x, int64_t n, int dim, const int32_t* offsets, const int32_t* ids, int nlist,
                        int32_t* row_offsets, float* rows, float* half_norms, int32_t* row_ids, void* stream);
/* IVF-PQ list storage: codes_sorted[p] = codes[ids[p]] (n rows of M bytes). */
int nafp_ivf_pq_lists(const uint8_t* codes, int64_t n, int M, const int32_t* ids, uint8_t* codes_sorted,
                      void* stream);

/* kind 0: IVF-Flat, 1: IVF-PQ.  nprobe is clamped to nlist. */
int64_t nafp_ivf_search_workspace_bytes(int64_t n_query, int nlist, int nprobe, int k, int kind);
/* out_dist / out_ids (n_query, k): the k nearest rows of the nprobe nearest lists; exact fp32 squared L2
 * distances; fewer than k rows: id -1, distance +inf. */
int nafp_ivf_flat_search(const float* query, int64_t n_query, const float* centroids, int nlist, int dim,
                         int nprobe, const float* rows, const float* half_norms, const int32_t* row_offsets,
                         const int32_t* row_ids, int k, float* out_dist, int32_t* out_ids, void* workspace,
                         int64_t workspace_bytes, void* stream);
/* The same with the ADC distance sum_m |(q - c_list)_m - P[m][code_m]|^2 from fp32 tables (codes_sorted /
 * offsets / ids: the lists as nafp_ivf_pq_lists and nafp_ivf_bucket leave them). */
int nafp_ivf_pq_search(const float* query, int64_t n_query, const float* centroids, int nlist, int dim, int nprobe,
                       const float* pq_centroids, int M, const uint8_t* codes_sorted, const int32_t* offsets,
                       const int32_t* ids, int k, float* out_dist, int32_t* out_ids, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* Precision of the IVF-PQ ADC (asymmetric distance) lookup tables.  Entry T[m][c] of the table of a (query,
 * list) pair is computed in fp32 either way: residual rr = q - centroids[list], then sum_u (rr[m * dsub + u] -
 * P[m][c][u])^2 with u ascending.
 *   NAFP_IVF_LUT_F32  the entries are kept as they are (the default everywhere).
 *   NAFP_IVF_LUT_F16  each entry is rounded ONCE to IEEE binary16, round to nearest even, gradual underflow
 *                     kept (with dim / M = 1 or 2 many entries are fp16 subnormals) -- the lookup tables of the
 *                     reference's GPU index (faiss useFloat16).  Entries above the binary16 range (65504) are
 *                     outside the contract; fingerprints are unit vectors, so real entries are at most 4.
 * Either way a row's distance is the sum over m = 0 .. 63, in that order, of its entries widened to fp32
 * and added in fp32; ties: the smaller id first. */
#define NAFP_IVF_LUT_F32 0
#define NAFP_IVF_LUT_F16 1

/* nafp_ivf_pq_search with the table precision chosen; lut = NAFP_IVF_LUT_F32 is nafp_ivf_pq_search, byte for
 * byte.  Workspace: nafp_ivf_search_workspace_bytes(..., kind 1), for either value. */
int nafp_ivf_pq_search_ex(const float* query, int64_t n_query, const float* centroids, int nlist, int dim,
                          int nprobe, const float* pq_centroids, int M, const uint8_t* codes_sorted,
                          const int32_t* offsets, const int32_t* ids, int k, float* out_dist, int32_t* out_ids,
                          int lut, void* workspace, int64_t workspace_bytes, void* stream);

/* The ADC tables themselves, as the search builds them, for n_pairs (query row, list) pairs given as two
 * device int32 arrays: out is (n_pairs, M, 256) float32 (lut 0) or binary16 (lut 1).  A pair that names a row
 * outside [0, n_query) or a list outside [0, nlist) gets NaNs.  A building block (re-use, tests). */
int nafp_ivf_pq_adc_tables(const float* query, int64_t n_query, const int32_t* pair_query,
                           const int32_t* pair_list, int64_t n_pairs, const float* centroids, int nlist, int dim,
                           const float* pq_centroids, int M, int lut, void* out, void* stream);

/* IVFPQ-RR (faiss IndexIVFPQR as eval/utils/get_index_faiss.py builds it: IVF-PQ plus a refine product
 * quantizer of M_refine = 4 sub-spaces x 2^4 codewords on the PQ stage's own residuals, and a re-ranking of
 * k * k_factor first-stage candidates by the distance to the refined reconstruction).  refine_centroids
 * (4, 16, dim / 4) float32; refine codes 2 bytes per row in insertion order, byte0 = c0 | c1 << 4, byte1 =
 * c2 | c3 << 4.  Other M_refine / nbits_refine: NAFP_ERR_UNSUPPORTED. */

/* out (n, dim) = x - decode(codes): x minus the PQ codewords its codes (n, M) name.  n * dim < 2^32 (one launch);
 * more rows: NAFP_ERR_UNSUPPORTED, call it in pieces. */
int nafp_ivf_pq_residuals(const float* x, int64_t n, int dim, const float* pq_centroids, int M, const uint8_t* codes,
                          float* out, void* stream);
/* per row of x (n, dim) and refine sub-space the nearest of the 16 codewords (equal distances: the smaller
 * code).  packed 1: codes (n, 2) as above; packed 0: codes (n, 4), one code per byte (bucketing keys). */
int nafp_ivf_refine_encode(const float* x, int64_t n, int dim, const float* refine_centroids, int M_refine,
                           int nbits_refine, int packed, uint8_t* codes, void* stream);

/* The wide first stage: nafp_ivf_pq_search_ex's contract (tables, distances, order, padding) for k1 <= 128
 * results per query.  nafp_ivf_pq_search[_ex] itself keeps refusing k > 32.  Workspace of this call and of
 * nafp_ivf_pqr_search (with k1 = k * k_factor): nafp_ivf_pq_wide_workspace_bytes; -1 for k1 > 128. */
int64_t nafp_ivf_pq_wide_workspace_bytes(int64_t n_query, int nlist, int nprobe, int k1);
int nafp_ivf_pq_search_wide(const float* query, int64_t n_query, const float* centroids, int nlist, int dim,
                            int nprobe, const float* pq_centroids, int M, const uint8_t* codes_sorted,
                            const int32_t* offsets, const int32_t* ids, int k1, float* out_dist, int32_t* out_ids,
                            int lut, void* workspace, int64_t workspace_bytes, void* stream);
/* The re-rank: for each of the k1 <= 128 candidate rows cand_ids (n_query, k1) names (-1: none), dist = sum over
 * dd ascending of (q[dd] - ((centroids[assign[id]][dd] + P[m][code_m][u]) + R[mr][rcode_mr][u']))^2 in fp32;
 * out (n_query, k), k <= 32 and <= k1: the k smallest by (distance, id), padded with +inf / -1.  assign (n_rows),
 * codes (n_rows, M) and refine_codes (n_rows, 2) are in insertion order. */
int nafp_ivf_pqr_rerank(const float* query, int64_t n_query, int dim, const int32_t* cand_ids, int k1,
                        const float* centroids, const int32_t* assign, const float* pq_centroids, int M,
                        const uint8_t* codes, const float* refine_centroids, int M_refine, int nbits_refine,
                        const uint8_t* refine_codes, int64_t n_rows, int k, float* out_dist, int32_t* out_ids,
                        void* stream);
/* Both stages: nafp_ivf_pq_search_wide for k1 = k * k_factor (k <= 32, k_factor 1 .. 4) into stage1_dist /
 * stage1_ids (n_query, k1; required), then nafp_ivf_pqr_rerank of those into out_dist / out_ids (n_query, k). */
int nafp_ivf_pqr_search(const float* query, int64_t n_query, const float* centroids, int nlist, int dim, int nprobe,
                        const float* pq_centroids, int M, const uint8_t* codes_sorted, const int32_t* offsets,
                        const int32_t* ids, const int32_t* assign, const uint8_t* codes,
                        const float* refine_centroids, int M_refine, int nbits_refine, const uint8_t* refine_codes,
                        int64_t n_rows, int k, int k_factor, float* out_dist, int32_t* out_ids, float* stage1_dist,
                        int32_t* stage1_ids, int lut, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * HNSW (csrc/hnsw.hip; host side eval/hnsw.py; float64 restatement tests/_hnsw_ref.py): faiss IndexHNSWFlat as
 * get_index_faiss.py:88-96 builds it, with a DETERMINISTIC ROUND-BASED build: every result below is a pure function of
 * (rows, level draws, parameters), and every loop has a static bound.
 *
 * Parameters: M = 16 links per row on levels >= 1, 2 M = 32 on level 0; ef 1 .. 128; k <= 32; dim 64 / 128 / 256;
 * levels 0 .. 7 (drawn on the host: row i gets min(7, floor(-ln(u_i) / ln M))).  Distances are fp32 squared L2; every
 * ordering is by (distance, id) ascending.  A link list is in (distance to its owner, id) order, padded with -1.
 *
 * The lists of one level are given as (links, slot, n_link_rows, link_stride): row r's list is the 2 M (level 0) or M
 * int32 at links[(slot ? slot[r] : r) * link_stride]; a slot outside [0, n_link_rows) is a row without lists.
 * eval/hnsw.py keeps level 0 as (capacity, 32) without a slot map and levels 1 .. 7 as (n_slots, 7, 16) for the rows
 * of level >= 1 (level l at links_upper + (l - 1) * 16, stride 7 * 16).
 *
 * Layer search (faiss's search_bounded_queue): a pool of at most ef (distance, id, expanded) entries in order,
 * starting with the entry.  Repeat: take the nearest unexpanded entry c (none: stop), mark it, and let the pool
 * become the ef best of pool U (neighbours of c on that level not in the pool).  Stop also after max_expansions
 * expansions (nafp_hnsw_default_max_expansions: 4 ef + 256).  A neighbour rejected or evicted once can never enter
 * later (the pool's last entry only improves), so no visited set is part of the contract.  ef = 1: greedy descent.
 *
 * Selection (faiss's shrink heuristic, pruned entries not kept): walk the candidates in order without the owner and
 * duplicates; accept c unless an accepted a has dist(c, a) < dist(c, owner); stop at the list's length.
 *
 * A round inserts rows [row0, row0 + n_new) into the graph of rows < row0, which stays frozen while they search it
 * (rows of one round do not see each other).  Entry point ep: the row of highest level L among rows < row0, the
 * smallest id among equals.  Per new row i of level l_i: cur = ep; for level L .. l_i + 1: cur = search(ef 1)[0]; for
 * level min(l_i, L) .. 0: W = search(ef = efConstruction), list(i, level) = select(i, W), cur = W[0].  Then, per old
 * row j and level on which new rows chose it: U = old list U those rows; the list becomes U in order if it fits,
 * select(j, U) otherwise -- a function of the set U alone.  eval/hnsw.py rounds: n_new = min(max(1, row0 / 8), 16384).
 *
 * Status: null pointers / negative sizes NAFP_ERR_INVALID_ARG; dim outside 64 / 128 / 256, k > 32, ef > 128, M != 16,
 * level > 7: NAFP_ERR_UNSUPPORTED (the workspace queries: -1), all before any GPU call.
 * ------------------------------------------------------------------------------------------- */
int nafp_hnsw_default_max_expansions(int ef);       /* 4 ef + 256; -1 for ef outside 1 .. 128 */
int64_t nafp_hnsw_reverse_workspace_bytes(int64_t n_old, int64_t n_new, int M, int level);
int64_t nafp_hnsw_search_workspace_bytes(int64_t n_query, int ef_search, int k);
/* Per query row of query (n_query, dim): the layer search of `level` from entries[q] (a row id; outside [0, n_rows): an
 * empty result) over the rows x (n_rows, dim).  query_levels (or null): a query with query_levels[q] < level searches
 * with ef = 1 (the descent of a new row above its own levels).  out (n_query, n_out), n_out <= ef: the first n_out
 * pool entries, padded with +inf / -1.  entries must not overlap out_ids or out_dist: a query's block writes its
 * results when it ends, while other blocks may not have read their entry yet. */
int nafp_hnsw_search_layer(const float* x, int64_t n_rows, int dim, const int32_t* links, const int32_t* slot,
                           int64_t n_link_rows, int64_t link_stride, int M, int level, const float* query,
                           int64_t n_query, const int32_t* entries, const int32_t* query_levels, int ef,
                           int max_expansions, int n_out, float* out_dist, int32_t* out_ids, void* stream);
/* The forward selection of a round on one level: for each new row row0 + i with new_levels[i] >= level its list :=
 * select(row0 + i, candidates i) from cand (n_new, ef) as nafp_hnsw_search_layer wrote them (in order, -1 ends).
 * Rows with new_levels[i] < level are left alone. */
int nafp_hnsw_select_forward(const float* x, int64_t n_rows, int dim, int64_t row0, int64_t n_new,
                             const int32_t* new_levels, int level, int M, const float* cand_dist,
                             const int32_t* cand_ids, int ef, int32_t* links, const int32_t* slot, int64_t n_link_rows,
                             int64_t link_stride, void* stream);
/* The reverse links of a round on one level: every row j < row0 that the lists of the new rows (new_levels[i] >=
 * level) name gets those rows into its list, as above.  Integer atomics count the rows per target, a scan and a
 * scatter gather them in arbitrary order, and the target's wave walks old list U gathered rows in (distance, id)
 * order: the new list depends on the set only.  Workspace: nafp_hnsw_reverse_workspace_bytes(row0, n_new, M, level). */
int nafp_hnsw_reverse_links(const float* x, int64_t n_rows, int dim, int64_t row0, int64_t n_new,
                            const int32_t* new_levels, int level, int M, int32_t* links, const int32_t* slot,
                            int64_t n_link_rows, int64_t link_stride, void* workspace, int64_t workspace_bytes,
                            void* stream);
/* The search: from `entry` (of level entry_level) the layer search with ef = 1 on levels entry_level .. 1
 * (links_upper (n_slots, 7, M) and slot; may be null for entry_level 0), then with ef = max(ef_search, k) on level 0
 * (links0 (>= n_rows, 2 M)); out (n_query, k): its first k entries, padded with +inf / -1.  A query's result does not
 * depend on the other queries of the call. */
int nafp_hnsw_search(const float* x, int64_t n_rows, int dim, const int32_t* links0, const int32_t* links_upper,
                     const int32_t* slot, int64_t n_slots, int M, int entry, int entry_level, const float* query,
                     int64_t n_query, int ef_search, int k, float* out_dist, int32_t* out_ids, void* workspace,
                     int64_t workspace_bytes, void* stream);

/* In-training mini search test (model/utils/mini_search_subroutines.py): pairwise_distances_for_eval (:28-93;
 * mode 0 = squared L2 clipped at 0 for 'argmin', 1 = dot product for 'argmax'; any dim) into out_scores
 * (n_query, n_db); then, per sequence length `scope`, the rank of the ground-truth start id
 * (t + gt_id_offset) among all candidate starts under the eye(scope) diagonal sum (conv_eye_func :96-119 and
 * the argsort / np.where of mini_search_eval :180-205): out_rank (n_query - scope + 1) int32. */
int nafp_minisearch_scores(const float* query, const float* db, int64_t n_query, int64_t n_db, int dim, int mode,
                           float* out_scores, void* stream);
int nafp_minisearch_ranks(const float* scores, int64_t n_query, int64_t n_db, int scope, int mode, int gt_id_offset,
                          int32_t* out_rank, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NAFP_H */
