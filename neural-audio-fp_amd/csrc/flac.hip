// FLAC frames decoded to interleaved little-endian PCM (s16 or s24 containers, MSB-justified) in a byte arena, gfx950.  A pre-pass of
// the ingest (ingest.hip, unchanged), which reads this arena as NAFP_INGEST_S16 / NAFP_INGEST_S24.
//
// Contract: include/nafp.h has it in full; the arithmetic, the bounds of every read and write and the layout of the int32 workspace
// are csrc/flac_decode.h, shared with the host.  A decoded frame is a pure function of (its bytes, its record).
//
// The bit stream of a frame is serial -- where a subframe, a partition or a Rice code starts is known only when everything before
// it has been read -- and frames are independent, so the parallelism is across frames.  Two kernels per launch:
//   flac_frames_kernel.  ONE LANE PER FRAME: record checks, header, then per channel the subframe header, the residuals and, value
//   by value as the residuals come out of the bit reader, the predictor recurrence; then the CRC-16 over the bytes it has read.  The
//   lane's 32 coefficients and the ring of its last 64 samples live in LDS, lanes interleaved ([j][lane]: no bank conflict, and no
//   dynamically indexed per-lane array that would spill to scratch); predictors up to order 12 run on statically indexed registers
//   instead; the CRC table (512 bytes) is built in LDS by the workgroup.  Values (wasted bits undone) go to the int32 workspace 32
//   at a time (a lane's next load waits for its stores: flac_decode.h), the status and the channel assignment to a per-frame word.  Lanes of a
//   wave are at different places of different frames, so a wave pays the union of its lanes' paths: a workgroup is one wave with
//   FL_FRAMES = 16 frames, which spreads a launch's few thousand frames over four times the SIMDs that full waves would.
//   flac_store_kernel.  One workgroup per frame at a time, one lane per output element (sample, channel), consecutive lanes writing
//   consecutive elements: channel decorrelation, justification, byte stores.  A failed frame's range is zeroed here.
// Prediction runs inside the serial stage, not as a stage of its own per (frame, channel): the recurrence is as serial as the bit
// reader and both advance one sample at a time, so a lane that reads a residual has the prediction's operands in LDS already.
#include "nafp_common.h"

#include "flac_decode.h"

namespace nafp {

constexpr int FL_THREADS = 64;                 // flac_frames_kernel: one wave
constexpr int FL_FRAMES = 16;                  // frames (active lanes) per workgroup
constexpr int FL_STORE_THREADS = 256;

__global__ __launch_bounds__(FL_THREADS) void flac_frames_kernel(const uint8_t* __restrict__ raw, int64_t raw_size,
                                                                 const nafp_flac_frame* __restrict__ frames, int64_t n_frames,
                                                                 int32_t* __restrict__ ws, int64_t scratch_size, int32_t* __restrict__ meta) {
    __shared__ int32_t s_coef[FL_MAX_ORDER * FL_FRAMES];
    __shared__ int32_t s_hist[FL_RING * FL_FRAMES];
    __shared__ uint16_t s_crc[256];
    const int tid = threadIdx.x;
    for (int i = tid; i < 256; i += FL_THREADS) s_crc[i] = (uint16_t)fl_crc16_entry((uint32_t)i);
    __syncthreads();
    const int64_t f = (int64_t)blockIdx.x * FL_FRAMES + tid;
    if (tid >= FL_FRAMES || f >= n_frames) return;
    const nafp_flac_frame rec = frames[f];
    int st = fl_record_fault(rec, raw_size, scratch_size), assign = 0;
    if (st == 0) st = fl_decode_frame(raw + rec.raw_off, rec, ws, s_coef + tid, s_hist + tid, FL_FRAMES, s_crc, &assign);
    meta[f] = st | (assign << 8);
}

__global__ __launch_bounds__(FL_STORE_THREADS) void flac_store_kernel(const nafp_flac_frame* __restrict__ frames, int64_t n_frames,
                                                                      const int32_t* __restrict__ ws, const int32_t* __restrict__ meta,
                                                                      uint8_t* __restrict__ scratch, int32_t* __restrict__ status) {
    const int tid = threadIdx.x;
    for (int64_t f = blockIdx.x; f < n_frames; f += gridDim.x) {
        const nafp_flac_frame rec = frames[f];
        const int st = meta[f] & 0xff, assign = meta[f] >> 8;
        if (status && tid == 0) status[f] = st;
        if (st == NAFP_FLAC_NO_RANGE) continue;
        const int n_el = rec.block_size * rec.channels;                    // <= 131072; the range is inside the arena (fl_record_fault)
        if (st != 0) {
            uint8_t* dst = scratch + rec.scratch_off;
            const int bytes = n_el * fl_container(rec.bps);
            for (int k = tid; k < bytes; k += FL_STORE_THREADS) dst[k] = 0;
            continue;
        }
        for (int e = tid; e < n_el; e += FL_STORE_THREADS) {
            const int i = e / rec.channels;
            fl_store_element(rec, assign, ws, scratch, i, e - i * rec.channels);
        }
    }
}

}  // namespace nafp

using namespace nafp;

extern "C" int nafp_flac_streaminfo_host(const void* bytes, int64_t n_bytes, nafp_flac_info* info) {
    if (!bytes || !info || n_bytes < 0) return NAFP_ERR_INVALID_ARG;
    return fl_streaminfo((const uint8_t*)bytes, n_bytes, info);
}

extern "C" int nafp_flac_index_host(const void* bytes, int64_t n_bytes, nafp_flac_info* info, nafp_flac_index_entry* frames_out, int64_t cap) {
    if (!bytes || !info || n_bytes < 0 || cap < 0 || (cap > 0 && !frames_out)) return NAFP_ERR_INVALID_ARG;
    return fl_index((const uint8_t*)bytes, n_bytes, info, frames_out, cap);
}

extern "C" int nafp_flac_decode_host(const void* raw, int64_t raw_size, const nafp_flac_frame* frames_host, int64_t n_frames, void* scratch,
                                     int64_t scratch_size, int32_t* status_out) {
    if (!raw || !scratch || raw_size < 0 || scratch_size < 0 || n_frames < 0 || (n_frames > 0 && !frames_host)) return NAFP_ERR_INVALID_ARG;
    std::vector<int32_t> ws((size_t)(scratch_size / 2 + 1));
    fl_decode_frames((const uint8_t*)raw, raw_size, frames_host, n_frames, (uint8_t*)scratch, scratch_size, status_out, ws.data());
    return NAFP_OK;
}

extern "C" int nafp_flac_check_frames_host(const nafp_flac_frame* frames_host, int64_t n_frames, int64_t raw_size, int64_t scratch_size) {
    if (n_frames < 0 || raw_size < 0 || scratch_size < 0 || (n_frames > 0 && !frames_host)) return NAFP_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n_frames; ++i)
        if (fl_record_fault(frames_host[i], raw_size, scratch_size) != 0) return NAFP_ERR_INVALID_ARG;
    return NAFP_OK;
}

extern "C" int nafp_flac_decode(const uint8_t* raw, int64_t raw_size, const nafp_flac_frame* frames_dev, int64_t n_frames, uint8_t* scratch,
                                int64_t scratch_size, int32_t* status_dev, void* stream) {
    if (!raw || !scratch || raw_size < 0 || scratch_size < 0 || n_frames < 0 || (n_frames > 0 && !frames_dev)) return NAFP_ERR_INVALID_ARG;
    if (n_frames == 0) return NAFP_OK;
    hipStream_t st = (hipStream_t)stream;
    // the workspace and the per-frame words live for this call only, in stream order; the pool keeps what it has been given, so
    // that a launch does not pay for a fresh allocation every time
    static thread_local int pool_ready_for = -1;
    int dev = 0;
    NAFP_HIP_CHECK(hipGetDevice(&dev));
    if (pool_ready_for != dev) {
        hipMemPool_t pool;
        NAFP_HIP_CHECK(hipDeviceGetDefaultMemPool(&pool, dev));
        uint64_t keep = UINT64_MAX;
        NAFP_HIP_CHECK(hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep));
        pool_ready_for = dev;
    }
    int32_t* ws = nullptr;
    int32_t* meta = nullptr;
    NAFP_HIP_CHECK(hipMallocAsync((void**)&ws, sizeof(int32_t) * (size_t)(scratch_size / 2 + 1), st));
    hipError_t e = hipMallocAsync((void**)&meta, sizeof(int32_t) * (size_t)n_frames, st);
    if (e == hipSuccess) {
        const int64_t groups = (n_frames + FL_FRAMES - 1) / FL_FRAMES;
        flac_frames_kernel<<<dim3((unsigned)groups), FL_THREADS, 0, st>>>(raw, raw_size, frames_dev, n_frames, ws, scratch_size, meta);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        const int64_t grid = n_frames < 8192 ? n_frames : 8192;
        flac_store_kernel<<<dim3((unsigned)grid), FL_STORE_THREADS, 0, st>>>(frames_dev, n_frames, ws, meta, scratch, status_dev);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(ws, st);
    if (meta) (void)hipFreeAsync(meta, st);
    NAFP_HIP_CHECK(e);
    return NAFP_OK;
}
