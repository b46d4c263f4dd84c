// Block codecs of RIFF/WAVE -- G.711 A-law / mu-law, IMA ADPCM and MS ADPCM at 4 bits -- and Apple's IMA4 packets of AIFF-C, decoded
// to interleaved int16 PCM, gfx950.  A pre-pass of the ingest (ingest.hip), which reads this kernel's output arena as NAFP_INGEST_S16.
//
// Contract (include/nafp.h has it in full; the arithmetic is csrc/codec_decode.h, shared with the host): int32 throughout, a
// decoded sample is a pure function of (its block's bytes, its place in the block).
//
// Two kernels, blockIdx.y = piece, the workgroups of a row striding over the piece's steps; every launch runs both (the pieces
// are known to the device only) and each leaves the other's pieces alone.
//   codec_g711_kernel.  G.711 is elementwise: a lane takes 8 bytes and writes 8 int16 as ONE 16-byte store; the vectors are laid
//   over the piece so that every store is 16-byte aligned whatever parity out_off has (the first and last vector of a piece are
//   partial and go sample by sample); the 8 bytes come as one 8-byte load, two 4-byte loads or eight 1-byte loads, never wider
//   than the source address is aligned.  No table: the expansion is shifts and adds.  This kernel also zeroes the stated range of
//   every inconsistent piece, of whatever codec.
//   codec_adpcm_kernel.  ADPCM is serial inside a block and parallel across blocks: ONE LANE PER (block, channel).  Lanes reading
//   global memory at a stride of block_align would waste every transaction, so a workgroup first stages a GROUP of consecutive
//   blocks -- one contiguous byte range -- into LDS with coalesced loads (16 bytes per lane where the range and block_align are
//   16-byte aligned, 4 where 4-byte aligned, single bytes otherwise), each block a row whose stride is an ODD number of dwords, so
//   that the lanes' reads at the same offset of consecutive blocks fall on different banks (a 256-byte block at its natural
//   stride would put all 64 lanes on one).  The lanes decode into a second LDS image, [block][frame][channel] int16 with an odd
//   dword row stride as well, and the whole workgroup then writes that image -- again one contiguous range of the output arena --
//   with coalesced 4-byte stores (2-byte ones for an odd first or last sample).
//   What a launch waits for is the RECURRENCE, not memory (DESIGN.md section 4.10.2 has the measurements): a lane needs 80 to
//   120 ns per nibble and a block of 4096 bytes is 8184 nibbles in a row, while the bytes of a whole generate launch move in a
//   few microseconds.  The time of a launch is therefore (rounds of resident workgroups) x (nibbles per block) x (time per
//   nibble), and the group size is chosen for the first factor: a workgroup owns 80 KB of LDS, half a compute unit's, and takes
//   as many blocks as that holds, both images counted, at most 256 lanes -- 64 blocks at block_align 256 mono, 16 at 1024
//   stereo, 4 at 4096 mono.  Measured against 64 KB (more rounds), 160 KB (one workgroup per compute unit: no fewer rounds for
//   the blocks of a launch, slower nibbles) and one-wave workgroups of 20 KB (8 decoding waves per compute unit share its SIMDs).
//   Apple IMA4 runs in the same kernel on a path of its own (cd_qt_piece): 34-byte packets of 64 nibbles, where staging and
//   stores set the time and not the recurrence.
#include "nafp_common.h"

#include "codec_decode.h"

namespace nafp {

constexpr int CD_THREADS = 256;
constexpr int CD_LDS_BYTES = 80 * 1024;                // half the LDS of a gfx950 compute unit: two workgroups on each
constexpr int CD_G711_STEP = CD_THREADS * 8;          // samples per workgroup step
constexpr int CD_QT_LANES = 256;                      // Apple IMA4: (block, channel) lanes per group, chosen by measurement
constexpr int CD_QT_IN_BYTES = CD_QT_LANES * CD_QT_PACKET + 16;      // a group's packets and the skew of their first byte; 16 | it
static_assert(CD_QT_LANES <= CD_THREADS && CD_QT_IN_BYTES % 16 == 0 && CD_QT_IN_BYTES + CD_QT_LANES * (CD_QT_SPB * 2 + 4) <= CD_LDS_BYTES,
              "Apple IMA4 group in LDS");

struct CdGroup { int in_dw, out_dw, blocks; };

// LDS rows of one ADPCM block (dwords, odd) and the blocks per group; the geometry is taken as checked
__host__ __device__ inline CdGroup cd_group(int channels, int block_align, int spb) {
    CdGroup g;
    g.in_dw = ((block_align + 3) / 4) | 1;
    g.out_dw = ((spb * channels * 2 + 3) / 4) | 1;
    const int fit = CD_LDS_BYTES / ((g.in_dw + g.out_dw) * 4);               // >= 8: at most 20,472 bytes per block
    const int lanes = CD_THREADS / channels;
    g.blocks = fit < lanes ? fit : lanes;
    return g;
}

struct CdLdsReader {
    const uint32_t* row;
    __device__ __forceinline__ uint32_t u8(int i) const { return ((const uint8_t*)row)[i]; }
    __device__ __forceinline__ uint32_t u32(int i) const { return row[i >> 2]; }
};
struct CdLdsWriter {
    int16_t* row;
    int channels;
    __device__ __forceinline__ void operator()(int frame, int c, int32_t x) const { row[frame * channels + c] = (int16_t)x; }
};

// the group's bytes [0, n_bytes) at src -> rows of in_dw dwords; U bytes per lane and load, src and block_align multiples of U
template <int U>
__device__ __forceinline__ void cd_stage(const uint8_t* __restrict__ src, int n_bytes, int block_align, int in_dw, uint32_t* s_in, int tid) {
    const int per_row = block_align / U;
    for (int i = tid; i < n_bytes / U; i += CD_THREADS) {
        const int r = i / per_row, k = i - r * per_row;
        if (U == 16) {
            const uint4 v = *(const uint4*)(src + (int64_t)i * 16);
            uint32_t* d = s_in + r * in_dw + k * 4;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        } else if (U == 4) {
            s_in[r * in_dw + k] = *(const uint32_t*)(src + (int64_t)i * 4);
        } else {
            ((uint8_t*)s_in)[r * in_dw * 4 + k] = src[i];
        }
    }
}

__device__ __forceinline__ void cd_g711_piece(const nafp_codec_piece& pc, const uint8_t* __restrict__ raw, int16_t* __restrict__ out, int tid) {
    const int64_t n = pc.n_blocks * pc.channels;                       // samples; inside both arenas (cd_piece_fault)
    const uint8_t* src = raw + pc.raw_off;
    int16_t* dst = out + pc.out_off;
    const int codec = pc.codec;
    const int pre = (int)(((uintptr_t)dst & 15) >> 1);                 // vector v holds samples [8 v - pre, 8 v - pre + 8): 16-byte aligned
    const int64_t n_vec = (n + pre + 7) / 8;
    for (int64_t v = (int64_t)blockIdx.x * CD_THREADS + tid; v < n_vec; v += (int64_t)gridDim.x * CD_THREADS) {
        const int64_t e0 = v * 8 - pre;
        if (e0 >= 0 && e0 + 8 <= n) {
            const uint8_t* p = src + e0;
            uint32_t lo, hi;
            if (((uintptr_t)p & 7) == 0) {
                const uint2 w = *(const uint2*)p;
                lo = w.x; hi = w.y;
            } else if (((uintptr_t)p & 3) == 0) {
                lo = ((const uint32_t*)p)[0]; hi = ((const uint32_t*)p)[1];
            } else {
                lo = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
                hi = (uint32_t)p[4] | ((uint32_t)p[5] << 8) | ((uint32_t)p[6] << 16) | ((uint32_t)p[7] << 24);
            }
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t word = k < 2 ? lo : hi;
                const int32_t a = cd_g711(codec, (word >> (16 * (k & 1))) & 0xffu);
                const int32_t b = cd_g711(codec, (word >> (16 * (k & 1) + 8)) & 0xffu);
                w[k] = ((uint32_t)a & 0xffffu) | ((uint32_t)b << 16);
            }
            *(uint4*)(dst + e0) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (int k = 0; k < 8; ++k) {
                const int64_t e = e0 + k;
                if (e >= 0 && e < n) dst[e] = (int16_t)cd_g711(codec, src[e]);
            }
        }
    }
}

// the group's output image, nb rows of row_len int16 at a stride of out_dw dwords -> n_el consecutive int16 of the arena at dst,
// inside it (cd_piece_fault): coalesced 4-byte stores, 2-byte ones for an odd first or last sample
__device__ __forceinline__ void cd_store_image(int16_t* __restrict__ dst, const uint16_t* so, int nb, int row_len, int out_dw, int tid) {
    const int n_el = nb * row_len;
    const int head = (int)(((uintptr_t)dst >> 1) & 1);
    const int n_pair = (n_el - head) / 2;
    for (int k = tid; k < n_pair; k += CD_THREADS) {
        const int e = head + 2 * k;
        int r = e / row_len, c0 = e - r * row_len;
        const uint32_t lo = so[r * out_dw * 2 + c0];
        if (++c0 == row_len) { c0 = 0; ++r; }
        const uint32_t hi = so[r * out_dw * 2 + c0];
        *(uint32_t*)(dst + e) = lo | (hi << 16);
    }
    if (tid == 0 && head) dst[0] = (int16_t)so[0];
    if (tid == 1 && ((n_el - head) & 1)) dst[n_el - 1] = (int16_t)so[(nb - 1) * out_dw * 2 + row_len - 1];
}

__device__ __forceinline__ void cd_adpcm_piece(const nafp_codec_piece& pc, const uint8_t* __restrict__ raw, int16_t* __restrict__ out,
                                               uint32_t* s_lds, int tid) {
    const int C = pc.channels, align = pc.block_align, spb = pc.spb, codec = pc.codec;
    const CdGroup g = cd_group(C, align, spb);
    const int row_len = spb * C;                                       // int16 per block
    uint32_t* s_in = s_lds;
    uint32_t* s_out = s_lds + g.blocks * g.in_dw;
    const uint8_t* base = raw + pc.raw_off;
    const int unit = ((uintptr_t)base % 16 == 0 && align % 16 == 0) ? 16 : (((uintptr_t)base % 4 == 0 && align % 4 == 0) ? 4 : 1);
    for (int64_t b0 = (int64_t)blockIdx.x * g.blocks; b0 < pc.n_blocks; b0 += (int64_t)gridDim.x * g.blocks) {
        const int nb = (int)(pc.n_blocks - b0 < g.blocks ? pc.n_blocks - b0 : g.blocks);
        const uint8_t* src = base + b0 * align;                        // [0, nb * align) inside the raw arena (cd_piece_fault)
        if (unit == 16) cd_stage<16>(src, nb * align, align, g.in_dw, s_in, tid);
        else if (unit == 4) cd_stage<4>(src, nb * align, align, g.in_dw, s_in, tid);
        else cd_stage<1>(src, nb * align, align, g.in_dw, s_in, tid);
        __syncthreads();
        if (tid < nb * C) {
            const int blk = tid / C, c = tid - blk * C;
            const CdLdsReader rd{s_in + blk * g.in_dw};
            const CdLdsWriter wr{(int16_t*)(s_out + blk * g.out_dw), C};
            if (codec == NAFP_CODEC_IMA4) cd_ima_channel(C, align, c, rd, wr);
            else cd_ms_channel(C, align, c, rd, wr);
        }
        __syncthreads();
        cd_store_image(out + pc.out_off + b0 * row_len, (const uint16_t*)s_out, nb, row_len, g.out_dw, tid);
        // the next round's staging writes s_in only, last read before the barrier above; s_out is next written after a barrier
    }
}

// n_bytes at src (any alignment) -> s_bytes + (src & 15), so that every 16-byte unit of global memory is a 16-byte unit of
// LDS: 16-byte loads over the aligned middle of the range, single bytes for the up to 15 before and after it.  Nothing outside
// [src, src + n_bytes) is read.  Returns the skew (src & 15); s_bytes is 16-byte aligned and holds n_bytes + 15.
__device__ __forceinline__ int cd_stage_linear(const uint8_t* __restrict__ src, int n_bytes, uint8_t* s_bytes, int tid) {
    const int skew = (int)((uintptr_t)src & 15);
    int head = skew ? 16 - skew : 0;
    if (head > n_bytes) head = n_bytes;
    const int n_vec = (n_bytes - head) / 16;
    for (int i = tid; i < n_vec; i += CD_THREADS) *(uint4*)(s_bytes + skew + head + 16 * i) = *(const uint4*)(src + head + 16 * i);
    const int tail = head + 16 * n_vec;                                // < 31 single bytes in all
    if (tid < head) s_bytes[skew + tid] = src[tid];
    else if (tid >= 32 && tid - 32 < n_bytes - tail) s_bytes[skew + tail + tid - 32] = src[tail + tid - 32];
    return skew;
}

struct CdLdsByteReader {
    const uint8_t* p;
    __device__ __forceinline__ uint32_t u8(int i) const { return p[i]; }
};

// Apple IMA4: a block is 34 C bytes -- 2-byte aligned at best, so the row staging above would go byte by byte -- and only 64
// nibbles per lane, so what a group costs is its staging and its stores, not the recurrence.  The group's byte range is staged as
// it stands (cd_stage_linear: 16-byte loads whatever the block stride), the lanes read their packets at a stride of 34 bytes (8.5
// dwords: the 64 lanes of a wave fall on different banks but for pairs that share a dword) and the output image and its stores are
// the ones above.  CD_QT_LANES lanes per group: 256 / C blocks, 8.7 KB in and 33.8 KB out.
__device__ __forceinline__ void cd_qt_piece(const nafp_codec_piece& pc, const uint8_t* __restrict__ raw, int16_t* __restrict__ out,
                                            uint32_t* s_lds, int tid) {
    const int C = pc.channels, align = CD_QT_PACKET * C, row_len = CD_QT_SPB * C;      // as cd_piece_fault found them
    const int blocks = CD_QT_LANES / C, out_dw = (row_len / 2) | 1;
    uint8_t* s_in = (uint8_t*)s_lds;
    uint32_t* s_out = s_lds + CD_QT_IN_BYTES / 4;
    const uint8_t* base = raw + pc.raw_off;
    for (int64_t b0 = (int64_t)blockIdx.x * blocks; b0 < pc.n_blocks; b0 += (int64_t)gridDim.x * blocks) {
        const int nb = (int)(pc.n_blocks - b0 < blocks ? pc.n_blocks - b0 : blocks);
        // [0, nb * align) at src is inside the raw arena (cd_piece_fault); nb * align <= CD_QT_LANES * 34
        const int skew = cd_stage_linear(base + b0 * align, nb * align, s_in, tid);
        __syncthreads();
        if (tid < nb * C) {
            const int blk = tid / C, c = tid - blk * C;
            const CdLdsByteReader rd{s_in + skew + blk * align};
            const CdLdsWriter wr{(int16_t*)(s_out + blk * out_dw), C};
            cd_qt_channel(c, rd, wr);
        }
        __syncthreads();
        cd_store_image(out + pc.out_off + b0 * row_len, (const uint16_t*)s_out, nb, row_len, out_dw, tid);
        // the next round's staging writes s_in only, last read before the barrier above; s_out is next written after a barrier
    }
}

__global__ __launch_bounds__(CD_THREADS) void codec_g711_kernel(const uint8_t* __restrict__ raw, int64_t raw_size,
                                                                const nafp_codec_piece* __restrict__ pieces,
                                                                int16_t* __restrict__ out, int64_t out_samples) {
    const nafp_codec_piece pc = pieces[blockIdx.y];
    const int tid = threadIdx.x;
    const int fault = cd_piece_fault(pc, raw_size, out_samples);
    if (fault == 1) return;
    if (fault != 0) {                                                  // the range the piece states is inside the arena: zero it
        const int64_t n = pc.n_blocks * pc.spb * pc.channels;
        int16_t* dst = out + pc.out_off;
        for (int64_t i = (int64_t)blockIdx.x * CD_THREADS + tid; i < n; i += (int64_t)gridDim.x * CD_THREADS) dst[i] = 0;
        return;
    }
    if (pc.codec == NAFP_CODEC_ALAW || pc.codec == NAFP_CODEC_ULAW) cd_g711_piece(pc, raw, out, tid);
}

__global__ __launch_bounds__(CD_THREADS) void codec_adpcm_kernel(const uint8_t* __restrict__ raw, int64_t raw_size,
                                                                 const nafp_codec_piece* __restrict__ pieces,
                                                                 int16_t* __restrict__ out, int64_t out_samples) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_lds[];
    const nafp_codec_piece pc = pieces[blockIdx.y];
    if (cd_piece_fault(pc, raw_size, out_samples) != 0) return;        // codec_g711_kernel deals with it
    if (pc.codec == NAFP_CODEC_IMA4 || pc.codec == NAFP_CODEC_MS4) cd_adpcm_piece(pc, raw, out, s_lds, threadIdx.x);
    else if (pc.codec == NAFP_CODEC_QT_IMA4) cd_qt_piece(pc, raw, out, s_lds, threadIdx.x);
}

}  // namespace nafp

using namespace nafp;

extern "C" int nafp_codec_samples_per_block(int codec, int channels, int block_align) {
    return cd_samples_per_block(codec, channels, block_align);
}

extern "C" int nafp_codec_blocks_per_group(int codec, int channels, int block_align) {
    const int spb = cd_samples_per_block(codec, channels, block_align);
    if (spb < 0) return -1;
    if (codec == NAFP_CODEC_ALAW || codec == NAFP_CODEC_ULAW) return CD_G711_STEP / channels;
    if (codec == NAFP_CODEC_QT_IMA4) return CD_QT_LANES / channels;
    return cd_group(channels, block_align, spb).blocks;
}

extern "C" int nafp_codec_decode_host(int codec, int channels, int block_align, const void* bytes, int64_t n_blocks, int16_t* out) {
    const int spb = cd_samples_per_block(codec, channels, block_align);
    if (spb < 0) return NAFP_ERR_UNSUPPORTED;
    if (n_blocks < 0 || (n_blocks > 0 && (!bytes || !out))) return NAFP_ERR_INVALID_ARG;
    cd_decode_blocks(codec, channels, block_align, spb, (const uint8_t*)bytes, n_blocks, out);
    return NAFP_OK;
}

extern "C" int nafp_codec_check_pieces_host(const nafp_codec_piece* pieces_host, int64_t n_pieces, int64_t raw_size, int64_t out_samples) {
    if (n_pieces < 0 || raw_size < 0 || out_samples < 0 || (n_pieces > 0 && !pieces_host)) return NAFP_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n_pieces; ++i) {
        const nafp_codec_piece& pc = pieces_host[i];
        if (cd_samples_per_block(pc.codec, pc.channels, pc.block_align) < 0) return NAFP_ERR_UNSUPPORTED;
        if (cd_piece_fault(pc, raw_size, out_samples) != 0) return NAFP_ERR_INVALID_ARG;
    }
    return NAFP_OK;
}

extern "C" int nafp_codec_decode_i16(const uint8_t* raw_bytes, int64_t raw_size, const nafp_codec_piece* pieces_dev, int64_t n_pieces,
                                     int16_t* out, int64_t out_samples, void* stream) {
    if (!raw_bytes || !out || n_pieces < 0 || raw_size < 0 || out_samples < 0 || (n_pieces > 0 && !pieces_dev)) return NAFP_ERR_INVALID_ARG;
    if (n_pieces == 0 || out_samples == 0) return NAFP_OK;
    // blockIdx.y = piece; a row is sized for twice the mean piece, in steps of 2048 samples for the elementwise kernel and of
    // 32768 (an ADPCM group decodes up to some 65,000) for the other; the bytes written do not depend on it
    NAFP_HIP_CHECK(hipFuncSetAttribute((const void*)codec_adpcm_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, CD_LDS_BYTES));
    const int64_t steps = (out_samples + CD_G711_STEP - 1) / CD_G711_STEP, groups = (out_samples + 32767) / 32768;
    for (int64_t p0 = 0; p0 < n_pieces; p0 += 32768) {
        const int64_t np = n_pieces - p0 < 32768 ? n_pieces - p0 : 32768;
        int64_t gx = 2 * ((steps + n_pieces - 1) / n_pieces), ga = 2 * ((groups + n_pieces - 1) / n_pieces);
        gx = gx < 1 ? 1 : (gx > 4096 ? 4096 : gx);
        ga = ga < 1 ? 1 : (ga > 4096 ? 4096 : ga);
        codec_g711_kernel<<<dim3((unsigned)gx, (unsigned)np), CD_THREADS, 0, (hipStream_t)stream>>>(raw_bytes, raw_size, pieces_dev + p0, out,
                                                                                                   out_samples);
        NAFP_LAUNCH_CHECK();
        codec_adpcm_kernel<<<dim3((unsigned)ga, (unsigned)np), CD_THREADS, CD_LDS_BYTES, (hipStream_t)stream>>>(raw_bytes, raw_size,
                                                                                                              pieces_dev + p0, out, out_samples);
        NAFP_LAUNCH_CHECK();
    }
    return NAFP_OK;
}
