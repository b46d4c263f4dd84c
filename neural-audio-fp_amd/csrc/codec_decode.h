// Per-sample and per-block arithmetic of the block codecs (include/nafp.h `nafp_codec_*`, DESIGN.md sections 4.10.2 and 4.10.5):
// G.711 A-law and mu-law, IMA ADPCM and MS ADPCM at 4 bits, Apple IMA4 packets.  Plain C++ in int32, no table for G.711, no 16-bit
// arithmetic.  ONE definition for the kernel (csrc/codec.hip), the host entry point nafp_codec_decode_host and any stand-alone
// host program: every function is NAFP_CODEC_HD, which is `__host__ __device__` under hipcc and nothing elsewhere.  A block is
// read through `rd` (u8(i): byte i of the block; u32(i): the little-endian dword at byte i, i a multiple of 4) and written through
// `wr(frame, channel, x)`, so the kernel can keep both in LDS and the host in plain arrays.
#ifndef NAFP_CODEC_DECODE_H
#define NAFP_CODEC_DECODE_H

#include <stdint.h>

#include "../../include/nafp.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NAFP_CODEC_HD __host__ __device__ inline
#else
#define NAFP_CODEC_HD inline
#endif

namespace nafp {

constexpr int CD_MAX_ALIGN = 4096;
constexpr int CD_MAX_G711_CHANNELS = 8;
constexpr int CD_MAX_SPB = 8185;                       // IMA mono at block_align 4096: 8 * 1023 + 1
constexpr int CD_QT_PACKET = 34;                       // Apple IMA4: a 2-byte header and 32 bytes of nibbles per channel
constexpr int CD_QT_SPB = 64;

NAFP_CODEC_HD int32_t cd_clamp16(int32_t x) { return x < -32768 ? -32768 : (x > 32767 ? 32767 : x); }

// frames per block; -1 for anything outside the contract
NAFP_CODEC_HD int cd_samples_per_block(int codec, int channels, int block_align) {
    if (block_align < 1 || block_align > CD_MAX_ALIGN || channels < 1) return -1;
    switch (codec) {
        case NAFP_CODEC_ALAW:
        case NAFP_CODEC_ULAW:
            return channels <= CD_MAX_G711_CHANNELS && block_align == channels ? 1 : -1;
        case NAFP_CODEC_IMA4: {
            if (channels > 2) return -1;
            const int body = block_align - 4 * channels;
            if (body < 4 * channels || body % (4 * channels) != 0) return -1;
            return 8 * (body / (4 * channels)) + 1;
        }
        case NAFP_CODEC_MS4: {
            if (channels > 2 || block_align <= 7 * channels) return -1;
            return 2 + 2 * (block_align - 7 * channels) / channels;      // 2 (align - 7 C) is a multiple of C for C = 1, 2
        }
        case NAFP_CODEC_QT_IMA4:
            return channels <= 2 && block_align == CD_QT_PACKET * channels ? CD_QT_SPB : -1;
    }
    return -1;
}

NAFP_CODEC_HD int32_t cd_ulaw(uint32_t byte) {
    const int32_t u = (int32_t)(~byte & 0xffu);
    const int32_t t = (((u & 15) << 3) + 0x84) << ((u & 0x70) >> 4);
    return (u & 0x80) ? 0x84 - t : t - 0x84;
}

NAFP_CODEC_HD int32_t cd_alaw(uint32_t byte) {
    const int32_t a = (int32_t)((byte ^ 0x55u) & 0xffu);
    int32_t t = (a & 15) << 4;
    const int32_t seg = (a & 0x70) >> 4;
    if (seg == 0) t += 8;
    else if (seg == 1) t += 0x108;
    else t = (t + 0x108) << (seg - 1);
    return (a & 0x80) ? t : -t;
}

NAFP_CODEC_HD int32_t cd_g711(int codec, uint32_t byte) { return codec == NAFP_CODEC_ALAW ? cd_alaw(byte) : cd_ulaw(byte); }

NAFP_CODEC_HD int32_t cd_ima_step(int idx) {
    static constexpr int16_t STEP[89] = {
        7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
        157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411,
        1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493,
        10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};
    return STEP[idx];
}

// one IMA nibble: pred and idx advance
NAFP_CODEC_HD void cd_ima_nibble(int32_t n, int32_t& pred, int32_t& idx) {
    const int32_t s = cd_ima_step(idx);
    int32_t d = s >> 3;
    if (n & 1) d += s >> 2;
    if (n & 2) d += s >> 1;
    if (n & 4) d += s;
    pred = cd_clamp16((n & 8) ? pred - d : pred + d);
    // IDX = {-1, -1, -1, -1, 2, 4, 6, 8} for n & 7
    const int32_t m = n & 7;
    idx += m < 4 ? -1 : 2 * (m - 3);
    idx = idx < 0 ? 0 : (idx > 88 ? 88 : idx);
}

// channel c of one IMA block
template <class Rd, class Wr>
NAFP_CODEC_HD void cd_ima_channel(int channels, int block_align, int c, const Rd& rd, const Wr& wr) {
    const uint32_t h = rd.u32(4 * c);
    int32_t pred = (int32_t)(int16_t)(uint16_t)(h & 0xffffu);
    int32_t idx = (int32_t)((h >> 16) & 0xffu);
    if (idx > 88) idx = 88;
    wr(0, c, pred);
    const int groups = (block_align - 4 * channels) / (4 * channels);
    for (int g = 0; g < groups; ++g) {
        uint32_t w = rd.u32(4 * channels * (g + 1) + 4 * c);
        for (int j = 0; j < 8; ++j, w >>= 4) {
            cd_ima_nibble((int32_t)(w & 15u), pred, idx);
            wr(1 + 8 * g + j, c, pred);
        }
    }
}

struct CdMsState { int32_t c1, c2, delta, samp1, samp2; };

NAFP_CODEC_HD int32_t cd_ms_adapt(int32_t n) {
    // a table in memory on purpose: its address depends on the nibble alone, so the load runs ahead of the delta recurrence,
    // while the same values from compares and selects put ten more instructions between every two nibbles (measured: + 9 %)
    static constexpr int16_t ADAPT[16] = {230, 230, 230, 230, 307, 409, 512, 614, 768, 614, 512, 409, 307, 230, 230, 230};
    return ADAPT[n];
}

// one MS nibble -> the sample
NAFP_CODEC_HD int32_t cd_ms_nibble(int32_t n, CdMsState& st) {
    const int32_t s = n >= 8 ? n - 16 : n;
    const int32_t pred = (st.samp1 * st.c1 + st.samp2 * st.c2) / 256;           // truncates toward zero
    const int32_t x = cd_clamp16(pred + s * st.delta);
    st.samp2 = st.samp1;
    st.samp1 = x;
    int32_t d = (cd_ms_adapt(n) * st.delta) >> 8;                              // arithmetic shift
    st.delta = d < 16 ? 16 : (d > 2796202 ? 2796202 : d);
    return x;
}

// channel c of one MS block
template <class Rd, class Wr>
NAFP_CODEC_HD void cd_ms_channel(int channels, int block_align, int c, const Rd& rd, const Wr& wr) {
    static constexpr int16_t C1[7] = {256, 512, 0, 192, 240, 460, 392};
    static constexpr int16_t C2[7] = {0, -256, 0, 64, 0, -208, -232};
    int32_t p = (int32_t)rd.u8(c);
    if (p > 6) p = 6;
    const int C = channels;
    CdMsState st;
    st.c1 = C1[p];
    st.c2 = C2[p];
    st.delta = (int32_t)(int16_t)(uint16_t)(rd.u8(C + 2 * c) | (rd.u8(C + 2 * c + 1) << 8));
    st.samp1 = (int32_t)(int16_t)(uint16_t)(rd.u8(3 * C + 2 * c) | (rd.u8(3 * C + 2 * c + 1) << 8));
    st.samp2 = (int32_t)(int16_t)(uint16_t)(rd.u8(5 * C + 2 * c) | (rd.u8(5 * C + 2 * c + 1) << 8));
    wr(0, c, st.samp2);
    wr(1, c, st.samp1);
    if (C == 1) {
        for (int i = 7, f = 2; i < block_align; ++i, f += 2) {
            const uint32_t b = rd.u8(i);
            wr(f, 0, cd_ms_nibble((int32_t)(b >> 4), st));
            wr(f + 1, 0, cd_ms_nibble((int32_t)(b & 15u), st));
        }
    } else {
        for (int i = 14, f = 2; i < block_align; ++i, ++f) {
            const uint32_t b = rd.u8(i);
            wr(f, c, cd_ms_nibble((int32_t)(c == 0 ? b >> 4 : b & 15u), st));
        }
    }
}

// channel c of one Apple IMA4 block: its packet at byte 34 c.  The header is big-endian and keeps the predictor's upper 9 bits;
// the predictor AFTER each nibble is a frame, the header's own value is none.  Nothing comes from the packet before.
template <class Rd, class Wr>
NAFP_CODEC_HD void cd_qt_channel(int c, const Rd& rd, const Wr& wr) {
    const int at = CD_QT_PACKET * c;
    const uint32_t h = (rd.u8(at) << 8) | rd.u8(at + 1);
    int32_t pred = (int32_t)(int16_t)(uint16_t)(h & 0xff80u);
    int32_t idx = (int32_t)(h & 0x7fu);
    if (idx > 88) idx = 88;
    for (int i = 0; i < 32; ++i) {
        const uint32_t b = rd.u8(at + 2 + i);
        cd_ima_nibble((int32_t)(b & 15u), pred, idx);
        wr(2 * i, c, pred);
        cd_ima_nibble((int32_t)(b >> 4), pred, idx);
        wr(2 * i + 1, c, pred);
    }
}

// channel c of one block of any of the codecs (the geometry is taken as checked: cd_samples_per_block > 0)
template <class Rd, class Wr>
NAFP_CODEC_HD void cd_block_channel(int codec, int channels, int block_align, int c, const Rd& rd, const Wr& wr) {
    if (codec == NAFP_CODEC_IMA4) cd_ima_channel(channels, block_align, c, rd, wr);
    else if (codec == NAFP_CODEC_MS4) cd_ms_channel(channels, block_align, c, rd, wr);
    else if (codec == NAFP_CODEC_QT_IMA4) cd_qt_channel(c, rd, wr);
    else wr(0, c, cd_g711(codec, rd.u8(c)));
}

// plain-array reader / writer (host; the kernel has LDS ones)
struct CdArrayReader {
    const uint8_t* p;
    NAFP_CODEC_HD uint32_t u8(int i) const { return p[i]; }
    NAFP_CODEC_HD uint32_t u32(int i) const {
        return (uint32_t)p[i] | ((uint32_t)p[i + 1] << 8) | ((uint32_t)p[i + 2] << 16) | ((uint32_t)p[i + 3] << 24);
    }
};
struct CdArrayWriter {
    int16_t* o;
    int channels;
    NAFP_CODEC_HD void operator()(int frame, int c, int32_t x) const { o[frame * channels + c] = (int16_t)x; }
};

// n_blocks whole blocks -> n_blocks * spb * channels interleaved int16
NAFP_CODEC_HD void cd_decode_blocks(int codec, int channels, int block_align, int spb, const uint8_t* bytes, int64_t n_blocks,
                                    int16_t* out) {
    for (int64_t b = 0; b < n_blocks; ++b) {
        const CdArrayReader rd{bytes + b * block_align};
        const CdArrayWriter wr{out + b * (int64_t)spb * channels, channels};
        for (int c = 0; c < channels; ++c) cd_block_channel(codec, channels, block_align, c, rd, wr);
    }
}

// the per-piece checks of the kernel.  0: consistent; 1: the output range the piece states (n_blocks * spb * channels int16 at
// out_off) is not a range of the arena, so nothing may be written; 2: anything else -- that range is zeroed.
NAFP_CODEC_HD int cd_piece_fault(const nafp_codec_piece& pc, int64_t raw_size, int64_t out_samples) {
    if (pc.n_blocks < 0 || pc.n_blocks > ((int64_t)1 << 40) || pc.spb < 1 || pc.spb > CD_MAX_SPB || pc.channels < 1 ||
        pc.channels > CD_MAX_G711_CHANNELS)
        return 1;
    const int64_t n = pc.n_blocks * pc.spb * pc.channels;                          // < 2^57
    if (pc.out_off < 0 || pc.out_off > out_samples || n > out_samples - pc.out_off) return 1;
    if (cd_samples_per_block(pc.codec, pc.channels, pc.block_align) != pc.spb) return 2;
    if (pc.raw_off < 0 || pc.raw_off > raw_size || pc.n_blocks > (raw_size - pc.raw_off) / pc.block_align) return 2;
    return 0;
}

}  // namespace nafp

#endif
