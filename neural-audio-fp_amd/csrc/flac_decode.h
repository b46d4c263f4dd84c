// FLAC: bit reader, frame-header parse, subframe decode, CRC-16 and output packing (include/nafp.h `nafp_flac_*`, DESIGN.md section
// 4.10.3).  Plain C++ in 32- / 64-bit integers.  ONE definition for the kernels (csrc/flac.hip), the host entry points
// nafp_flac_decode_host / nafp_flac_index_host and any stand-alone host program (tools/flac_host_check.cpp): every function of the
// decode is NAFP_FLAC_HD, which is `__host__ __device__` under hipcc and nothing elsewhere.
//
// A frame is decoded in two steps that meet in an int32 WORKSPACE `ws`:
//   fl_decode_frame   one caller per frame, serial: header, subframes, residuals AND the predictor recurrence, then the CRC-16.  The
//                     value of channel c, sample i (wasted bits already undone) goes to ws[fl_ws_index(rec, bw, c * block + i)].
//   fl_store_element  one caller per (sample, channel): channel decorrelation, MSB-justification, the little-endian store.
// The workspace needs no size of its own: element k of a frame is kept at HALF THE BYTE OFFSET of output element k of that frame,
// (scratch_off + k * bw) >> 1 with bw = 2 or 3 bytes per output sample.  Output elements are at least 2 bytes apart, so distinct
// elements of frames whose output ranges do not overlap never share a slot, and a frame whose output range lies in the scratch
// arena stays inside a workspace of scratch_size / 2 + 1 int32.
//
// CORRUPT INPUT.  No byte of a frame can take the decoder out of its arithmetic or its arenas: FlBits never loads past the frame's
// stated length (bits past it read as zero and raise `over`), every unary run is bounded by the value it may produce and by the
// frame's end, every count that sizes a loop or a shift comes from a checked field, and every store index is k < channels * block of
// a record whose range fl_record_fault has placed inside the arena.  Signed overflow cannot occur: a prediction is an int64 sum of
// at most 32 products of a coefficient of at most 15 bits with an int32 sample (< 2^51), everything else wraps in uint32.
#ifndef NAFP_FLAC_DECODE_H
#define NAFP_FLAC_DECODE_H

#include <stdint.h>

#include <vector>

#include "../../include/nafp.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NAFP_FLAC_HD __host__ __device__ inline
#else
#define NAFP_FLAC_HD inline
#endif

namespace nafp {

constexpr int FL_MAX_BLOCK = 16384;
constexpr int FL_MAX_CHANNELS = 8;
constexpr int FL_MAX_ORDER = 32;
constexpr int FL_MAX_RATE = 655350;

// ---- CRCs ------------------------------------------------------------------------------------------------------------------------
// CRC-16, polynomial 0x8005, initial 0, MSB first, unreflected: entry i of the byte table
NAFP_FLAC_HD uint32_t fl_crc16_entry(uint32_t i) {
    uint32_t c = i << 8;
    for (int k = 0; k < 8; ++k) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xffffu : (c << 1) & 0xffffu;
    return c;
}
NAFP_FLAC_HD uint32_t fl_crc16(const uint8_t* p, int64_t n, const uint16_t* tab) {
    uint32_t c = 0;
    for (int64_t i = 0; i < n; ++i) c = ((c << 8) & 0xffffu) ^ tab[(c >> 8) ^ p[i]];
    return c;
}
// CRC-8, polynomial 0x07, initial 0 (headers only: at most 16 bytes, no table)
NAFP_FLAC_HD uint32_t fl_crc8(const uint8_t* p, int n) {
    uint32_t c = 0;
    for (int i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xffu : (c << 1) & 0xffu;
    }
    return c;
}

// ---- frame header ----------------------------------------------------------------------------------------------------------------
struct FlHeader {
    int blocking;        // 0: `number` counts frames, 1: samples
    int block_size;      // 1 .. 65536 as coded
    int rate;            // 0: as STREAMINFO
    int assign;          // 0 .. 10
    int channels;
    int bps;             // 0: as STREAMINFO
    int64_t number;
};

// The header at p[0, n): its length in bytes (5 .. 16), or 0 when it is none: sync, reserved bits and codes, the coded number, CRC-8.
NAFP_FLAC_HD int fl_parse_header(const uint8_t* p, int64_t n, FlHeader& h) {
    if (n < 6 || p[0] != 0xffu || (p[1] & 0xfeu) != 0xf8u) return 0;
    h.blocking = p[1] & 1;
    const int bs_code = p[2] >> 4, rate_code = p[2] & 15;
    const int assign = p[3] >> 4, size_code = (p[3] >> 1) & 7;
    if (bs_code == 0 || rate_code == 15 || assign > 10 || size_code == 3 || size_code == 7 || (p[3] & 1)) return 0;
    h.assign = assign;
    h.channels = assign < 8 ? assign + 1 : 2;
    h.bps = size_code == 0 ? 0 : (size_code == 1 ? 8 : (size_code == 2 ? 12 : (size_code == 4 ? 16 : (size_code == 5 ? 20 : 24))));
    int pos = 4;
    // the coded number: UTF-8 scheme extended to 36 bits
    const uint32_t b0 = p[pos++];
    int extra;
    uint64_t v;
    if (b0 < 0x80u) { extra = 0; v = b0; }
    else if (b0 < 0xc0u) return 0;
    else if (b0 < 0xe0u) { extra = 1; v = b0 & 0x1fu; }
    else if (b0 < 0xf0u) { extra = 2; v = b0 & 0x0fu; }
    else if (b0 < 0xf8u) { extra = 3; v = b0 & 0x07u; }
    else if (b0 < 0xfcu) { extra = 4; v = b0 & 0x03u; }
    else if (b0 < 0xfeu) { extra = 5; v = b0 & 0x01u; }
    else if (b0 == 0xfeu) { extra = 6; v = 0; }
    else return 0;
    if (extra == 6 && !h.blocking) return 0;                 // a frame number has at most 31 bits
    if (pos + extra + 1 > n) return 0;
    for (int k = 0; k < extra; ++k) {
        const uint32_t b = p[pos++];
        if ((b & 0xc0u) != 0x80u) return 0;
        v = (v << 6) | (b & 0x3fu);
    }
    h.number = (int64_t)v;
    if (bs_code == 1) h.block_size = 192;
    else if (bs_code <= 5) h.block_size = 576 << (bs_code - 2);
    else if (bs_code == 6) { if (pos + 1 >= n) return 0; h.block_size = (int)p[pos] + 1; pos += 1; }
    else if (bs_code == 7) { if (pos + 2 >= n) return 0; h.block_size = (((int)p[pos] << 8) | (int)p[pos + 1]) + 1; pos += 2; }
    else h.block_size = 256 << (bs_code - 8);
    if (rate_code <= 11) {
        h.rate = rate_code == 0 ? 0 : rate_code == 1 ? 88200 : rate_code == 2 ? 176400 : rate_code == 3 ? 192000 : rate_code == 4 ? 8000 :
                 rate_code == 5 ? 16000 : rate_code == 6 ? 22050 : rate_code == 7 ? 24000 : rate_code == 8 ? 32000 : rate_code == 9 ? 44100 :
                 rate_code == 10 ? 48000 : 96000;
    } else if (rate_code == 12) { if (pos + 1 >= n) return 0; h.rate = (int)p[pos] * 1000; pos += 1; }
    else { if (pos + 2 >= n) return 0; h.rate = (((int)p[pos] << 8) | (int)p[pos + 1]) * (rate_code == 13 ? 1 : 10); pos += 2; }
    if (pos >= n) return 0;
    if (fl_crc8(p, pos) != p[pos]) return 0;
    return pos + 1;
}

// ---- bit reader ------------------------------------------------------------------------------------------------------------------
// MSB-first over p[0, n).  `acc` holds `cnt` unread bits at its top, zeros below.  Bytes at and past n are never loaded: they read
// as zero, and fl_over() then says that more was consumed than the frame holds.
struct FlBits {
    const uint8_t* p;
    int64_t n, next;
    uint64_t acc;
    int cnt;
};
NAFP_FLAC_HD void fl_open(FlBits& b, const uint8_t* p, int64_t n) { b.p = p; b.n = n; b.next = 0; b.acc = 0; b.cnt = 0; }
// After a refill at least 33 bits are there (zeros past the end).  Single bytes up to the next 4-byte aligned address (once per frame:
// frames start anywhere) and over the frame's last bytes, whole 32-bit words in between: a lane waits for ONE load per 32 bits
// of stream, not four.
NAFP_FLAC_HD void fl_refill(FlBits& b) {
    if (b.cnt > 32) return;
    while (b.cnt <= 56 && ((((uintptr_t)(b.p + b.next)) & 3) != 0 || b.next + 4 > b.n)) {
        const uint64_t v = b.next < b.n ? b.p[b.next] : 0;
        b.acc |= v << (56 - b.cnt);
        b.cnt += 8;
        ++b.next;
    }
    if (b.cnt <= 32) {                                       // here: aligned, and four more bytes inside the frame
        uint32_t w;
        __builtin_memcpy(&w, __builtin_assume_aligned(b.p + b.next, 4), 4);
        b.acc |= (uint64_t)__builtin_bswap32(w) << (32 - b.cnt);
        b.cnt += 32;
        b.next += 4;
    }
}
NAFP_FLAC_HD int64_t fl_consumed_bits(const FlBits& b) { return b.next * 8 - b.cnt; }
NAFP_FLAC_HD bool fl_over(const FlBits& b) { return fl_consumed_bits(b) > b.n * 8; }
// nbits in 0 .. 32
NAFP_FLAC_HD uint32_t fl_u(FlBits& b, int nbits) {
    fl_refill(b);
    if (nbits <= 0) return 0;
    const uint32_t v = (uint32_t)(b.acc >> (64 - nbits));
    b.acc <<= nbits;
    b.cnt -= nbits;
    return v;
}
NAFP_FLAC_HD int32_t fl_s(FlBits& b, int nbits) {
    if (nbits <= 0) return 0;
    const uint32_t v = fl_u(b, nbits), m = 1u << (nbits - 1);
    return (int32_t)((v ^ m) - m);
}
// zero bits before the next one bit; *bad is set when the run exceeds max_q or reaches the frame's end
NAFP_FLAC_HD uint32_t fl_unary(FlBits& b, uint32_t max_q, bool* bad) {
    uint64_t q = 0;
    for (;;) {
        fl_refill(b);
        if (b.acc == 0) {
            q += (uint64_t)b.cnt;
            b.cnt = 0;
            if (q > max_q || fl_over(b) || b.next >= b.n) { *bad = true; return 0; }
            continue;
        }
        const int z = __builtin_clzll(b.acc);                // z < cnt: the bits below cnt are zero
        q += (uint64_t)z;
        b.acc = (b.acc << z) << 1;
        b.cnt -= z + 1;
        if (q > max_q) { *bad = true; return 0; }
        return (uint32_t)q;
    }
}

// ---- frame record ----------------------------------------------------------------------------------------------------------------
NAFP_FLAC_HD bool fl_depth_taken(int bps) { return bps == 8 || bps == 12 || bps == 16 || bps == 20 || bps == 24; }
NAFP_FLAC_HD int fl_container(int bps) { return bps <= 16 ? 2 : 3; }

// 0, NAFP_FLAC_NO_RANGE (the record states no range of the scratch arena: nothing is written) or NAFP_FLAC_BAD_RECORD (the range it
// states is zeroed)
NAFP_FLAC_HD int fl_record_fault(const nafp_flac_frame& r, int64_t raw_size, int64_t scratch_size) {
    if (r.channels < 1 || r.channels > FL_MAX_CHANNELS || r.block_size < 1 || r.block_size > FL_MAX_BLOCK || r.bps < 1 || r.bps > 24 ||
        r.scratch_off < 0)
        return NAFP_FLAC_NO_RANGE;
    const int64_t bytes = (int64_t)r.block_size * r.channels * fl_container(r.bps);
    if (scratch_size < bytes || r.scratch_off > scratch_size - bytes) return NAFP_FLAC_NO_RANGE;
    if (!fl_depth_taken(r.bps) || r.rate < 1 || r.rate > FL_MAX_RATE || r.n_bytes < 1 || r.raw_off < 0 || raw_size < r.n_bytes ||
        r.raw_off > raw_size - r.n_bytes)
        return NAFP_FLAC_BAD_RECORD;
    return 0;
}

NAFP_FLAC_HD int64_t fl_ws_index(const nafp_flac_frame& r, int bw, int k) { return (r.scratch_off + (int64_t)k * bw) >> 1; }

// ---- frame decode ----------------------------------------------------------------------------------------------------------------
constexpr int FL_RING = 64;            // samples of a channel kept behind the decoder: 32 of history + 32 waiting for their store
constexpr int FL_REG_TAPS = 12;        // predictors up to this order run on statically indexed registers

// One subframe of width w bits: `block` values to ws (wasted bits undone).  coef: 32 int32, hist: FL_RING int32, element j at
// [j * stride] (the kernel keeps them in LDS, lanes interleaved).  Every sample goes through the ring `hist`; the workspace is
// written 32 samples at a time, because on the device a lane's next load of stream bytes waits for its stores to be acknowledged:
// a store after every sample made the sample wait for memory, a burst every 32 does not.  The prediction reads the ring for orders
// above FL_REG_TAPS and registers below: coefficients and the last FL_REG_TAPS samples in two fully unrolled arrays (zeros beyond the
// order), one 32 x 32 -> 64-bit multiply-add per tap.  Returns 0 or a NAFP_FLAC_* reason.
NAFP_FLAC_HD int fl_subframe(FlBits& b, const nafp_flac_frame& rec, int bw, int c, int w, int32_t* ws, int32_t* coef, int32_t* hist, int stride) {
    const int block = rec.block_size;
    const int base = c * block;
    bool bad = false;
    if (fl_u(b, 1) != 0) return NAFP_FLAC_BAD_SUBFRAME;
    const int type = (int)fl_u(b, 6);
    int wasted = 0;
    if (fl_u(b, 1)) {
        wasted = (int)fl_unary(b, (uint32_t)w, &bad) + 1;
        if (bad) return fl_over(b) ? NAFP_FLAC_TRUNCATED : NAFP_FLAC_BAD_SUBFRAME;
    }
    if (wasted >= w) return NAFP_FLAC_BAD_SUBFRAME;
    w -= wasted;
    if (type == 0) {
        const uint32_t v = (uint32_t)fl_s(b, w) << wasted;
        for (int i = 0; i < block; ++i) ws[fl_ws_index(rec, bw, base + i)] = (int32_t)v;
        return fl_over(b) ? NAFP_FLAC_TRUNCATED : 0;
    }
    // sample i into the ring; the 32 samples that end at i, or the block's last few, out to the workspace
    auto put = [&](int i, int32_t s) {
        hist[(i & (FL_RING - 1)) * stride] = s;
        if ((i & 31) == 31 || i == block - 1)
            for (int k = i & ~31; k <= i; ++k)
                ws[fl_ws_index(rec, bw, base + k)] = (int32_t)((uint32_t)hist[(k & (FL_RING - 1)) * stride] << wasted);
    };
    if (type == 1) {
        for (int i = 0; i < block; ++i) {
            put(i, fl_s(b, w));
            if ((i & 255) == 255 && fl_over(b)) return NAFP_FLAC_TRUNCATED;
        }
        return fl_over(b) ? NAFP_FLAC_TRUNCATED : 0;
    }
    int order, shift = 0;
    if (type >= 8 && type <= 12) order = type - 8;
    else if (type >= 32) order = type - 31;
    else return NAFP_FLAC_BAD_SUBFRAME;
    if (order > block) return NAFP_FLAC_BAD_SUBFRAME;
    for (int i = 0; i < order; ++i) put(i, fl_s(b, w));
    if (type >= 32) {
        const int precision = (int)fl_u(b, 4) + 1;
        if (precision == 16) return NAFP_FLAC_BAD_SUBFRAME;
        shift = fl_s(b, 5);
        if (shift < 0) return NAFP_FLAC_BAD_SUBFRAME;
        for (int j = 0; j < order; ++j) coef[j * stride] = fl_s(b, precision);
    } else {
        const int32_t c0 = order == 1 ? 1 : order == 2 ? 2 : order == 3 ? 3 : 4;
        const int32_t c1 = order == 2 ? -1 : order == 3 ? -3 : -6;
        const int32_t c2 = order == 3 ? 1 : 4;
        if (order > 0) coef[0] = c0;
        if (order > 1) coef[stride] = c1;
        if (order > 2) coef[2 * stride] = c2;
        if (order > 3) coef[3 * stride] = -1;
    }
    if (fl_over(b)) return NAFP_FLAC_TRUNCATED;
    const bool in_regs = order <= FL_REG_TAPS;
    int32_t cr[FL_REG_TAPS], hr[FL_REG_TAPS];                 // hr[j] = sample i - 1 - j
#pragma unroll
    for (int j = 0; j < FL_REG_TAPS; ++j) {
        const bool on = in_regs && j < order;
        cr[j] = on ? coef[j * stride] : 0;
        hr[j] = on ? hist[((order - 1 - j) & (FL_RING - 1)) * stride] : 0;
    }
    // residual
    const int method = (int)fl_u(b, 2);
    if (method > 1) return NAFP_FLAC_BAD_RESIDUAL;
    const int pbits = method ? 5 : 4, esc = method ? 31 : 15;
    const int po = (int)fl_u(b, 4);
    if ((block & ((1 << po) - 1)) != 0 || (block >> po) < order) return NAFP_FLAC_BAD_RESIDUAL;
    const int per = block >> po;
    int i = order;
    for (int part = 0; part < (1 << po); ++part) {
        const int param = (int)fl_u(b, pbits);
        const int end = (part + 1) * per;
        const int raw_bits = param == esc ? (int)fl_u(b, 5) : 0;
        const uint32_t max_q = param == esc ? 0u : (0xffffffffu >> param);
        for (; i < end; ++i) {
            int32_t res;
            if (param == esc) {
                res = fl_s(b, raw_bits);
            } else {
                const uint32_t q = fl_unary(b, max_q, &bad);
                if (bad) return fl_over(b) || b.next >= b.n ? NAFP_FLAC_TRUNCATED : NAFP_FLAC_BAD_RESIDUAL;
                const uint32_t u = (q << param) | fl_u(b, param);
                res = (int32_t)((u >> 1) ^ (0u - (u & 1u)));
            }
            int64_t sum = 0;
            if (in_regs) {
#pragma unroll
                for (int j = 0; j < FL_REG_TAPS; ++j) sum += (int64_t)cr[j] * (int64_t)hr[j];
            } else {
                for (int j = 0; j < order; ++j) sum += (int64_t)coef[j * stride] * (int64_t)hist[((i - 1 - j) & (FL_RING - 1)) * stride];
            }
            const int32_t s = (int32_t)((uint32_t)res + (uint32_t)(int32_t)(sum >> shift));
#pragma unroll
            for (int j = FL_REG_TAPS - 1; j > 0; --j) hr[j] = hr[j - 1];
            hr[0] = s;
            put(i, s);
        }
        if (fl_over(b)) return NAFP_FLAC_TRUNCATED;
    }
    return 0;
}

// The frame at fp[0, rec.n_bytes), the record already passed fl_record_fault.  crc_tab: fl_crc16_entry(0 .. 255).  Returns the status;
// *assign is the frame's channel assignment (valid with status 0).
NAFP_FLAC_HD int fl_decode_frame(const uint8_t* fp, const nafp_flac_frame& rec, int32_t* ws, int32_t* coef, int32_t* hist, int stride,
                                 const uint16_t* crc_tab, int* assign) {
    FlHeader h;
    const int hl = fl_parse_header(fp, rec.n_bytes, h);
    *assign = 0;
    if (hl == 0) return NAFP_FLAC_BAD_HEADER;
    if (h.block_size != rec.block_size || h.channels != rec.channels || (h.bps != 0 && h.bps != rec.bps) || (h.rate != 0 && h.rate != rec.rate))
        return NAFP_FLAC_HEADER_MISMATCH;
    *assign = h.assign;
    const int bw = fl_container(rec.bps);
    FlBits b;
    fl_open(b, fp + hl, (int64_t)rec.n_bytes - hl);
    for (int c = 0; c < rec.channels; ++c) {
        const bool side = (h.assign == 8 && c == 1) || (h.assign == 9 && c == 0) || (h.assign == 10 && c == 1);
        const int st = fl_subframe(b, rec, bw, c, rec.bps + (side ? 1 : 0), ws, coef, hist, stride);
        if (st != 0) return st;
    }
    fl_refill(b);
    fl_u(b, b.cnt & 7);                                      // zero padding to the byte boundary
    const uint32_t stated = fl_u(b, 16);
    if (fl_over(b)) return NAFP_FLAC_TRUNCATED;
    const int64_t end = hl + fl_consumed_bits(b) / 8;        // <= rec.n_bytes
    return fl_crc16(fp, end - 2, crc_tab) == stated ? 0 : NAFP_FLAC_BAD_CRC16;
}

// Output element (sample i, channel c) of a frame decoded with status 0: decorrelate, justify, store little-endian.
NAFP_FLAC_HD void fl_store_element(const nafp_flac_frame& rec, int assign, const int32_t* ws, uint8_t* scratch, int i, int c) {
    const int bw = fl_container(rec.bps), block = rec.block_size;
    uint32_t v = (uint32_t)ws[fl_ws_index(rec, bw, c * block + i)];
    if (assign >= 8 && rec.channels == 2) {
        const uint32_t a0 = c == 0 ? v : (uint32_t)ws[fl_ws_index(rec, bw, i)];
        const uint32_t a1 = c == 1 ? v : (uint32_t)ws[fl_ws_index(rec, bw, block + i)];
        if (assign == 8) v = c == 0 ? a0 : a0 - a1;                                // left, side
        else if (assign == 9) v = c == 0 ? a0 + a1 : a1;                           // side, right
        else {                                                                     // mid, side
            const uint32_t m = (a0 << 1) | (a1 & 1u);
            v = (uint32_t)((int32_t)(c == 0 ? m + a1 : m - a1) >> 1);
        }
    }
    uint8_t* dst = scratch + rec.scratch_off + ((int64_t)i * rec.channels + c) * bw;
    if (bw == 2) {
        v <<= 16 - rec.bps;
        dst[0] = (uint8_t)(v & 0xffu);
        dst[1] = (uint8_t)((v >> 8) & 0xffu);
    } else {
        v <<= 24 - rec.bps;
        dst[0] = (uint8_t)(v & 0xffu);
        dst[1] = (uint8_t)((v >> 8) & 0xffu);
        dst[2] = (uint8_t)((v >> 16) & 0xffu);
    }
}

// ---- host only: STREAMINFO and the frame index -----------------------------------------------------------------------------------
// The stream's STREAMINFO after an optional ID3v2 tag; info->refusal names what is not taken (NAFP_FLAC_REFUSE_*), 0 if all is.
inline int fl_streaminfo(const uint8_t* p, int64_t n, nafp_flac_info* info) {
    *info = nafp_flac_info{};
    int64_t pos = 0;
    if (n >= 10 && p[0] == 'I' && p[1] == 'D' && p[2] == '3') {
        const int64_t size = ((int64_t)(p[6] & 0x7f) << 21) | ((int64_t)(p[7] & 0x7f) << 14) | ((int64_t)(p[8] & 0x7f) << 7) | (p[9] & 0x7f);
        pos = 10 + size + ((p[5] & 0x10) ? 10 : 0);
    }
    if (pos + 4 > n || p[pos] != 'f' || p[pos + 1] != 'L' || p[pos + 2] != 'a' || p[pos + 3] != 'C') {
        const bool ogg = pos + 4 <= n && p[pos] == 'O' && p[pos + 1] == 'g' && p[pos + 2] == 'g' && p[pos + 3] == 'S';
        info->refusal = ogg ? NAFP_FLAC_REFUSE_OGG : NAFP_FLAC_REFUSE_MARKER;
        return NAFP_OK;
    }
    pos += 4;
    if (pos + 4 + 34 > n || (p[pos] & 0x7f) != 0 || p[pos + 1] != 0 || p[pos + 2] != 0 || p[pos + 3] != 34) {
        info->refusal = NAFP_FLAC_REFUSE_STREAMINFO;
        return NAFP_OK;
    }
    bool last = (p[pos] & 0x80) != 0;
    const uint8_t* s = p + pos + 4;
    info->min_block = (s[0] << 8) | s[1];
    info->max_block = (s[2] << 8) | s[3];
    info->rate = (s[10] << 12) | (s[11] << 4) | (s[12] >> 4);
    info->channels = ((s[12] >> 1) & 7) + 1;
    info->bps = (((s[12] & 1) << 4) | (s[13] >> 4)) + 1;
    info->total_samples = ((int64_t)(s[13] & 15) << 32) | ((int64_t)s[14] << 24) | ((int64_t)s[15] << 16) | ((int64_t)s[16] << 8) | s[17];
    for (int k = 0; k < 16; ++k) info->md5[k] = s[18 + k];
    pos += 4 + 34;
    while (!last && pos + 4 <= n) {
        last = (p[pos] & 0x80) != 0;
        pos += 4 + (((int64_t)p[pos + 1] << 16) | ((int64_t)p[pos + 2] << 8) | p[pos + 3]);
    }
    info->audio_off = pos < n ? pos : n;
    if (!fl_depth_taken(info->bps)) info->refusal = NAFP_FLAC_REFUSE_DEPTH;
    else if (info->max_block > FL_MAX_BLOCK) info->refusal = NAFP_FLAC_REFUSE_BLOCK;
    return NAFP_OK;
}

struct FlCrc16Table {
    uint16_t t[256];
    FlCrc16Table() { for (uint32_t i = 0; i < 256; ++i) t[i] = (uint16_t)fl_crc16_entry(i); }
};
inline const uint16_t* fl_crc16_table() { static const FlCrc16Table tab; return tab.t; }

// The frames at frames[0, n): what the kernels write, from the same functions -- scratch bytes and one status per frame.  A failed
// frame's range is zeroed; NAFP_FLAC_NO_RANGE writes nothing.  ws: scratch_size / 2 + 1 int32.
inline void fl_decode_frames(const uint8_t* raw, int64_t raw_size, const nafp_flac_frame* frames, int64_t n, uint8_t* scratch,
                             int64_t scratch_size, int32_t* status, int32_t* ws) {
    int32_t coef[FL_MAX_ORDER], hist[FL_RING];
    for (int64_t f = 0; f < n; ++f) {
        const nafp_flac_frame& rec = frames[f];
        int st = fl_record_fault(rec, raw_size, scratch_size), assign = 0;
        if (st == 0) st = fl_decode_frame(raw + rec.raw_off, rec, ws, coef, hist, 1, fl_crc16_table(), &assign);
        if (status) status[f] = st;
        if (st == NAFP_FLAC_NO_RANGE) continue;
        if (st != 0) {
            const int64_t bytes = (int64_t)rec.block_size * rec.channels * fl_container(rec.bps);
            for (int64_t k = 0; k < bytes; ++k) scratch[rec.scratch_off + k] = 0;
            continue;
        }
        for (int i = 0; i < rec.block_size; ++i)
            for (int c = 0; c < rec.channels; ++c) fl_store_element(rec, assign, ws, scratch, i, c);
    }
}

// The frame index of a whole stream (header comment of nafp_flac_index_host, include/nafp.h).  Candidates are found by the sync
// pattern, kept when their header parses (reserved bits and codes, coded number, CRC-8) AND continues the chain: in a fixed-blocksize
// stream the frame number is the predecessor's plus one and the predecessor is a full block; in a variable-blocksize stream the
// coded sample number is the predecessor's first sample plus its block size.  The chain starts at the first valid header, whatever
// its number.  A candidate that breaks continuity is dropped.  A FALSE candidate that keeps continuity by chance is not recognised
// here: it ends its predecessor early and both are caught by their CRC-16 when they are decoded -- failed frames, zeros.  A last
// frame that the file cuts short is left out.  At most `cap` entries are written; info->n_indexed counts all.
inline int fl_index(const uint8_t* p, int64_t n, nafp_flac_info* info, nafp_flac_index_entry* out, int64_t cap) {
    const int st = fl_streaminfo(p, n, info);
    if (st != NAFP_OK || info->refusal) return st;
    int64_t count = 0, samples = 0;
    nafp_flac_index_entry prev{};
    int prev_blocking = 0;
    int64_t prev_number = 0;
    for (int64_t pos = info->audio_off; pos + 6 <= n;) {
        if (p[pos] != 0xffu || (p[pos + 1] & 0xfeu) != 0xf8u) { ++pos; continue; }
        FlHeader h;
        const int hl = fl_parse_header(p + pos, n - pos, h);
        bool take = hl > 0 && h.block_size <= info->max_block;
        if (take && count > 0) {
            if (h.blocking != prev_blocking) take = false;
            else if (h.blocking == 0) take = h.number == prev_number + 1 && prev.block_size == info->max_block;
            else take = h.number == prev.first_sample + prev.block_size;
        }
        if (!take) { ++pos; continue; }
        if (count > 0) {
            prev.n_bytes = pos - prev.offset;
            if (count - 1 < cap) out[count - 1] = prev;
            samples += prev.block_size;
        }
        prev.offset = pos;
        prev.first_sample = h.blocking ? h.number : h.number * (int64_t)info->max_block;
        prev.block_size = h.block_size;
        prev.n_bytes = 0;
        prev_blocking = h.blocking;
        prev_number = h.number;
        ++count;
        pos += hl;
    }
    if (count > 0) {
        // the last frame: taken only if the file holds all of it (one host decode into a buffer of its own)
        prev.n_bytes = n - prev.offset;
        nafp_flac_frame rec{};
        rec.raw_off = prev.offset; rec.scratch_off = 0; rec.n_bytes = (int32_t)(prev.n_bytes < (1 << 30) ? prev.n_bytes : (1 << 30)); rec.block_size = prev.block_size;
        rec.channels = info->channels; rec.bps = info->bps; rec.rate = info->rate > 0 ? info->rate : 1;
        const int64_t bytes = (int64_t)rec.block_size * rec.channels * fl_container(rec.bps);
        std::vector<uint8_t> tmp((size_t)bytes);
        std::vector<int32_t> ws((size_t)(bytes / 2 + 1));
        int32_t status = 0;
        fl_decode_frames(p, n, &rec, 1, tmp.data(), bytes, &status, ws.data());
        if (status == NAFP_FLAC_TRUNCATED) --count;
        else {
            if (count - 1 < cap) out[count - 1] = prev;
            samples += prev.block_size;
        }
    }
    info->n_indexed = count;
    info->indexed_samples = samples;
    return NAFP_OK;
}

}  // namespace nafp

#endif
