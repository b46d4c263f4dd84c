// Stand-alone host check of csrc/codec_decode.h -- the arithmetic the codec kernel and nafp_codec_decode_host share -- under the
// address and undefined-behaviour sanitizers, with no GPU and no Python:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/codec_decode_check.cpp -o codec_decode_check
//     ./codec_decode_check
//
// Blocks of uniformly random bytes (they reach step indices above 88, bPredictor above 6, negative and tiny iDelta and both sample
// clamps) of every codec, channel count and the block_align grid are decoded from a heap buffer of exactly n_blocks * block_align
// bytes into one of exactly n_blocks * spb * channels int16, so that a read or write one byte outside either is reported; signed
// overflow or an out-of-range shift anywhere in the int32 arithmetic is reported too.  Prints one checksum line per case and
// "ok"; exit status 0 only if nothing was reported.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../neural-audio-fp_amd/csrc/codec_decode.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {                                   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

int main() {
    using namespace nafp;
    const int aligns[] = {1, 2, 3, 8, 9, 15, 16, 24, 37, 255, 256, 512, 1024, 2047, 2048, 4095, 4096};
    int cases = 0;
    for (int codec = NAFP_CODEC_ALAW; codec <= NAFP_CODEC_MS4; ++codec)
        for (int ch = 1; ch <= 8; ++ch)
            for (int align : aligns) {
                const int spb = cd_samples_per_block(codec, ch, align);
                if (spb < 0) continue;
                const int64_t n_blocks = align <= 64 ? 300 : (align <= 512 ? 40 : 6);
                uint8_t* in = (uint8_t*)malloc((size_t)(n_blocks * align));
                int16_t* out = (int16_t*)malloc((size_t)(n_blocks * spb * ch) * sizeof(int16_t));
                for (int64_t i = 0; i < n_blocks * align; ++i) in[i] = (uint8_t)rnd();
                if (codec == NAFP_CODEC_MS4 && align > 7 * ch + 2) {       // iDelta = -32768, -1, 0, 1 and 32767 in the first blocks
                    const int v[5] = {-32768, -1, 0, 1, 32767};
                    for (int b = 0; b < 5; ++b)
                        for (int c = 0; c < ch; ++c) {
                            in[b * align + ch + 2 * c] = (uint8_t)(v[b] & 0xff);
                            in[b * align + ch + 2 * c + 1] = (uint8_t)((v[b] >> 8) & 0xff);
                        }
                }
                cd_decode_blocks(codec, ch, align, spb, in, n_blocks, out);
                nafp_codec_piece pc = {0, n_blocks, 0, codec, ch, align, spb};
                if (cd_piece_fault(pc, n_blocks * align, n_blocks * spb * ch) != 0) { printf("piece check failed\n"); return 1; }
                pc.n_blocks += 1;
                if (cd_piece_fault(pc, n_blocks * align, (n_blocks + 1) * spb * ch) != 2) { printf("piece check failed\n"); return 1; }
                uint32_t sum = 0;
                int lo = 0, hi = 0;
                for (int64_t i = 0; i < n_blocks * spb * ch; ++i) {
                    sum = sum * 31u + (uint16_t)out[i];
                    lo = out[i] < lo ? out[i] : lo;
                    hi = out[i] > hi ? out[i] : hi;
                }
                printf("codec %d channels %d block_align %4d spb %4d blocks %3d: min %6d max %6d checksum %08x\n", codec, ch, align, spb,
                       (int)n_blocks, lo, hi, sum);
                free(in);
                free(out);
                ++cases;
            }
    printf("ok: %d cases\n", cases);
    return 0;
}
