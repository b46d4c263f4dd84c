// Stand-alone host check of csrc/flac_decode.h -- the bit reader, header parse, subframe decode, CRC-16, output packing and frame
// index that the FLAC kernels, nafp_flac_decode_host and nafp_flac_index_host share -- under the address and undefined-behaviour
// sanitizers, with no GPU and no Python:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/flac_host_check.cpp -o flac_host_check
//     ./flac_host_check [tests/golden/flac_streams_v1.bin] [mutations per stream, default 400]
//
// The seed streams are valid FLAC streams written by tests/_flac_ref.py (golden_streams(): every depth, 1 to 8 channels, all channel
// assignments, constant / verbatim / fixed / LPC subframes up to order 32, both Rice methods, escape partitions, wasted bits, fixed
// and variable block sizes).  Each is first decoded as it is (every frame must come out with status 0), then as seeded MUTATIONS:
// single bit flips, truncations, overwritten bytes (header and parameter fields among them: the first 24 bytes of a frame are hit
// four times as often), runs of 0x00 (over-long unary runs) and 0xff, and frame records that disagree with the stream.  Every
// mutated stream lives in a heap buffer of exactly its length and is indexed (fl_index) and decoded (fl_decode_frames) twice -- with
// the records of its own index and with the records of the valid stream's index -- into an output buffer of exactly the stated
// size and a workspace of exactly scratch_size / 2 + 1 words, so that a read or write one byte outside any of them, a signed overflow
// or an out-of-range shift is reported.  After every decode the frames that failed must be all zero and 8 guard bytes around each
// arena untouched.  The six NAMED mutations of stream 0 that tests/test_gpu_flac.py launches on the device (named_mutations() in
// tests/_flac_ref.py: same definitions) are run first.  Prints one line per stream and "ok: N mutations"; exit status 0 only if
// nothing was reported.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../neural-audio-fp_amd/csrc/flac_decode.h"

using namespace nafp;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {                                   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

struct Indexed {
    nafp_flac_info info;
    std::vector<nafp_flac_index_entry> frames;
};

// index of the stream in an exact-size heap copy
static Indexed index_of(const std::vector<uint8_t>& data) {
    Indexed r;
    uint8_t* p = (uint8_t*)malloc(data.size() ? data.size() : 1);
    memcpy(p, data.data(), data.size());
    if (fl_index(p, (int64_t)data.size(), &r.info, nullptr, 0) != NAFP_OK) { printf("fl_index failed\n"); exit(1); }
    r.frames.resize((size_t)r.info.n_indexed);
    if (r.info.n_indexed > 0) fl_index(p, (int64_t)data.size(), &r.info, r.frames.data(), r.info.n_indexed);
    free(p);
    return r;
}

static std::vector<nafp_flac_frame> records_of(const Indexed& ix) {
    std::vector<nafp_flac_frame> recs;
    const int bw = fl_container(ix.info.bps);
    int64_t at = 0;
    for (const nafp_flac_index_entry& e : ix.frames) {
        nafp_flac_frame r{};
        r.raw_off = e.offset;
        r.scratch_off = at;
        r.n_bytes = (int32_t)(e.n_bytes < (1 << 30) ? e.n_bytes : (1 << 30));
        r.block_size = e.block_size;
        r.channels = ix.info.channels;
        r.bps = ix.info.bps;
        r.rate = ix.info.rate;
        recs.push_back(r);
        at += (int64_t)e.block_size * ix.info.channels * bw;
    }
    return recs;
}

static int64_t decodes = 0;

// decode `recs` over an exact-size copy of `data`; returns the number of failed frames, exits on a broken promise
static int decode_checked(const std::vector<uint8_t>& data, const std::vector<nafp_flac_frame>& recs, int64_t scratch_size, bool must_pass, bool check_zero = true) {
    const int G = 8;
    uint8_t* raw = (uint8_t*)malloc(data.size() ? data.size() : 1);
    memcpy(raw, data.data(), data.size());
    uint8_t* out = (uint8_t*)malloc((size_t)scratch_size + 2 * G);
    memset(out, 0xa5, (size_t)scratch_size + 2 * G);
    int32_t* ws = (int32_t*)malloc(sizeof(int32_t) * (size_t)(scratch_size / 2 + 1));
    std::vector<int32_t> status(recs.size() + 1, -1);
    fl_decode_frames(raw, (int64_t)data.size(), recs.data(), (int64_t)recs.size(), out + G, scratch_size, status.data(), ws);
    ++decodes;
    int failed = 0;
    for (int k = 0; k < G; ++k)
        if (out[k] != 0xa5 || out[G + scratch_size + k] != 0xa5) { printf("guard bytes written\n"); exit(1); }
    for (size_t f = 0; f < recs.size(); ++f) {
        if (status[f] < 0 || status[f] > NAFP_FLAC_NO_RANGE) { printf("status %d\n", status[f]); exit(1); }
        if (status[f] == 0) continue;
        ++failed;
        if (must_pass) { printf("valid frame %zu failed with status %d\n", f, status[f]); exit(1); }
        if (status[f] == NAFP_FLAC_NO_RANGE || !check_zero) continue;      // (records whose ranges overlap: the later frame wins)
        const int64_t bytes = (int64_t)recs[f].block_size * recs[f].channels * fl_container(recs[f].bps);
        for (int64_t k = 0; k < bytes; ++k)
            if (out[G + recs[f].scratch_off + k] != 0) { printf("failed frame %zu is not zero\n", f); exit(1); }
    }
    free(raw); free(out); free(ws);
    return failed;
}

static int64_t scratch_of(const std::vector<nafp_flac_frame>& recs) {
    int64_t n = 0;
    for (const nafp_flac_frame& r : recs) {
        const int64_t end = r.scratch_off + (int64_t)r.block_size * r.channels * fl_container(r.bps);
        n = end > n ? end : n;
    }
    return n;
}

// one mutated stream: indexed and decoded with its own records and with the valid stream's
static int run_mutant(const std::vector<uint8_t>& m, const std::vector<nafp_flac_frame>& valid_recs, int64_t valid_scratch) {
    int failed = 0;
    const Indexed ix = index_of(m);
    if (ix.info.refusal == 0 && !ix.frames.empty()) {
        const std::vector<nafp_flac_frame> recs = records_of(ix);
        failed += decode_checked(m, recs, scratch_of(recs), false);
    }
    failed += decode_checked(m, valid_recs, valid_scratch, false);
    return failed;
}

int main(int argc, char** argv) {
    const char* path = argc > 1 ? argv[1] : "tests/golden/flac_streams_v1.bin";
    const int per_stream = argc > 2 ? atoi(argv[2]) : 400;
    FILE* fh = fopen(path, "rb");
    if (!fh) { printf("cannot open %s\n", path); return 1; }
    std::vector<uint8_t> blob;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, fh)) > 0;) blob.insert(blob.end(), buf, buf + n);
    fclose(fh);
    if (blob.size() < 12 || memcmp(blob.data(), "NAFPFLAC", 8) != 0) { printf("%s: not a stream file\n", path); return 1; }
    uint32_t count;
    memcpy(&count, blob.data() + 8, 4);
    size_t pos = 12;
    int64_t mutations = 0, failed_frames = 0;
    for (uint32_t s = 0; s < count; ++s) {
        uint32_t len;
        memcpy(&len, blob.data() + pos, 4);
        const std::vector<uint8_t> data(blob.begin() + pos + 4, blob.begin() + pos + 4 + len);
        pos += 4 + len;
        const Indexed ix = index_of(data);
        if (ix.info.refusal != 0 || ix.frames.empty()) { printf("stream %u: refused or empty\n", s); return 1; }
        const std::vector<nafp_flac_frame> recs = records_of(ix);
        const int64_t scratch = scratch_of(recs);
        decode_checked(data, recs, scratch, true);
        int64_t failed = 0;
        if (s == 0 && recs.size() >= 3) {                     // the named mutations (tests/_flac_ref.py named_mutations())
            const nafp_flac_index_entry& e = ix.frames[1];
            FlHeader h;
            const int hl = fl_parse_header(data.data() + e.offset, e.n_bytes, h);
            std::vector<uint8_t> m = data;
            m[e.offset + e.n_bytes / 2] ^= 0x10;              // a body bit flip
            failed += run_mutant(m, recs, scratch); ++mutations;
            std::vector<nafp_flac_frame> r2 = recs;           // a truncation: the record ends three bytes early
            r2[1].n_bytes -= 3;
            failed += decode_checked(data, r2, scratch, false); ++mutations;
            m = data;                                         // an over-long unary run: the body is zeros
            for (int64_t k = e.offset + hl + 2; k < e.offset + e.n_bytes - 1; ++k) m[k] = 0;
            failed += run_mutant(m, recs, scratch); ++mutations;
            m = data; m[e.offset + hl] = 0x7e;                // subframe type 63: LPC order 32 above the block size of 16
            failed += run_mutant(m, recs, scratch); ++mutations;
            m = data; m[e.offset + hl] = 0x04;                // subframe type 2: reserved
            failed += run_mutant(m, recs, scratch); ++mutations;
            r2 = recs; r2[1].block_size += 1;                 // inconsistent records: block size, channels, raw range, no range
            failed += decode_checked(data, r2, scratch + 64, false, false); ++mutations;
            r2 = recs; r2[1].channels = r2[1].channels == 1 ? 2 : 1; r2[1].block_size = r2[1].channels == 1 ? 2 * recs[1].block_size : recs[1].block_size / 2;
            failed += decode_checked(data, r2, scratch, false); ++mutations;
            r2 = recs; r2[1].raw_off = (int64_t)data.size() - r2[1].n_bytes + 1;
            failed += decode_checked(data, r2, scratch, false); ++mutations;
            r2 = recs; r2[1].scratch_off = scratch - 1;
            failed += decode_checked(data, r2, scratch, false); ++mutations;
        }
        for (int k = 0; k < per_stream; ++k) {
            std::vector<uint8_t> m = data;
            const uint32_t kind = rnd() % 6;
            const nafp_flac_index_entry& e = ix.frames[rnd() % ix.frames.size()];
            // where: anywhere in the file, or (half the time) in a frame, its first 24 bytes favoured
            int64_t at = rnd() % m.size();
            if (rnd() & 1) at = e.offset + ((rnd() & 3) ? rnd() % (e.n_bytes < 24 ? e.n_bytes : 24) : rnd() % e.n_bytes);
            if (kind == 0) m[at] ^= (uint8_t)(1u << (rnd() & 7));
            else if (kind == 1) m.resize((size_t)at);
            else if (kind == 2) m[at] = (uint8_t)rnd();
            else if (kind == 3 || kind == 4) {
                const int64_t n = 1 + rnd() % 64;
                for (int64_t j = at; j < at + n && j < (int64_t)m.size(); ++j) m[j] = kind == 3 ? 0x00 : 0xff;
            } else {                                          // records that disagree with the stream
                std::vector<nafp_flac_frame> r2 = recs;
                nafp_flac_frame& r = r2[rnd() % r2.size()];
                const uint32_t w = rnd() % 7;
                if (w == 0) r.block_size = (int32_t)(rnd() % 20000) - 100;
                else if (w == 1) r.channels = (int32_t)(rnd() % 12) - 1;
                else if (w == 2) r.bps = (int32_t)(rnd() % 40) - 2;
                else if (w == 3) r.n_bytes = (int32_t)(rnd() % (2 * m.size() + 1)) - 5;
                else if (w == 4) r.raw_off = (int64_t)(rnd() % (2 * m.size() + 1)) - 5;
                else if (w == 5) r.scratch_off = (int64_t)(rnd() % (2 * scratch + 1)) - 5;
                else r.rate = (int32_t)rnd();
                failed += decode_checked(m, r2, scratch, false, false);
                ++mutations;
                continue;
            }
            failed += run_mutant(m, recs, scratch);
            ++mutations;
        }
        printf("stream %2u: %6zu bytes, %3zu frames, %d ch x %2d bits: valid decode ok, %lld frames of its mutants failed their checks\n", s,
               data.size(), recs.size(), ix.info.channels, ix.info.bps, (long long)failed);
        failed_frames += failed;
    }
    printf("ok: %lld mutations of %u streams, %lld decodes, %lld failed frames, nothing reported\n", (long long)mutations, count,
           (long long)decodes, (long long)failed_frames);
    return 0;
}
