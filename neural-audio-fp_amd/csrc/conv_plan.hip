// The plan of a conv GEMM launch (declarations: nafp_common.h).  Host code only: no kernel, no HIP call; plan_conv_gemm() takes the knobs as an argument.
#include <algorithm>
#include <climits>

#include "nafp_common.h"

namespace nafp {

constexpr int BN = 128;          // column width the tile counts of the policy are expressed in

const ConvKnobs& conv_knobs() {
    static const ConvKnobs k;
    return k;
}

// [r5] The batch size the INFERENCE forward plans for.  Tile shape and split-K factor of a layer used to follow the launch's own
// batch, so the fp32 summation order of a segment -- the last bits of its fingerprint -- depended on how many segments shared its
// launch.  nafp_encoder_forward* now plan every launch as if it held fwd_plan_b() segments (640: the bench
// and generate launch size, so nothing changes there) and only the grid follows B: the bytes of a fingerprint no longer depend on
// TS_BATCH_SZ or on the launch size.  Training plans per launch as before.
int64_t fwd_plan_b() { return conv_knobs().plan_b; }

// Split-K policy: layers whose M x N tiling yields too few workgroups to fill 256 CUs
// (the late convs: M = 640...20480 rows at B = 640) split their K-steps across blockIdx.z.
static int live_k_steps(const ConvGeom& g) {
    // K-steps (BK = 16) of the taps that read real data for at least one output position
    const int n_in = g.axis == 0 ? g.Tin : g.Fin, n_out = g.axis == 0 ? g.Tout : g.Fout;
    int n_live = 0;
    for (int t = 0; t < 3; ++t) {
        bool live = false;
        for (int o = 0; o < n_out && !live; ++o) { const int i = o * g.stride - g.pad + t; live = i >= 0 && i < n_in; }
        n_live += live;
    }
    return n_live * g.Cin / 16;
}

// K-steps (BK = 16) of a tile of the transposed conv: with stride 2 the parity classes of tile_pos()
// carry 2 resp. 1 live taps (1.5 on average), with stride 1 all three.  (An estimate for the split-K policy only: the kernel skips
// dead taps per tile.  [r5] The exact per-class count -- a third of this for the layers whose forward conv has ONE live tap at the
// 1-s input -- was tried in its place: same-box A/B 11.69 vs 11.75 ms at B = 640, 22.29 vs 22.21 at 1280, 85.6 vs 85.2 at 5120:
// the split factor is not what limits those launches -- they share the chip with the side stream's weight gradients.)
static int dgrad_k_steps(const ConvGeom& g) { return (g.stride == 2 ? 3 : 6) * g.Cout / 32; }

static int choose_split(int64_t n_tiles, int k_steps, int64_t out_floats, double slots, const ConvKnobs& knobs) {
    // Score each split factor S by (how full the last round of workgroups is) x (share of a
    // workgroup's time spent in its K-loop rather than prologue/epilogue); 768 = 256 CUs x 3
    // resident workgroups.  Splitting costs a slab round trip, so it must win by a margin.
    if (knobs.splitk == 0) return 1;
    if (knobs.splitk > 0) return knobs.splitk;
    if (n_tiles >= 3072) return 1;
    if (slots == 1280.0)       // forward, 64-column tiles, 5 per CU.  Measured at B = 640: 1280 tiles (convs 6, 8) fill the slots and are
        // best unsplit; 640 tiles in two parts: conv9 (96 K-steps) 0.187 -> 0.167 ms, conv7 (48 K-steps) 0.098 -> 0.096
        return (n_tiles >= 1000 || k_steps / 2 < 24 || 2 * out_floats * 4 > ((int64_t)64 << 20)) ? 1 : 2;
    if (slots == 768.0 && n_tiles <= 200) {
        // few 128 x 128 tiles (the late convs): measured at B = 640 (tools/plan_sweep.sh) a 3-way split is the best or within
        // 2 % of it for 80 and 160 tiles, 6-way for 40; keep at least 8 K-steps per part
        int S = n_tiles <= 40 ? 6 : 3;
        while (S > 1 && (k_steps / S < 8 || (int64_t)S * out_floats * 4 > ((int64_t)64 << 20))) --S;
        return S;
    }
    const double overhead_steps = 6.0;
    int best = 1; double best_score = 0.0;
    for (int S = 1; S <= 16; ++S) {
        const double k = (double)k_steps / S;
        if (S > 1 && (k < 8.0 || (int64_t)S * out_floats * 4 > ((int64_t)64 << 20))) break;
        const double w = (double)n_tiles * S;
        const double rounds = (double)((int64_t)((w + slots - 1) / slots));
        double score = (w / (rounds * slots)) * (k / (k + overhead_steps));
        if (S > 1) score *= 0.93;                      // slab write + read + finish launch
        if (score > best_score + 1e-9) { best_score = score; best = S; }
    }
    return best;
}

static int tile_pt(int P) {
    int pt = 1;
    while (pt * 2 <= P && pt * 2 <= 32) pt *= 2;          // largest power of two <= min(P, 32)
    return pt;
}

// Position slots of a FORWARD tile.  Default: the largest power of two <= min(P, 32).  Where a sizeable share of the output
// positions has a tap that reads only zero padding -- TF SAME puts the odd padding element behind the data, so with stride 2
// that is the LAST output coordinate along the conv axis (tap 2), and for the stride-1 layer on two frames each of the two
// frames has its own dead tap -- the tile takes positions of ONE class (PT divides both class sizes; along T the classes
// are made contiguous by tile_pos(), perm 2) and the kernel's tile-wide dead-tap skip drops that tap's K-steps.
// Taken only when it saves >= 3 % of the launch's MACs and does not cost the launch its register-resident statistics
// (4 or 8 samples per position).  At the 1-s input and B = 640: conv8 -1/3, conv6 -1/6, conv13 -1/6, convs 4 / 11 -1/12,
// conv2 -1/24 of their K-steps.  NAFP_TAPCLASS=0 switches it off.
struct FwdTile { int pt, perm; double saved; };
static FwdTile fwd_tile(const ConvGeom& g, int BM, const ConvKnobs& knobs) {
    const int P = g.Fout * g.Tout;
    FwdTile r{tile_pt(P), 0, 0.0};
    const int L = g.axis == 0 ? g.Tout : g.Fout, n_in = g.axis == 0 ? g.Tin : g.Fin;
    if (!knobs.tapclass || L < 2) return r;
    auto mask = [&](int o) { unsigned m = 0; for (int t = 0; t < 3; ++t) { const int i = o * g.stride - g.pad + t; if (i >= 0 && i < n_in) m |= 1u << t; } return m; };
    unsigned m0 = 0;
    for (int o = 0; o + 1 < L; ++o) m0 |= mask(o);
    const unsigned m1 = mask(L - 1);
    const int n_all = __builtin_popcount(m0 | m1), n0 = __builtin_popcount(m0), n1 = __builtin_popcount(m1);
    const int64_t c1 = P / L, c0 = (int64_t)c1 * (L - 1);                 // positions per class
    const double saved = n_all == 0 ? 0.0 : (double)(c0 * (n_all - n0) + c1 * (n_all - n1)) / ((double)P * n_all);
    if (saved < 0.03) return r;
    int pt = 1;
    while (pt * 2 <= 32 && c0 % (pt * 2) == 0 && c1 % (pt * 2) == 0) pt *= 2;
    const int st = BM / pt, st_def = BM / r.pt;
    const bool fast = st == 4 || st == 8, fast_def = st_def == 4 || st_def == 8;
    if (st < 4 || (fast_def && !fast)) return r;
    r.pt = pt; r.perm = g.axis == 0 ? 2 : 0; r.saved = saved;
    return r;
}

// Position slots of a DGRAD tile (rows = input positions of the conv).  With stride 2 the positions are enumerated parity
// class by parity class (tile_pos(), perm 1: one class receives taps {0, 2}, the other only tap {1}) so that a tile of ONE
// class skips the structurally zero taps; that needs PT to divide both class sizes.  The default (largest power of two
// <= min(P, 32)) straddles the classes whenever a class has fewer than 32 positions -- the transposed convs of layers 9,
// 10, 11, 13, 15 at the 1-s input then multiplied all three taps, twice the needed K-steps (BSZ 5120: dgrad_9 72
// TFLOP/s of useful work, dgrad_13 59).  Any samples-per-position count works for the PLAIN epilogue.
static int dgrad_tile_pt(const ConvGeom& g) {
    const int P = g.Fin * g.Tin;
    int pt = tile_pt(P);
    const int L = g.axis == 0 ? g.Tin : g.Fin;
    if (g.stride == 1 && g.axis == 0 && L == 2 && g.pad == 1) {        // two frames, each with its own dead tap (perm 2)
        while (pt > 1 && (P / 2) % pt != 0) pt >>= 1;
        return pt;
    }
    if (g.stride != 2 || L < 2) return pt;
    const int c0 = g.pad & 1, n0 = (L - c0 + 1) / 2;
    const int per = P / L;                                  // positions per coordinate value along the tap axis
    const int s0 = per * n0, s1 = per * (L - n0);
    while (pt > 1 && (s0 % pt != 0 || s1 % pt != 0)) pt >>= 1;
    return pt;
}

// Tile height of a launch: 256 rows (8 waves, 2 workgroups per CU) when the launch has enough 128-row tiles to fill the
// chip several times over with the larger tile as well -- those launches are never split along K; 128 rows otherwise.
// NAFP_BM256 = minimum number of 128-row tiles (0 = never; default 2000).  Measured at B = 640, same box, ms per launch
// for convs 1-5 with thresholds 0 / 2000 / 1000: 1.185 0.605 0.316 0.315 0.289 / 1.160 0.591 0.306 0.306 0.293 /
// 1.166 0.592 0.307 0.306 0.334 -- conv5 has 1280 tiles of 128 rows = 640 of 256: 1.25 rounds of 512 slots.
static int pick_bm(int64_t B, int P, int Cout, const ConvKnobs& knobs) {
    if (knobs.bm256_min_tiles <= 0) return 128;
    const int pt = tile_pt(P), ST = 128 / pt;
    const int64_t n_tiles = ((B + ST - 1) / ST) * ((P + pt - 1) / pt) * (Cout / BN);
    return n_tiles >= knobs.bm256_min_tiles ? 256 : 128;
}

// Tile width of a launch that runs 128-row tiles: 64 columns (4 workgroups per CU, each half the work) where the
// 128 x 128 tiling gives few, coarse workgroups.  NAFP_BN64: 0 never, 2 whenever Cout allows, 1 (default) by tile count.
// (Diagnostic override for tile-plan sweeps: NAFP_FWD_PLAN / NAFP_DGRAD_PLAN = "bn:S" force the column width and split factor of
// every forward FULL / transposed launch on 128-row tiles, where legal; tools/plan_sweep.sh and dgrad_plan_sweep.sh run the
// combinations and print per-conv times.)
static int pick_bn(int64_t n_tiles128, int Cout, const ConvKnobs& knobs) {
    if (knobs.bn64 == 0 || Cout % 64 != 0) return 128;
    if (knobs.bn64 == 2) return 64;
    // plan sweep at B = 640 (tools/plan_sweep.sh): with <= 160 tiles of 128 x 128 (convs 9-15) the 128-column tile with a
    // split-K of 3-6 beats the 64-column tile by 8-10 %; with 320-640 tiles (convs 6-8) the 64-column tile wins or ties
    return (n_tiles128 < knobs.bn64_tiles && n_tiles128 >= knobs.bn64_min) ? 64 : 128;
}

// Tile of a FORWARD launch: rows x position slots x class order.
struct FwdPlan { int BM, pt, perm; };
static FwdPlan fwd_plan(int64_t B, const ConvGeom& g, bool full_epilogue, bool fuse0, bool force128, const ConvKnobs& knobs) {
    const int P = g.Fout * g.Tout;
    FwdPlan r{(fuse0 || force128) ? 128 : pick_bm(B, P, g.Cout, knobs), tile_pt(P), 0};
    if (r.BM == 256 && full_epilogue && 256 / r.pt != 8) r.BM = 128;      // FULL mode on 256 rows keeps its statistics in registers: 8 samples per position
    if (full_epilogue && !fuse0) {
        FwdTile ft = fwd_tile(g, r.BM, knobs);
        if (r.BM == 256 && ft.saved == 0.0) {
            // the 256-row tile cannot hold one class with 8 samples per position (conv8 at large batches: 16 positions
            // per class), the 128-row tile can: a third of the K-steps outweighs the larger tile's few per cent
            const FwdTile f2 = fwd_tile(g, 128, knobs);
            if (f2.saved >= 0.10) { r.BM = 128; ft = f2; }
        }
        r.pt = ft.pt; r.perm = ft.perm;
    }
    return r;
}

static int find_kernel(int BM, int bn, int ring, int epi, int arith, bool fuse0) {      // ring 0: whatever the row has
    for (int i = 0; i < conv_kernel_row_count; ++i) {
        const ConvKernelRow& r = conv_kernel_rows[i];
        if (r.BM == BM && r.bn == bn && (ring == 0 || r.ring == ring) && r.epi == epi && r.arith == arith && r.fuse0 == fuse0) return i;
    }
    return -1;
}

ConvPlan plan_conv_gemm(const ConvPlanIn& in, const ConvGeom& g, const ConvKnobs& knobs) {
    ConvPlan pl{};
    pl.rc = NAFP_ERR_UNSUPPORTED;
    const int64_t B = in.B;
    const bool full = !in.plain && !in.dgrad;
    if (g.Cin % 32 != 0 || g.Cout % BN != 0 || B > (1 << 24)) return pl;      // (Cout >= 128 also is what splitk_finish_kernel needs: a wave, 256 floats, spans <= 2 rows)
    // backward w.r.t. the conv input: rows = input positions, source = dT (B,Fout,Tout,Cout), weights = wp flipped to (Cin, 3*Cout); see row_geom()
    if (in.dgrad && (!in.plain || g.Cout % 32 != 0 || g.Cin % BN != 0 || (g.stride != 1 && g.stride != 2))) return pl;
    // the GEMM's own view: P rows per sample and N columns, of the conv's output -- of its INPUT for the transposed conv
    const int P = in.dgrad ? g.Fin * g.Tin : g.Fout * g.Tout, N = in.dgrad ? g.Cin : g.Cout;
    const int64_t sample_in = in.dgrad ? (int64_t)g.Fout * g.Tout * g.Cout : (int64_t)g.Fin * g.Tin * g.Cin;
    // (plan_b: the inference forward plans as if the launch held plan_b segments -- see fwd_plan_b())
    const int64_t Bp = (in.plan_b > 0 && full && !in.fuse0) ? in.plan_b : B;
    // the exact-split kernels, bf16x3 == 2, run best on 128-row tiles at three workgroups per CU (measured in profiles/r05_experiments.md);
    // a transposed conv on the exact split (x6d): 128-row tiles as well
    const bool x6 = in.bf16x3 == 2 && full && in.split_weights, x6d = in.bf16x3 == 2 && in.plain && in.dgrad && in.split_weights;
    pl.P = P;
    if (in.dgrad) {
        pl.BM = x6d ? 128 : pick_bm(B, P, N, knobs);
        pl.PT = dgrad_tile_pt(g);
        pl.k_steps = dgrad_k_steps(g);
        const int L = g.axis == 0 ? g.Tin : g.Fin;             // extent of the rows along the tap axis
        if (g.stride == 2 && L >= 2) {
            pl.perm_on = 1; pl.perm_c0 = g.pad & 1;            // class 0: coordinate + pad even -> taps {0, 2}
            pl.perm_n0 = (L - pl.perm_c0 + 1) / 2;
        } else if (g.stride == 1 && g.axis == 0 && L == 2 && g.pad == 1) {
            // stride 1 on two frames (conv8 at the 1-s input): input frame 0 receives taps {0, 1}, frame 1 taps {1, 2}: the
            // forward class order (last frame of every line last) separates them
            pl.perm_on = 2;
        }
    } else {
        const FwdPlan fp = fwd_plan(Bp, g, full, in.fuse0, x6, knobs);
        pl.BM = fp.BM; pl.PT = fp.pt; pl.perm_on = fp.perm;
        pl.k_steps = live_k_steps(g);
    }
    const int BM = pl.BM, ST = pl.ST = BM / pl.PT;
    pl.n_sg = (int)((B + ST - 1) / ST);
    const int n_pb = pl.n_pb = (P + pl.PT - 1) / pl.PT;
    // per-tile A descriptor covers ST samples: must stay below the 2 GiB OOB marker
    if ((int64_t)ST * sample_in * 4 >= ((int64_t)1 << 31)) return pl;
    const int64_t wbytes = (int64_t)g.Cout * 3 * g.Cin * 4;
    if (wbytes >= ((int64_t)1 << 31)) return pl;
    pl.wp_bytes = (unsigned)wbytes;
    pl.abl = in.plain ? 0 : knobs.abl;
    pl.opt = knobs.gemm_prio;

    // columns and split factor, decided at the planning batch
    const int64_t n_tiles128 = (int64_t)pl.n_sg * n_pb * (N / BN);
    const int64_t n_tiles128_plan = ((Bp + ST - 1) / ST) * n_pb * (N / BN);
    int bn = (BM == 256 || in.fuse0) ? 128 : pick_bn(n_tiles128_plan, N, knobs);
    const PlanOverride ov = (full && !in.fuse0) ? knobs.fwd_plan : in.dgrad ? knobs.dgrad_plan : PlanOverride{};
    const bool forced = BM == 128 && ov.bn > 0 && !in.sizing;
    if (forced && (ov.bn == 128 || N % 64 == 0)) bn = ov.bn;
    const int64_t n_tiles = n_tiles128 * (BN / bn), n_tiles_plan = n_tiles128_plan * (BN / bn);
    const int64_t out_floats = B * P * N;
    int S = 1;
    if (in.slab_floats > 0 && !in.fuse0 && BM == 128) {
        S = choose_split(n_tiles_plan, pl.k_steps, Bp * P * N, bn == 64 ? ((knobs.n64_two_stage && !in.plain) ? 1280.0 : 1024.0) : 768.0, knobs);
        if (forced && ov.S > 0) { S = ov.S; while (S > 1 && pl.k_steps / S < 4) --S; }
        // (the sizing has always kept the policy's column width under an override and taken the larger of the two split factors)
        if (in.sizing && ov.S > 0) S = std::max(S, ov.S);
        if (S * out_floats > in.slab_floats) S = 1;
        if (x6 && bn == 64 && S == 2 && (ST == 4 || ST == 8)) S = 1;      // convs 7, 9 at B = 640: unsplit on the bf16 pipe beats the two f32 parts + finish (only where the unsplit launch IS a split-arithmetic one: register-resident statistics)
    }
    pl.bn = bn; pl.S = S;
    pl.mode = in.plain ? 1 : S > 1 ? 2 : 0;

    // which finish a split launch takes
    // FULL split launches on 64-column tiles finish in-kernel (last-arriver) when the caller provides arrival counters
    // (measured per conv at B = 640: with >= 320 output tiles the last arrivers finish faster than a second launch --
    // conv7 0.119 -> 0.104 ms, conv9 0.193 -> 0.178 --, with 160 or fewer the finish kernel's finer split wins by 2-8 %)
    // (decided at the planning batch like S itself: the two finishes group a sample's statistics into different partial sums)
    // (round-5 ADVICE: the launch's own tile count used to decide as well -- above ~4096 segments convs 7 and 9 fell back to the finish
    // kernel and a fingerprint's last bits depended on the launch size again; now a launch with more tiles than arrival counters runs as
    // several launches over sample ranges, see below)
    const bool in_kernel_finish = knobs.split_inkernel > 0 && S > 1 && !in.plain && bn == 64 && in.tickets && n_tiles_plan >= knobs.split_inkernel &&
                                  (int64_t)n_pb * (N / bn) <= NAFP_TICKET_SLOTS;
    // PLAIN split launches (the transposed convs) with arrival counters: the last arriver adds the parts and stores the result
    // (its epilogue is a sum: nothing like the FULL epilogue's serial tail) -- NAFP_PLAIN_INKERNEL=0 restores slab + plain_finish_kernel
    const bool plain_in_kernel = knobs.plain_inkernel > 0 && S > 1 && in.plain && in.tickets && n_tiles <= NAFP_TICKET_SLOTS && !x6d;      // (the exact-split parts finish through plain_finish_kernel)
    pl.finish = S == 1 ? CONV_FINISH_NONE : in_kernel_finish ? CONV_FINISH_IN_KERNEL_FULL : plain_in_kernel ? CONV_FINISH_IN_KERNEL_PLAIN : CONV_FINISH_KERNEL;
    if (pl.finish == CONV_FINISH_KERNEL && in.plain) {
        pl.finish_grid = (unsigned)std::min<int64_t>((out_floats / 4 + 255) / 256, 8192);
    } else if (pl.finish == CONV_FINISH_KERNEL) {
        // the finish kernel's block size follows the planning batch (it sets the partial sums of the statistics); it wants >= 1024 workgroups
        const int64_t f4_plan = Bp * P * N / 4;
        pl.finish_f4 = f4_plan >= 1024 * 1024 ? 1024 : f4_plan >= 1024 * 512 ? 512 : 256;
        pl.finish_grid = (unsigned)((out_floats / 4 + pl.finish_f4 - 1) / pl.finish_f4);
    }

    // the grid and its mapping
    // NAFP_XCDMAP: 0 = the plain 3-D grids, 1 (default) = 1-D grid in XCD-aware order, the operand to keep inside one L2 chosen
    // by size (column-fastest unless the live weights outweigh the activations read), 2 / 3 = force column- / row-fastest
    const int n_col = N / bn;
    pl.xcd_group = 1;
    while ((1 << pl.log2_ncol) < n_col) ++pl.log2_ncol;
    const int64_t total_wg = (int64_t)pl.n_sg * n_pb * n_col * S;
    // (launches that finish their split-K in-kernel keep the plain grid: measured at B = 640 the map costs convs 7 and 9 5 us each)
    bool xm = knobs.xcdmap != 0 && !in.fuse0 && !in_kernel_finish && !plain_in_kernel && (1 << pl.log2_ncol) == n_col && total_wg < ((int64_t)1 << 31);
    if (xm) {
        const double a_bytes = (double)B * (double)sample_in * 4.0, w_bytes = (double)pl.k_steps * 16.0 * N * 4.0;
        const bool row_fast = knobs.xcdmap == 3 || (knobs.xcdmap == 1 && w_bytes > a_bytes);
        pl.xcd_group = row_fast ? pl.n_sg * n_pb : n_col * S;
        pl.xcd_full = (int)(total_wg / (8 * (int64_t)pl.xcd_group) * (8 * (int64_t)pl.xcd_group));
        if (pl.xcd_group <= 1 || pl.xcd_full == 0) xm = false;              // one item per group: the plain order already is this order
        else pl.opt |= row_fast ? (8 | 16) : 8;
    }
    const bool g3 = !xm && S == 1 && knobs.grid3d != 0 && (knobs.grid3d == 1 || BM == 256 || bn == 128);
    if (g3) pl.opt |= 4;
    pl.grid = xm ? dim3((unsigned)total_wg)
            : g3 ? dim3((unsigned)pl.n_sg, (unsigned)n_pb, (unsigned)n_col)
                 : dim3((unsigned)((int64_t)pl.n_sg * n_pb), (unsigned)n_col, (unsigned)S);
    if (!xm && (n_pb > 65535 || n_col > 65535)) return pl;
    // more output tiles than arrival counters: sample ranges of at most NAFP_TICKET_SLOTS tiles, one launch each (the last arrivers
    // leave the counters at zero, so the ranges reuse them and the slab in stream order); every sample sees exactly the launch it
    // would have seen in a smaller batch
    if (in_kernel_finish && n_tiles > NAFP_TICKET_SLOTS) pl.range_step = NAFP_TICKET_SLOTS / ((int64_t)n_pb * n_col) * ST;

    // the kernel
    const bool fast_st = ST == 4 || ST == 8;                // statistics in registers
    int epi, arith = 0;
    if (in.fuse0) {
        // conv0 generated in-kernel: this conv must be the 3x1 conv that consumes conv0's output; the fused kernel carries the inference epilogue only
        const ConvGeom* f0 = in.f0_geom;
        if (in.plain || S != 1 || !f0 || g.axis != 1 || f0->Cout != g.Cin || f0->Tout != g.Tin || f0->Fin != g.Fin || g.Cin % 16 != 0 ||
            in.v_out || !fast_st)
            return pl;
        epi = 0;
        if (in.bf16x3 == 2 && in.split_weights) {
            if (g.Cin != 128) return pl;                     // the exact-split generator is written for conv0's 128 channels
            arith = 2;
        }
    } else {
        epi = plain_in_kernel ? 5 : in_kernel_finish ? 4 : pl.mode != 0 ? 3 : !fast_st ? 2 : in.v_out ? 1 : 0;
    }
    const bool two_stage = knobs.n64_two_stage && bn == 64 && (epi == 0 || epi == 1 || epi == 4);
    if (!in.fuse0) {
        // which launches leave the f32 pipe.  The bf16 kernels on 64 columns carrying the inference / training epilogue exist on the 2-stage
        // ring only; the exact split also has the generic-statistics epilogue (samples per position other than 4 / 8: the small late layers of a
        // large training batch; NAFP_X6_ANY) and the split-K parts of 128-column tiles; launches that finish in-kernel stay on the f32 kernels
        const bool ring_ok = bn == 128 || two_stage;
        if (x6) arith = (epi <= 1 ? ring_ok : epi == 2 ? knobs.x6_any : epi == 3 ? bn == 128 : false) ? 2 : 0;
        if (x6d && epi == 3) arith = 2;
        if (!arith && in.bf16x3 && epi == 0 && ring_ok) arith = 1;
    }
    pl.kernel = find_kernel(BM, bn, arith ? 0 : two_stage ? 2 : 3, epi, arith, in.fuse0);
    if (pl.kernel < 0) return pl;
    const ConvKernelRow& row = conv_kernel_rows[pl.kernel];
    pl.lds_bytes = (row.ring * ((BM + bn) * 16 + row.extra_stage_floats) + 2 * BM + 96 + (in.fuse0 ? 4 * g.Cin : 0)) * (int)sizeof(float) + knobs.lds_pad;
    pl.rc = NAFP_OK;
    return pl;
}

// Workspace the split-K policy wants: the planner's split factor with the slab unlimited, for the forward FULL launch (planned at
// plan_b when given) and, with_dgrad, for the transposed conv.  What the sizing has never known, and still does not (a larger slab
// would change which launches split): the arithmetic.  It asks for f32 launches, so under bf16x3 == 2 -- which forces 128-row tiles
// on forward and transposed convs -- a layer whose f32 plan runs 256-row tiles gets no slab and its exact-split launch stays unsplit.
// Under NAFP_FWD_PLAN / NAFP_DGRAD_PLAN it takes the policy's column width and the larger of the two split factors (ConvPlanIn::sizing).
int64_t conv_gemm_slab_floats(int64_t B, const ConvGeom& g, bool with_dgrad, int64_t plan_b) {
    ConvPlanIn in{};
    in.B = B; in.plan_b = plan_b; in.slab_floats = INT64_MAX; in.sizing = true;
    const ConvPlan fwd = plan_conv_gemm(in, g, conv_knobs());
    int64_t need = fwd.rc == NAFP_OK && fwd.S > 1 ? (int64_t)fwd.S * B * fwd.P * g.Cout : 0;
    if (with_dgrad) {
        in.plan_b = 0; in.plain = in.dgrad = true;
        const ConvPlan d = plan_conv_gemm(in, g, conv_knobs());
        if (d.rc == NAFP_OK && d.S > 1) need = std::max(need, (int64_t)d.S * B * d.P * g.Cin);
    }
    return need;
}

}  // namespace nafp
