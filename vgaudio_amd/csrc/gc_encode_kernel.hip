// gc_encode_kernel.hip -- GC-ADPCM frame encoder for gfx950 (the headline kernel).
//
// Replaces VGAudio/Codecs/GcAdpcm/GcAdpcmEncoder.cs:14-171 (Encode, DspEncodeFrame,
// DspEncodeCoef), bit-exact.
//
// ADPCM is a serial recurrence inside a channel (the reconstructed samples 12,13 of frame
// k are the history of frame k+1, :40-41; sample s+1 needs reconstructed sample s, :138,160),
// so time = frames x (wave-instructions per frame): the kernel is bound by VALU issue (one
// instruction per 4 cycles per SIMD for this mix; LABNOTES.md 4.0), not by HBM.
//
//  * lane = (channel, predictor, scale candidate): 16 lanes per channel, 4 channels per
//    encoder wave; a helper wave per workgroup prepares 16-frame tiles in LDS (below).
//  * Speculation on the retry loop (:127-170): the reference's first quantise pass is one
//    scale too small 93 % of the time and exactly right 6 %, so candidate A runs the pass
//    at scale s1 and candidate B at s1+1 IN PARALLEL LANES; two compares on the exchanged
//    overflow values decide which one the reference ends on.  Third trips, overflow bumps
//    and everything else that is rare sit behind ONE wave-uniform branch per frame.
//  * The quantise pass is integer-only on a packed pair of 16-bit history values (12 VALU ops per sample
//    instead of the float/double detour); exactness conditions in gc_encode_core.hpp S2/S3, P1-P6.  Since round 10 the
//    piece kernels run it on numbers moved up by 2^30 (pass_fast_core_b, B1-B5): the rounding sign is the subtract's
//    borrow, one op a sample less; the seam, tail and chain code keeps pass_fast_core_t.
//  * 8-predictor argmin + winner-history broadcast: v_min_u32 / v_or_b32 with DPP operands
//    (quad_perm, row_half_mirror, row_mirror) -- 8 VALU ops, no LDS.
#include "common.hpp"
#include "gc_encode_core.hpp"
#include "gcadpcm_kernels.hpp"
#include "seams.hpp"
#include "gc_plan8.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace vga {
namespace gc {

constexpr int DPP_QUAD_XOR1 = 0xB1;         // quad_perm [1,0,3,2]
constexpr int DPP_QUAD_XOR2 = 0x4E;         // quad_perm [2,3,0,1]
constexpr int DPP_ROW_HALF_MIRROR = 0x141;  // i <-> 7-i inside each 8 lanes
constexpr int DPP_ROW_MIRROR = 0x140;       // i <-> 15-i inside each 16 lanes

template <int CTRL>
__device__ __forceinline__ int dpp(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}

__device__ __forceinline__ unsigned umin32(unsigned a, unsigned b) { return a < b ? a : b; }

// all-reduce over each 16-lane row
template <class Op>
__device__ __forceinline__ unsigned row16_reduce(unsigned v, Op op)
{
    v = op(v, (unsigned)dpp<DPP_QUAD_XOR1>((int)v));
    v = op(v, (unsigned)dpp<DPP_QUAD_XOR2>((int)v));
    v = op(v, (unsigned)dpp<DPP_ROW_HALF_MIRROR>((int)v));
    v = op(v, (unsigned)dpp<DPP_ROW_MIRROR>((int)v));
    return v;
}


// =====================================================================================================
// gc_encode_kernel -- SW encoder (serial) waves + one helper wave per workgroup (4 channels per encoder wave).
// Everything that does not depend on the reconstructed history is taken off the serial wave:
//   helper wave (wave 1), one 16-frame tile AHEAD of the encoder:
//     * coalesced global loads of the tile (lane = frame j of channel g: 28 contiguous bytes),
//     * unpack to int32, x*2048 + 1024 + 2^30 (pass_b_row), and for each of the 8 predictors the max/min pre-scan distance over the
//       twelve samples s = 2..13 that involve input samples only (GcAdpcmEncoder.cs:107-115),
//     * all of it into LDS (double-buffered), plus the coalesced flush of the previous tile's frames
//       (the zero-padded partial last frame travels through the same path);
//   serial wave (wave 0): per frame 7 LDS reads, the two history-dependent pre-scan distances, the
//     speculative quantise pass, candidate resolution, DPP argmin, one LDS write.
// The hot loop is ONE copy of the frame body (a few KB of code): the reference's third-and-later
// quantise passes re-enter the same pass code through a wave-uniform loop, and the never-on-audio
// fallbacks (literal f32/f64 pass, sequential pre-scan tie-break) are out-of-line functions.  Measured:
// compiling the rare paths inline cost 80 ms of 257 ms (code size, register pressure, branches).
// The SIMDs have idle issue slots next to a lone latency-bound wave (tools/ubench_valu.hip: two waves
// per SIMD do not slow each other's dependent chains), so the helper costs the encoder nothing.
// measured at configs[1]: 1 encoder wave -> 209.5 ms, 2 -> 200.1 ms (two pieces per channel)
#ifdef VGA_DEBUG_TIMESTAMPS
// tools/time_wave_ends.py (a -DVGA_DEBUG_TIMESTAMPS build under tools/variants/ only): when every workgroup's encoder wave
// 0 started and ended, in ticks of the 100 MHz wall clock
__device__ unsigned long long g_vga_enc_ts[1 << 16];
extern "C" int vga_debug_encode_timestamps(unsigned long long *out, int n)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_vga_enc_ts), (size_t)n * sizeof(unsigned long long));
}
#endif
// Diagnostics of the data-dependent parts (vga_testing_gc_encode_stats, include/vgaudio_hip_testing.h; bench.py's
// signal_sensitivity block): counted with a handful of atomics per piece and per seam -- nothing in the frame loop but one
// scalar add inside the cold block.  Summed over every launch of the process since the last reset.
//   [0] seams closed inside their piece   [1] seams left open for gc_encode_chain_kernel   [2] frames re-encoded by seam runs
//   [3] wave-frames encoded by the piece kernels   [4] ... of which took the cold block (third trips, bump loop, inexact sums;
//   counted by -DVGA_GC_STATS builds only -- tools/build_variants.sh stats:"-DVGA_GC_STATS" -- 0 otherwise, [7] says which)
//   [5] channels gc_encode_chain_kernel had to walk   [6] pieces encoded   [7] 1 = this build counts [4]
//   [8] (vga_testing_gc_encode_stats_n only) channels with an open seam whose chain the self-served kernel walked itself (round
//   15, the hand-over below): what [5] counts when the hand-over is switched off
constexpr int GC_STATS = 9;
__device__ unsigned long long g_vga_gc_stats[GC_STATS];
extern "C" int vga_testing_gc_encode_stats_n(unsigned long long *out, int n, int reset)
{
    if (n < 0 || n > GC_STATS) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (out && n > 0 && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_vga_gc_stats), (size_t)n * sizeof(unsigned long long)) != hipSuccess) return -1;
#ifdef VGA_GC_STATS
    if (out && n > 7) out[7] = 1;
#else
    if (out && n > 7) out[7] = 0;
#endif
    if (reset) {
        const unsigned long long zero[GC_STATS] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_vga_gc_stats), zero, sizeof zero) != hipSuccess) return -1;
    }
    return 0;
}
extern "C" int vga_testing_gc_encode_stats(unsigned long long *out8, int reset) { return vga_testing_gc_encode_stats_n(out8, 8, reset); }
constexpr int SW = 2;              // encoder (serial) waves per workgroup; one helper wave serves them all
constexpr int ENC_THREADS = 64 * (SW + 1);
// issue priorities (s_setprio) of the encoder waves and of the helper wave.  Round 6 (profiles/r06_t_encode_priority*.log):
// helper at 1 or 2, or at priorities that differ between the helpers of a SIMD (by wave slot, rotating per piece or per
// tile): 143.7-144.9 ms against 144.0-144.4; helper at 3: 148.5; encoder waves below the helper: 150 ms.
#ifndef VGA_GC_ENCODER_PRIO
#define VGA_GC_ENCODER_PRIO 3
#endif
#ifndef VGA_GC_HELPER_PRIO
#define VGA_GC_HELPER_PRIO 0
#endif
// waves per SIMD gc_encode_persistent_kernel is compiled for (tools/build_variants.sh: 4,4 is the 128-VGPR build of round 12,
// measured and not kept: see persistent_wgs_per_cu)
#ifndef VGA_GC_PERSISTENT_WAVES_PER_EU
#define VGA_GC_PERSISTENT_WAVES_PER_EU 3, 3
#endif
// Two lane layouts of the encoder wave (template parameter CPW = channels per encoder wave):
//   CPW = 4: lane = (channel, predictor, scale candidate A/B) -- the candidates of the retry loop run side by side;
//   CPW = 8: lane = (channel, predictor) -- candidate B (s1 + 1) and candidate A (s1) run one after the other in the
//            same lane.  Twice the channels share every per-frame fixed cost (row reads, pre-scan, resolution,
//            argmin, the cold block's pass), which is worth more than the second pass costs: LABNOTES.md 4.1.
// Round 13, SELF (CPW = 8 only): the self-served shape -- a workgroup is ONE wave that is encoder and helper of its eight
// channel slots in turn: helper role lane = (slot = lane >> 3, frame = lane & 7), encoder role (slot = lane >> 3, predictor =
// lane & 7); one tile buffer, no workgroup barrier, no issue priority.  All waves of a SIMD are then alike (three at 168
// VGPRs, by counting: twelve workgroups per CU), and each has its tile boundary's work to issue where the others' chains wait.
template <int CPW, bool SELF = false>
struct Lay {
    static_assert(!SELF || CPW == 8, "the self-served shape is the (channel, predictor) layout");
    static constexpr int EW = SELF ? 1 : SW;   // encoder waves per workgroup
    static constexpr int CS = CPW * EW;    // channel slots per workgroup
    static constexpr int TF = 64 / CS;     // frames per tile: one helper lane per (channel slot, frame)
    static constexpr int THREADS = SELF ? 64 : ENC_THREADS;
    static constexpr int BUFS = SELF ? 1 : 2;  // tile buffers: the wave that fills the one of SELF is the wave that drains it
};
// Round 12: everything a (channel slot, frame) owns in LDS -- the helper's row, its pre-scan words and the winner's record --
// is ONE 192-byte slot, so that an encoder lane reaches all of it from one address register with immediate offsets (the
// four arrays of before cost four address registers, which a 128-VGPR frame loop spilled).  A channel slot's frames are
// padded by 16 bytes: the eight channel slots of an encoder wave then read their 16-byte pieces from disjoint LDS banks.
template <int CS, int TF>
struct GcTileT {
    struct Slot {
        uint32_t xw[8];        // the frame as packed pairs (in[2i], in[2i + 1]), 7 used (round 8)
        int in2048p[16];       // x * 2048 + 1024 + 2^30: the row of pass_fast_core_b (round 10, gc_encode_core.hpp B1)
        uint32_t pre[8];       // per predictor: clamp16(max d) & 0xFFFF | clamp16(min d) << 16, over s = 2..13
        int4 out[4];           // the winner's frame, unpacked: q[0..13], predictor, scale; the helper packs it when it flushes
    };
    struct Group { Slot f[TF]; uint32_t pad[4]; };
    Group g[CS];               // [channel slot][frame]
};
typedef short short2v __attribute__((ext_vector_type(2)));
struct XW7 { uint32_t v[7]; };

// inline: measured 267 ms out of line vs 260 ms inline at configs[1] (round 1)
#define VGA_COLD __device__ __forceinline__

// Rare +M/-M tie of the pre-scan (argument by value: the hot copy of the frame stays in registers).
VGA_COLD int prescan_sequential_cold(XW7 xs, uint32_t hist, int c0, int c1)
{
    int x[16];
    unpack_row(xs.v, hist, x);
    return prescan_sequential(x, c0, c1);
}

#ifdef VGA_GC_R05_COLD
#define VGA_COLD_OPAQUE(v) ((void)0)
#else
#define VGA_COLD_OPAQUE(v) VGA_OPAQUE(v)
#endif
// Third and later trips / the generic redo for one frame.  Its mere presence in the frame loop costs the hot
// path (a build with the block compiled in but never run: 172 ms vs 140 ms without it), which is why the
// frame's tail is instantiated once per branch below instead of merging the two branches' results.
struct ColdState {
    uint32_t xw[7];            // the frame as packed pairs; the paths that want ints unpack it where they run
    int mp[14];                // the row moved up by 2^30 (pass_b_row)
    uint32_t hist;             // (x[0], x[1]) packed
    int c0, c1, s1;
    // what this lane needs (any of them in any lane sends the wave here):
    //   generic: the reference's loop as written from `start` (the scalePower its loop continues from): the bump loop
    //            (:166-168) was entered, or the coefficients can wrap int32
    //   drop:    (lane-per-candidate layout) the pair's other lane redoes the whole loop: this lane is out
    //   wide:    the final pass ran at the cap with an overflow above 3 (until round 8 its 32-bit error sum could have wrapped
    //            and the pass ran again at once; the sum in pairs cannot wrap and the exact-sum rule below covers the lane)
    //   resume:  third and later trips
    // start: -100 = not known yet: the loop stands behind the bumps of the pass that started them (bump_a: the pass at s1
    // with overflow ov_a, else the pass at s1 + 1 with ov_b) -- worked out only by a lane that goes that way (round 6: the
    // bump loops ran, under an empty exec mask as a rule, on every visit of the cold block)
    int generic, start, drop, wide, resume;
    int bump_a, ov_a, ov_b;
};
// sum_exact: r.total came from the reference's loop as written (exact whatever its size); 0: from a fast pass at final_sp,
// exact below 2^28 and "at least 2^28" otherwise (gc_encode_core.hpp E3)
struct ColdOut { PassOutB r; int final_sp; int fin; int sum_exact; };
// inline: 370 ms out of line (the by-value state goes through scratch) vs 209 inline (round 1)
__device__ __forceinline__
ColdOut encode_frame_cold(ColdState st, PassOutB r, int final_sp, int fin)
{
    uint32_t xw[7];
    int mp[14];
#pragma unroll
    for (int i = 0; i < 7; i++) xw[i] = st.xw[i];
#pragma unroll
    for (int i = 0; i < 14; i++) mp[i] = st.mp[i];
    int sum_exact = 0;
    if (st.drop) fin = 0;
    if (__any(st.generic != 0)) {                  // hostile input, and tones the first scale misjudges by 2^5 and more
        if (st.generic) {
            // (the frame is made opaque here: hipcc otherwise hoists the literal pass's set-up -- fourteen shifts, 64-bit
            // mads -- out of this branch into every visit of the cold block)
            int xg[16];
            unpack_row(xw, st.hist, xg);
#pragma unroll
            for (int i = 0; i < 16; i++) VGA_COLD_OPAQUE(xg[i]);
            const int start = st.start != -100 ? st.start
                                               : (st.bump_a ? apply_bumps(st.s1, st.ov_a) : apply_bumps(st.s1 + 1, st.ov_b));
            r = as_pass_b(resume_passes(xg, st.c0, st.c1, start, final_sp));
            fin = 1;
            sum_exact = 1;
        }
    }
    // Round 5: until then any lane whose pass at the cap overflowed by more than 3 sent the whole wave through the
    // reference's loop from its start (three to four passes, the literal f32 / f64 one among them) -- 96 % of the wave-frames of
    // full-scale white noise and of a clipped square (bench.py signal_sensitivity: 316 and 343 ms against 146).  The pass
    // itself is right (gc_encode_core.hpp S2 holds for every int32 distance) and so is its error sum wherever the argmin
    // looks at the value (E3); a `wide` lane stays final with the sum it has, the caller applies the exact-sum rule.
    if (st.wide) fin = 1;
    if (__any(st.resume != 0)) {
        if (st.resume) {
            // third and later trips, same straight-line tests as the first trip
            int sp = st.s1 + 1;                    // < 12: neither candidate was at the cap
            for (;;) {
                sp++;
#if defined(VGA_GC_NO_FAST_PASSES) || defined(VGA_GC_NO_FAST_THIRD)  // (timing-only switches, tools/build_variants.sh)
                bool short_pass = false;
#else
                bool short_pass = !__any(sp > 9);  // (over the lanes still in this loop) without the f32 detour, as the first two passes
#endif
                if (short_pass) {
                    r = pass_fast_core_b<true>(xw, st.hist, mp, st.c0, st.c1, sp);
                    short_pass = !__any(!pass_no_round_is_exact(sp, r.max_overflow));
                }
                if (!short_pass) r = pass_fast_core_b<false>(xw, st.hist, mp, st.c0, st.c1, sp);
                const bool cap = sp >= 12;
                if ((unsigned)r.max_overflow > (cap ? 3u : 248u)) {      // bump loop / inexact sum: generic
                    int xg[16];                                          // (opaque: see above)
                    unpack_row(xw, st.hist, xg);
#pragma unroll
                    for (int i = 0; i < 16; i++) VGA_COLD_OPAQUE(xg[i]);
                    r = as_pass_b(resume_passes(xg, st.c0, st.c1, sp - 1, final_sp));
                    sum_exact = 1;
                    break;
                }
                final_sp = sp;
                if (cap || r.max_overflow <= 1) break;
            }
            fin = 1;
        }
    }
    ColdOut o;
    o.r = r;
    o.final_sp = final_sp;
    o.fin = fin;
    o.sum_exact = sum_exact;
    return o;
}

// Time segments (blockIdx.y; LABNOTES.md 4.3): with fewer channels than fill the chip, a channel's stream is cut into
// pieces of `seg_frames` frames encoded side by side.  Piece 0 starts from the caller's history, the others from a
// guess -- the two INPUT samples before the piece -- and gc_encode_seam_kernel closes the seams afterwards.
// seg_state[piece][channel] receives every piece's final history.  At BASELINE configs[1] there is one piece.
// REPAIR is a template parameter only so that the two launches carry different names in profiles (the repair launch
// normally returns at once and would halve the kernel's average duration).
// RAGGED (the `*_v` entry points): channel slots map to channels through rg.order (longest first: slot 0 of a workgroup
// holds its longest channel), every slot has its own length and offsets, a piece exists for a slot only as far as its
// channel reaches.  The workgroup runs as many tiles as its longest slot needs; a slot whose frames have run out keeps
// encoding (clamped loads, nothing flushed) with its history frozen.
// One (channel group, time piece) = what a workgroup of the plain launch does: gc_encode_kernel calls it once with its
// block indices, gc_encode_persistent_kernel once per item it takes from the queue.
template <bool REPAIR, int CPW, bool RAGGED, bool SELF = false, class P = Pieces>
__device__ __forceinline__ void gc_encode_piece(
    const int bx, const int by,
    const int16_t *__restrict__ pcm, int64_t pcm_pitch, int nch, int total_samples, const P seg,
    const int16_t *__restrict__ coefs, const int16_t *__restrict__ hist1,
    const int16_t *__restrict__ hist2, uint8_t *__restrict__ adpcm, int64_t adpcm_pitch, int16_t *__restrict__ seg_state,
    const int *__restrict__ first_open, const Ragged &rg)
{
    // Repair launch (first_open != nullptr, one workgroup row): channels with a seam that would not close are encoded
    // again, serially, from the earliest such seam among the workgroup's four channels to the end of the stream --
    // starting from seg_state of the piece before, which is the real history for all four (every seam before it
    // closed).  Workgroups without such a channel leave at once.
    constexpr bool repair = REPAIR;
    constexpr int CS = Lay<CPW, SELF>::CS, TF = Lay<CPW, SELF>::TF, BUFS = Lay<CPW, SELF>::BUFS;
    static_assert(!(SELF && REPAIR), "the repair launch keeps the 2 + 1 shape");
    using GcTile = GcTileT<CS, TF>;
    int64_t first_frame = seg.first(by);
    int repair_piece = 0;
    if (repair) {
        int k = SEAM_OPEN_LIMIT;
        for (int g = 0; g < CS; g++) {
            const int slot = bx * CS + g;
            if (slot < nch) {
                const int c = RAGGED ? rg.order[slot] : slot;
                k = first_open[c] < k ? first_open[c] : k;
            }
        }
        if (!is_open(k)) return;
        repair_piece = k;
        first_frame = seg.first(k);
    }
    // the workgroup's longest channel (slot 0 when ragged) decides whether the piece exists and how many tiles it has
    const int total_wg = RAGGED ? rg.length[rg.order[bx * CS]] : total_samples;
    if (first_frame * 14 >= total_wg) return;
    const int64_t piece_samples = repair ? (int64_t)0x7fffffff : (int64_t)seg.frames(by) * 14;
    auto piece_samples_of = [&](int total) {
        const int64_t rem = (int64_t)total - first_frame * 14;
        return (int)(rem < 0 ? 0 : (rem < piece_samples ? rem : piece_samples));
    };
    pcm += first_frame * 14;
    adpcm += first_frame * 8;
    using Slot = typename GcTile::Slot;
    static_assert(TF % 2 == 0, "the frame loop takes a tile's frames in pairs");
    // (`end`: what the row reads one frame past the last channel slot's last pair land in; see the frame loop)
    struct Tiles { GcTile t[BUFS]; Slot end; };
    __shared__ Tiles s_tiles;
    GcTile (&s_tile)[BUFS] = s_tiles.t;
    __shared__ int s_ncold[Lay<CPW, SELF>::EW];
    const int tid = threadIdx.x;
    const int wave = SELF ? 0 : tid >> 6;
    const bool helper = !SELF && wave == SW;
    const int lane = tid & 63;
    // encoder wave: CPW channels x 8 predictors (x 2 candidates when CPW = 4); helper wave: CS channel slots x TF frames
    constexpr int LPC = 64 / CPW;                          // lanes per channel: 16 or 8
    int grp = helper ? lane / TF : wave * CPW + lane / LPC;        // channel slot of this lane
    const int l16 = lane & (LPC - 1);
    const int hfr = lane % TF;                         // helper lanes: the frame inside the tile
    const int slot_raw = bx * CS + grp;
    const bool live = slot_raw < nch;
    const int slot = live ? slot_raw : nch - 1;
    const int ch = RAGGED ? rg.order[slot] : slot;
    const int16_t *src = pcm + (RAGGED ? rg.pcm_off[ch] : (int64_t)ch * pcm_pitch);
    uint8_t *dst = adpcm + (RAGGED ? rg.adpcm_off[ch] : (int64_t)ch * adpcm_pitch);

    const int sample_count = piece_samples_of(RAGGED ? rg.length[ch] : total_samples);   // this slot's share of the piece
    const int full_frames = sample_count / 14;
    const int tail = sample_count - full_frames * 14;
    const int frames = full_frames + (tail ? 1 : 0);
    const int frames_wg = RAGGED ? (piece_samples_of(total_wg) + 13) / 14 : frames;
    const int tiles = (frames_wg + TF - 1) / TF;

    // ---------------------------------------------------------------- the helper role (a wave of its own, or SELF: this wave)
    // load_frame: the lane's frame of the tile from global memory, frame index clamped: as ints and as packed pairs
    // (in[2i], in[2i+1]) -- the self-served shape keeps the pairs alone across a tile's frames and unpacks them again
    auto load_frame = [&](int tile, uint32_t (&w)[7], int (&in)[14]) __attribute__((always_inline)) {
        const int fr = RAGGED ? imax(imin(tile * TF + hfr, frames - 1), 0) : imin(tile * TF + hfr, frames - 1);
        if (fr < full_frames) {
            const uint32_t *p32 = reinterpret_cast<const uint32_t *>(src + (int64_t)fr * 14);
#pragma unroll
            for (int i = 0; i < 7; i++) w[i] = p32[i];
#pragma unroll
            for (int i = 0; i < 7; i++) {
                in[2 * i] = (int)(int16_t)(w[i] & 0xFFFF);
                in[2 * i + 1] = (int)w[i] >> 16;
            }
        } else {                                   // zero-padded partial last frame (:32-33)
#pragma unroll
            for (int s = 0; s < 14; s++) in[s] = (s < tail) ? (int)src[(int64_t)fr * 14 + s] : 0;
#pragma unroll
            for (int i = 0; i < 7; i++) w[i] = (uint32_t)(in[2 * i] & 0xFFFF) | ((uint32_t)in[2 * i + 1] << 16);
        }
    };
    // prepare_from: everything of the frame that depends on input samples only, into the lane's LDS slot
    // (cpk[p]: (c1, c0) of predictor p as a packed pair, low half c1)
    // Round 14, the self-served shape only (the shapes with a helper wave measured no gain and a loss at 1024 channels: they keep
    // the loop they had).  `numer` (wave-uniform, decided once per piece: no channel of the wave has coefficients above the
    // bound of pass_b_coef_ok): the range of samples 2..13 in the numerator domain (gc_encode_core.hpp N1, N3-N7,
    // prescan_numer_word) -- cpk[p] is then (-c1, -c0) of predictor p, low half -c1.  A wave with a hostile channel keeps the
    // reference's unchecked sum and the quotient, as a loop rolled over the predictors (rare: it must be small, not fast);
    // pair_of(p) hands it (c1, c0) of predictor p.
    auto prepare_from = [&](int tile, const uint32_t (&w)[7], const int (&in)[14], const uint32_t (&cpk)[8], const bool numer,
                            auto pair_of) __attribute__((always_inline)) {
        Slot &T = s_tile[tile & (BUFS - 1)].g[grp].f[hfr];
        uint4 *xr = reinterpret_cast<uint4 *>(&T.xw[0]);   // the pairs as loaded (the ints: in2048p and the pre-scan)
        xr[0] = make_uint4(w[0], w[1], w[2], w[3]);
        xr[1] = make_uint4(w[4], w[5], w[6], (!RAGGED || tile * TF + hfr < frames) ? 1u : 0u);   // (the spare dword: slot_has_frame)
        int4 *qr = reinterpret_cast<int4 *>(&T.in2048p[0]);
        qr[0] = make_int4(pass_b_row(in[0]), pass_b_row(in[1]), pass_b_row(in[2]), pass_b_row(in[3]));
        qr[1] = make_int4(pass_b_row(in[4]), pass_b_row(in[5]), pass_b_row(in[6]), pass_b_row(in[7]));
        qr[2] = make_int4(pass_b_row(in[8]), pass_b_row(in[9]), pass_b_row(in[10]), pass_b_row(in[11]));
        qr[3] = make_int4(pass_b_row(in[12]), pass_b_row(in[13]), 0, 0);
        // pre-scan distances of samples 2..13 (:107-115): predicted = (in[k]*c1 + in[k+1]*c0) / 2048 for the
        // pair starting at k = s - 2.  One v_dot2c_i32_i16 per (predictor, sample): the pairs at even k are
        // the loaded dwords, the pairs at odd k one v_alignbit each (shared by the 8 predictors); the
        // wrap of int32 is the reference's (unchecked arithmetic).
        uint32_t pair[12];
#pragma unroll
        for (int k = 0; k < 12; k++)
            pair[k] = (k & 1) ? __builtin_amdgcn_alignbit(w[(k + 1) / 2], w[(k - 1) / 2], 16) : w[k / 2];
        uint4 *pr = reinterpret_cast<uint4 *>(&T.pre[0]);
        if constexpr (!SELF) {
            uint32_t pre[8];
#pragma unroll
            for (int p = 0; p < 8; p++) {
                int dmax = 0, dmin = 0;
#ifdef VGA_GC_ABLATE_HELPER_PRESCAN                                  // timing only: what the helper's 96 distances per frame cost the launch
                dmax = in[2 + p] & 1023;
                dmin = -(in[3 + p] & 1023);
#else
#pragma unroll
                for (int k = 0; k < 12; k++) {
                    const int predicted = div2048(__builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, pair[k]),
                                                                         __builtin_bit_cast(short2v, cpk[p]), 0, false));
                    const int d = in[k + 2] - predicted;
                    dmax = imax(dmax, d);
                    dmin = imin(dmin, d);
                }
#endif
                pre[p] = (uint32_t)(clamp16i(dmax) & 0xFFFF) | ((uint32_t)clamp16i(dmin) << 16);
            }
            pr[0] = make_uint4(pre[0], pre[1], pre[2], pre[3]);
            pr[1] = make_uint4(pre[4], pre[5], pre[6], pre[7]);
        } else if (__builtin_expect(numer, 1)) {
            int a2048[12];
#pragma unroll
            for (int k = 0; k < 12; k++) a2048[k] = in[k + 2] * 2048;
            uint32_t pre[8];
#pragma unroll
            for (int q = 0; q < 8; q++) pre[q] = prescan_numer_word(pair, a2048, cpk[q]);
            pr[0] = make_uint4(pre[0], pre[1], pre[2], pre[3]);
            pr[1] = make_uint4(pre[4], pre[5], pre[6], pre[7]);
        } else {
#pragma unroll 1
            for (int q = 0; q < 8; q++) {
                const uint32_t cp = pair_of(q);
                int dmax = 0, dmin = 0;
#pragma unroll
                for (int k = 0; k < 12; k++) {
                    const int d = in[k + 2] - div2048(dot2_i16_wrap(pair[k], cp));
                    dmax = imax(dmax, d);
                    dmin = imin(dmin, d);
                }
                T.pre[q] = sat_pack16(dmax, dmin);
            }
        }
    };
    auto flush = [&](int tile) __attribute__((always_inline)) {
        const int fr = tile * TF + hfr;
        if (!live || fr >= frames) return;
        const int4 *rec = &s_tile[tile & (BUFS - 1)].g[grp].f[hfr].out[0];
        const int4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
        const int q[14] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y};
        uint2 v;
        pack_frame_mod16(q, r3.z, r3.w, v.x, v.y);   // the record holds q - Z from the hot pass, q from the reference's loop: alike mod 16
        if (fr < full_frames) {
            *reinterpret_cast<uint2 *>(dst + (int64_t)fr * 8) = v;
        } else {
            // partial last frame: SampleCountToByteCount(tail) bytes (:38)
            const int nbytes = (tail + 2 + 1) / 2;
            const uint64_t both = ((uint64_t)v.y << 32) | v.x;
            for (int b = 0; b < nbytes; b++) dst[(int64_t)fr * 8 + b] = (uint8_t)(both >> (8 * b));
        }
    };
    if (helper) {
        // ---------------------------------------------------------------- helper wave
        __builtin_amdgcn_s_setprio(VGA_GC_HELPER_PRIO);
        uint32_t cpk[8];                               // (c1, c0) of predictor p as a packed pair: low half c1
#pragma unroll
        for (int p = 0; p < 8; p++)
            cpk[p] = (uint32_t)(uint16_t)coefs[ch * 16 + 2 * p + 1] | ((uint32_t)(uint16_t)coefs[ch * 16 + 2 * p] << 16);
        auto prepare = [&](int tile) {
            uint32_t w[7];
            int in[14];
            load_frame(tile, w, in);
            prepare_from(tile, w, in, cpk, false, [](int) { return 0u; });
        };
        if (tiles > 0) prepare(0);
        __syncthreads();
        for (int tile = 0; tile < tiles; tile++) {
            if (tile + 1 < tiles) prepare(tile + 1);
            if (tile > 0) flush(tile - 1);
            __syncthreads();
        }
        if (tiles > 0) flush(tiles - 1);
        return;
    }

    // -------------------------------------------------------------------- serial (encoder) wave
    if constexpr (!SELF) __builtin_amdgcn_s_setprio(VGA_GC_ENCODER_PRIO);   // its latency is the kernel's run time: win every issue arbitration
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);   // (wave-uniform: a scalar register, for the tile heads)
    int p = CPW == 4 ? l16 >> 1 : l16;
    const bool cand_b = CPW == 4 && (l16 & 1) != 0;
    const int c0 = coefs[ch * 16 + 2 * p];
    const int c1 = coefs[ch * 16 + 2 * p + 1];
    // the bound of pass_fast_core_b (gc_encode_core.hpp B3: 30720, below the 32767 at which the predictor can wrap int32); a lane
    // above it takes the reference's loop as written
    const bool coef_ok = pass_b_coef_ok(c0, c1);
    int h0 = hist2 ? hist2[ch] : 0;   // pcmBuffer[0] = History2 (GcAdpcmEncoder.cs:24)
    int h1 = hist1 ? hist1[ch] : 0;   // pcmBuffer[1] = History1 (:25)
    if (repair) {
        h0 = seg_state[((int64_t)(repair_piece - 1) * nch + ch) * 2];
        h1 = seg_state[((int64_t)(repair_piece - 1) * nch + ch) * 2 + 1];
    } else if (by > 0 && (!RAGGED || frames > 0)) {   // a later piece: the guess
        h0 = src[-2];
        h1 = src[-1];
    }
    uint32_t hpk = pack16(h0, h1);                     // the history as the pass and the pre-scan take it: (h0, h1) in one register

    if (lane == 0) s_ncold[wave] = 0;                  // cold blocks this piece (diagnostics, g_vga_gc_stats)
    // (the pre-scan word is not part of the row: it is read at the head of its own frame, a dot product and the head distances
    // ahead of its use, and not a frame ahead -- one register less across the passes of the frame before)
    struct Row { uint32_t xw[7]; int mp[14]; };
    auto read_row = [&](const Slot &T, Row &R) {
        const uint4 *xr = reinterpret_cast<const uint4 *>(&T.xw[0]);
        const uint4 a0 = xr[0], a1 = xr[1];
        // keep the padding lanes "used": hipcc otherwise splits the 16-byte row reads into odd-sized ones
        asm volatile("" ::"v"(a1.w));
        uint32_t *xw = R.xw;
        xw[0] = a0.x; xw[1] = a0.y; xw[2] = a0.z; xw[3] = a0.w; xw[4] = a1.x; xw[5] = a1.y; xw[6] = a1.z;
        const int4 *qr = reinterpret_cast<const int4 *>(&T.in2048p[0]);
        const int4 e0 = qr[0], e1 = qr[1], e2 = qr[2], e3 = qr[3];
        asm volatile("" ::"v"(e3.z), "v"(e3.w));
        int *mp = R.mp;
        mp[0] = e0.x; mp[1] = e0.y; mp[2] = e0.z; mp[3] = e0.w; mp[4] = e1.x; mp[5] = e1.y; mp[6] = e1.z; mp[7] = e1.w;
        mp[8] = e2.x; mp[9] = e2.y; mp[10] = e2.z; mp[11] = e2.w; mp[12] = e3.x; mp[13] = e3.y;
    };
    // the lane's pre-scan word of the frame.  Its byte offset is made opaque per frame: hipcc otherwise forms slot + 4 p once
    // for the two frames of a loop trip and keeps that second address alive across the first frame (spilled at 128 VGPRs).
    auto read_pre = [&](const Slot &T) __attribute__((always_inline)) -> uint32_t {
        int pp = p;
        asm volatile("" : "+v"(pp));
        return T.pre[pp];
    };
    // RAGGED: is this frame one of the slot's own (else the slot's history stays frozen)?  The helper says so in the row's spare
    // dword, read where the frame's tail needs it: a per-lane frame count kept across the loop was one register too many.
    auto slot_has_frame = [&](const Slot &T) __attribute__((always_inline)) -> bool {
        if constexpr (RAGGED) return T.xw[7] != 0u;
        else return true;
    };
    auto pack = [](const uint32_t (&xw)[7]) {
        XW7 xs;
#pragma unroll
        for (int i = 0; i < 7; i++) xs.v[i] = xw[i];
        return xs;
    };
    // The two history-dependent pre-scan distances (:107-115), operands taken from pairs: predicted(s = 0) is the dot product of
    // the history pair (h0, h1) with (c1, c0), predicted(s = 1) that of (h1, x[2]) -- one v_alignbit across the history and the
    // row's first dword.  Unclamped dot product: int32 wraps where the reference's unchecked sum does.
    // Round 9, when no lane of the wave has coefficients that can wrap (wave-uniform, decided once per piece): both distances in
    // the numerator domain (gc_encode_core.hpp N1, head_distance_numer_b) from the clamped three-operand dot product with 1024 + 2^30 as
    // its accumulator.  The first one is P0, the dot product step 0 of both passes needs anyway: formed once here and handed to
    // them.  A wave with a hostile lane keeps the unchecked sum and the quotient for all its lanes (such a lane's first scale is
    // where the reference's loop as written starts from).
    const uint32_t cpk = pack16(c1, c0);
    // the rare pass with the 64-bit error sum keeps the old form (bound 32767) and takes the row as it was: 2^30 off again
    auto wide_total = [&](const uint32_t (&xw)[7], const int (&mp)[14], int sp) -> uint64_t {
        int row[14];
#pragma unroll
        for (int i = 0; i < 14; i++) row[i] = mp[i] - PASS_B_OFF;
        return pass_fast_core_wide(xw, hpk, row, c0, c1, sp).total;
    };
    const bool head_numer = __builtin_amdgcn_ballot_w64(!coef_ok) == 0;
    auto prescan_head = [&](const Row &R, int &d0, int &d1, int &P0) __attribute__((always_inline)) {
        P0 = predicted_b(hpk, cpk);
        if (__builtin_expect(head_numer, 1)) {
            d0 = head_distance_numer_b(R.mp[0], P0);
            d1 = head_distance_numer_b(R.mp[1], predicted_b(__builtin_amdgcn_alignbit(R.xw[0], hpk, 16), cpk));
        } else {
            d0 = pair_lo(R.xw[0]) - div2048(dot2_i16_wrap(hpk, cpk));
            d1 = pair_hi(R.xw[0]) - div2048(dot2_i16_wrap(__builtin_amdgcn_alignbit(R.xw[0], hpk, 16), cpk));
        }
    };
    // the first scale from the frame's range: the tie of +M and -M (gc_encode_core.hpp F4) needs pos == neg, looked at behind
    // one wave-uniform test
    auto first_scale = [&](const Row &R, uint32_t pre, int d0, int d1) __attribute__((always_inline)) -> int {
        const int dmax = imax(imax((int)(int16_t)(pre & 0xFFFF), d0), d1);
        const int dmin = imin(imin((int)pre >> 16, d0), d1);
        int sum, pos;
        int s1 = first_scale_power_nt(dmax, dmin, sum, pos);
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(sum == 0) != 0, 0)) {   // +M and -M both present (silence has sum == 1: F5): first occurrence decides
            if (sum == 0 && first_scale_tie(pos)) s1 = first_scale_power_from_md(prescan_sequential_cold(pack(R.xw), hpk, c0, c1));
        }
        return s1;
    };

    auto encode_frame = [&](Row &R, Slot &S, uint32_t pre) {
        const uint32_t (&xw)[7] = R.xw;
        // ---- pre-scan (:107-124): two history-dependent distances + the helper's range for s = 2..13
        int s1, P0;
        {
            int d0, d1;
            prescan_head(R, d0, d1, P0);
            s1 = first_scale(R, pre, d0, d1);
        }
        // ---- first trip: candidate A at s1, B at s1+1 (speculation on the loop of :127-170)
        int final_sp = imin(s1 + (cand_b ? 1 : 0), 12);
        const bool at_cap = final_sp >= 12;            // the loop never goes past 12: this pass ends it
        const unsigned ov_limit = at_cap ? 3u : 248u;  // see `rare` below
        PassOutB r = pass_fast_core_b<false, true>(xw, hpk, R.mp, c0, c1, final_sp, P0);
        // Straight-line resolution, valid when no lane is `rare`:
        //   * no overflow can start the bump loop (:166-168 needs max_overflow + 8 > 256),
        //   * the 32-bit error sum of every lane that can become final is exact (gc_encode_core.hpp S3:
        //     final lanes have overflow <= 1, or <= 3 at the cap, so (2 ov + 1) << (k - 11) <= 34996),
        //   * (total << 4) of the final lanes fits the 32-bit argmin key (`wide` otherwise; lanes that
        //     overflowed are not final and their error sums -- often huge -- are never looked at).
        // eff = overflow as the loop condition sees it (a pass at the cap ends the loop whatever it overflowed).
        // `rare`: the bump loop can start, or the coefficients can wrap -- the pair's A lane redoes the reference's loop
        // as written, for the whole wave (hostile input).  A pass at the cap that overflowed by more than 3 (loud noise,
        // clipped waves) is right except for its 32-bit error sum: `inexact`, the same pass again with a 64-bit sum.
        const bool rare = !coef_ok || (!at_cap && (unsigned)r.max_overflow > ov_limit);
        const int eff = at_cap ? 0 : r.max_overflow;
        const int eff_other = dpp<DPP_QUAD_XOR1>(eff);
        // A is final iff its pass did not overflow by more than 1; B is final iff A is not and B did not.
        bool fin = eff < 2 && (eff_other | (cand_b ? 0 : 2)) >= 2;
        const bool resume = !cand_b && imin(eff, eff_other) >= 2;     // both overflowed: A carries on at s1+2
        const bool inexact = fin && at_cap && (unsigned)r.max_overflow > ov_limit;
        // ---- the frame's tail: argmin over the 8 predictors (first index wins ties, :66-76), winner's history
        // broadcast, winner's record to LDS.  A lambda so that the hot and the cold branch each get their own
        // copy: merging the two branches' PassOut registers instead put the copies on the hot path.
        // 32-bit keys: error sums from 2^28 on share one key (such a predictor loses to any below -- as a rule it is one of
        // several wild ones); only when a channel's BEST is that large (`sat`, wave-uniform) do the 64-bit keys decide -- in
        // the cold block: the hot copy of the frame's tail holds no 64-bit code.
        constexpr unsigned SAT = (1u << 28) - 1;
        auto argmin32 = [&](const PassOutB &r, bool fin, bool &sat) __attribute__((always_inline)) -> int {
            const unsigned tot = umin32((unsigned)(r.total >> 32) ? SAT : (unsigned)r.total, SAT);
            const unsigned key = fin ? ((tot << 4) | (unsigned)l16) : 0xFFFFFFFFu;
            const unsigned best = row16_reduce(key, [](unsigned a, unsigned b) { return a < b ? a : b; });
            sat = __any((best >> 4) >= SAT);
            return (int)(best & 15u);
        };
        auto argmin64 = [&](uint64_t total, bool fin) __attribute__((always_inline)) -> int {
            uint64_t key = fin ? ((total << 4) | (uint64_t)l16) : ~0ull;
#define VGA_MIN64_STAGE(CTRL)                                                          \
            {                                                                          \
                const unsigned olo = (unsigned)dpp<CTRL>((int)(uint32_t)key);          \
                const unsigned ohi = (unsigned)dpp<CTRL>((int)(uint32_t)(key >> 32));  \
                const uint64_t okey = ((uint64_t)ohi << 32) | olo;                     \
                key = okey < key ? okey : key;                                         \
            }
            VGA_MIN64_STAGE(DPP_QUAD_XOR1)
            VGA_MIN64_STAGE(DPP_QUAD_XOR2)
            VGA_MIN64_STAGE(DPP_ROW_HALF_MIRROR)
            VGA_MIN64_STAGE(DPP_ROW_MIRROR)
#undef VGA_MIN64_STAGE
            return (int)(key & 15u);
        };
        // ---- the frame's tail: winner's history broadcast, winner's record to LDS.  A lambda so that the hot and the cold
        // branch each get their own copy: merging the two branches' PassOut registers instead put the copies on the hot path.
        auto commit = [&](const PassOutB &r, int final_sp, int winner) __attribute__((always_inline)) {
            const bool won = l16 == winner;
            const unsigned pay = row16_reduce(won ? r.hist_pair : 0u,
                                              [](unsigned a, unsigned b) { return a | b; });
            if (won) {                                           // packed and flushed by the helper, a tile at a time
                int4 *rec = &S.out[0];
                rec[0] = make_int4(r.q2[0], r.q2[1], r.q2[2], r.q2[3]);
                rec[1] = make_int4(r.q2[4], r.q2[5], r.q2[6], r.q2[7]);
                rec[2] = make_int4(r.q2[8], r.q2[9], r.q2[10], r.q2[11]);
                rec[3] = make_int4(r.q2[12], r.q2[13], p, final_sp);
            }
            if (slot_has_frame(S)) hpk = pay;    // pcmBuffer[0] = pcmBuffer[14], pcmBuffer[1] = pcmBuffer[15] (:40-41), as the pair
        };
        bool sat = false;
        const int winner32 = argmin32(r, fin && !inexact, sat);      // (a lane whose sum is not to be trusted yet is not in it)
        if (__builtin_expect(__any(rare || resume || inexact) || sat, 0)) {
            // ---- cold block (third trips: a third of the wave-frames on the synthetic set, LABNOTES 8.4)
#ifdef VGA_GC_STATS                                                  // (a -DVGA_GC_STATS build only: five instructions per cold block = 1 ms of the launch)
            if (lane == 0) atomicAdd(&s_ncold[wave], 1);
#endif
            ColdState st;
#pragma unroll
            for (int i = 0; i < 7; i++) st.xw[i] = xw[i];
#pragma unroll
            for (int i = 0; i < 14; i++) st.mp[i] = R.mp[i];
            st.hist = hpk;
            st.c0 = c0; st.c1 = c1; st.s1 = s1;
            const bool redo = __any(rare);             // (this layout: every pair's A lane walks the whole loop again, B lanes are out)
            st.generic = redo && !cand_b; st.start = s1 - 1; st.drop = redo && cand_b;
            st.wide = !redo && inexact; st.resume = !redo && resume;
            st.bump_a = 0; st.ov_a = 0; st.ov_b = 0;
            const ColdOut o = encode_frame_cold(st, r, final_sp, fin);
            bool sat2 = false;
            int winner = argmin32(o.r, o.fin != 0, sat2);
            if (sat2) {
                // the exact-sum rule (gc_encode_core.hpp E4): a channel's best sum is 2^28 or more, 64-bit keys decide -- and a final
                // lane up there whose sum came from a fast pass has "at least 2^28" for a sum: the pass at its scale again with the
                // scalar 64-bit error term.  (Coefficients that can wrap went through the reference's loop: sum_exact.)
                uint64_t total = o.r.total;
                if (o.fin != 0 && needs_exact_sum(total, o.sum_exact != 0))
                    total = wide_total(xw, R.mp, o.final_sp);
                winner = argmin64(total, o.fin != 0);
            }
            commit(o.r, o.final_sp, winner);
        } else
            commit(r, final_sp, winner32);
    };

    // ---- CPW = 8: lane = (channel, predictor); both trips of the reference's loop are passes of the SAME lane, one behind
    // the other: the pass at s1 for its overflow, then the final pass at the scale that overflow names (round 11).
    auto encode_frame8 = [&](Row &R, Slot &S, uint32_t pre) {
        const uint32_t (&xw)[7] = R.xw;
        int s1, P0;
        {
            int d0, d1;
            prescan_head(R, d0, d1, P0);
            s1 = first_scale(R, pre, d0, d1);
        }
        const int sp_a = imin(s1, 12), sp_b = imin(s1 + 1, 12);
        // Round 5: when every lane of the wave quantises at scale 9 or below (70 % of the synthetic set's wave-frames) the two
        // passes run without the detour through f32 -- (int)(float)d is d below 2^24, two conversions a sample less -- and each
        // lane checks from its overflow that no distance reached 2^24 (gc_encode_core.hpp: NO_ROUND); a lane that cannot
        // tell sends the wave through the passes as they always were.
        // Round 11: the pass at s1 runs for its overflow alone; it tells the lane which scale the reference ends on (or that the
        // lane goes to the cold block), and ONE final pass at that scale, sp2, delivers the nibbles, the history pairs and the
        // overflow the flags read where they read pass B's (gc_encode_core.hpp T1, T2: final_pass_pair).
        PassOutB r;
        int ov_a, sp2;
#ifdef VGA_GC_NO_FAST_PASSES                                       // (timing-only switch, tools/build_variants.sh)
        bool short_passes = false;
#else
        bool short_passes = !__any(sp_b > 9);
#endif
        if (short_passes) {
            r = final_pass_pair<true>(xw, hpk, R.mp, c0, c1, sp_a, sp_b, P0, ov_a, sp2);
            // (hostile coefficients: the lane walks the reference's loop as written whatever these passes say)
            const bool trusted = !coef_ok || (pass_no_round_is_exact(sp_a, ov_a) && pass_no_round_is_exact(sp2, r.max_overflow));
            short_passes = !__any(!trusted);
        }
        if (!short_passes) r = final_pass_pair<false>(xw, hpk, R.mp, c0, c1, sp_a, sp_b, P0, ov_a, sp2);
        const int ov_2 = r.max_overflow;
        // Which of the two passes the reference ends on, and what can stand in the way (each lane for itself, round 5):
        // gc_encode_core.hpp frame_flags.  Round 12: the hot path forms ONE bit from them, as compares and lane-mask logic
        // (frame_goes_cold); the single flags are worked out inside the cold branch, by the lanes that got there.
#ifdef VGA_GC_ABLATE_THIRD_TRIPS                                     // timing only (tools/build_variants.sh): what the cold block costs
        const FrameFlags ff0 = frame_flags(sp_a, sp_b, ov_a, ov_2, coef_ok);
        const bool cold = ff0.generic || ff0.inexact;
#else
        const bool cold = frame_goes_cold(sp_a, sp_b, ov_a, ov_2, coef_ok).cold;
#endif
        // (Round 6, measured and taken out again: the winning lanes storing the right pass's nibbles under their own masks
        // instead of fourteen selects in every lane -- 18 VALU instructions a frame less, two more exec-masked branches on
        // the wave's critical path: 148.5 ms against 146.0, profiles/r06_e_encode_variants.log.
        // Round 10, the same end without a branch, measured and taken out as well: every lane issuing the record writes of
        // BOTH passes, each to the record or to a dummy slot of the lane's own by two address selects -- 8 VALU instructions
        // a frame less, four LDS writes more: 118.3-118.7 ms against 117.8-118.5, profiles/r10_encode_ab.log.)
        // one error block (round 10): the final pass hands over its history pairs, the sum is formed here
        r.total = error_sum_pairs(xw, r.pairs);
        r.exact = true;
        const int final_sp = sp2;
        // 32-bit keys: error sums from 2^28 on share one key (such a predictor loses to any below); only when a channel's BEST
        // is that large (`sat`, wave-uniform) do the 64-bit keys decide -- in the cold block
        constexpr unsigned SAT = (1u << 28) - 1;
        auto argmin32 = [&](const PassOutB &r, bool fin, bool &sat) __attribute__((always_inline)) -> int {
            const unsigned tot = umin32((unsigned)(r.total >> 32) ? SAT : (unsigned)r.total, SAT);
            unsigned key = fin ? ((tot << 3) | (unsigned)p) : 0xFFFFFFFFu;
            key = umin32(key, (unsigned)dpp<DPP_QUAD_XOR1>((int)key));
            key = umin32(key, (unsigned)dpp<DPP_QUAD_XOR2>((int)key));
            key = umin32(key, (unsigned)dpp<DPP_ROW_HALF_MIRROR>((int)key));
            sat = __any((key >> 3) >= SAT);
            return (int)(key & 7u);
        };
        auto argmin64 = [&](uint64_t total, bool fin) __attribute__((always_inline)) -> int {
            uint64_t key = fin ? ((total << 3) | (uint64_t)p) : ~0ull;
#define VGA_MIN64_STAGE(CTRL)                                                          \
            {                                                                          \
                const unsigned olo = (unsigned)dpp<CTRL>((int)(uint32_t)key);          \
                const unsigned ohi = (unsigned)dpp<CTRL>((int)(uint32_t)(key >> 32));  \
                const uint64_t okey = ((uint64_t)ohi << 32) | olo;                     \
                key = okey < key ? okey : key;                                         \
            }
            VGA_MIN64_STAGE(DPP_QUAD_XOR1)
            VGA_MIN64_STAGE(DPP_QUAD_XOR2)
            VGA_MIN64_STAGE(DPP_ROW_HALF_MIRROR)
#undef VGA_MIN64_STAGE
            return (int)(key & 7u);
        };
        auto commit = [&](const PassOutB &r, int final_sp, int winner) __attribute__((always_inline)) {
            const bool won = p == winner;
            unsigned pay = won ? r.hist_pair : 0u;
            pay |= (unsigned)dpp<DPP_QUAD_XOR1>((int)pay);
            pay |= (unsigned)dpp<DPP_QUAD_XOR2>((int)pay);
            pay |= (unsigned)dpp<DPP_ROW_HALF_MIRROR>((int)pay);
            if (won) {
                int4 *rec = &S.out[0];
                rec[0] = make_int4(r.q2[0], r.q2[1], r.q2[2], r.q2[3]);
                rec[1] = make_int4(r.q2[4], r.q2[5], r.q2[6], r.q2[7]);
                rec[2] = make_int4(r.q2[8], r.q2[9], r.q2[10], r.q2[11]);
                rec[3] = make_int4(r.q2[12], r.q2[13], p, final_sp);
            }
            if (slot_has_frame(S)) hpk = pay;    // (a slot past its last frame keeps the history it ended on)
        };
        bool sat = false;
        const int winner32 = argmin32(r, !cold, sat);
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(cold) != 0 || sat, 0)) {
#ifdef VGA_GC_STATS                                                  // (a -DVGA_GC_STATS build only: five instructions per cold block = 1 ms of the launch)
            if (lane == 0) atomicAdd(&s_ncold[wave], 1);
#endif
            // what this lane needs there (a lane that is not cold has none of them set)
            const FrameFlags ff = frame_flags(sp_a, sp_b, ov_a, ov_2, coef_ok);
            const bool bump_a = ff.bump_a, generic = ff.generic, inexact = ff.inexact;
#ifdef VGA_GC_ABLATE_THIRD_TRIPS
            const bool resume = false;
#else
            const bool resume = ff.resume;                         // both overflowed: on to s1 + 2 in the cold block
#endif
            ColdState st;
#pragma unroll
            for (int i = 0; i < 7; i++) st.xw[i] = xw[i];
#pragma unroll
            for (int i = 0; i < 14; i++) st.mp[i] = R.mp[i];
            st.hist = hpk;
            st.c0 = c0; st.c1 = c1; st.s1 = s1;
            st.generic = generic; st.drop = 0; st.wide = inexact; st.resume = resume;
            // where the reference's loop stands (the value of scalePower before its next ++): at its start for hostile
            // coefficients; behind the bumps of the pass that started them otherwise (encode_frame_cold works that out)
#ifdef VGA_GC_R05_COLD                                                // (timing only: the cold block's entry as it was in round 5)
            st.start = !coef_ok ? s1 - 1 : (bump_a ? apply_bumps(s1, ov_a) : apply_bumps(s1 + 1, ov_2));
#else
            st.start = !coef_ok ? s1 - 1 : -100;
#endif
            st.bump_a = bump_a; st.ov_a = ov_a; st.ov_b = ov_2;      // (ov_2 is pass B's wherever the cold block reads it: not fin_a)
            const ColdOut o = encode_frame_cold(st, r, final_sp, (generic || resume) ? 0 : 1);
            bool sat2 = false;
            int winner = argmin32(o.r, o.fin != 0, sat2);
            if (sat2) {
                // the exact-sum rule (gc_encode_core.hpp E4): a channel's best sum is 2^28 or more, 64-bit keys decide -- and a final
                // lane up there whose sum came from a fast pass has "at least 2^28" for a sum: the pass at its scale again with the
                // scalar 64-bit error term.  (Coefficients that can wrap went through the reference's loop: sum_exact.)
                uint64_t total = o.r.total;
                if (o.fin != 0 && needs_exact_sum(total, o.sum_exact != 0))
                    total = wide_total(xw, R.mp, o.final_sp);
                winner = argmin64(total, o.fin != 0);
            }
            commit(o.r, o.final_sp, winner);
        } else
            commit(r, final_sp, winner32);
    };
    auto encode_one = [&](Row &R, Slot &S, uint32_t pre) __attribute__((always_inline)) {
        if constexpr (CPW == 4) encode_frame(R, S, pre);
        else encode_frame8(R, S, pre);
    };

#ifdef VGA_DEBUG_TIMESTAMPS
    if (!repair && tid == 0 && gridDim.y != 1) g_vga_enc_ts[2 * ((blockIdx.y * gridDim.x + blockIdx.x) & 32767)] = wall_clock64();
#endif
    // a tile's frames, by the encoder role
    auto encode_tile = [&](int tile) __attribute__((always_inline)) {
        const int buf = tile & (BUFS - 1);
        const int nf = imin(TF, frames_wg - tile * TF);
#ifndef VGA_GC_NO_TILE_REDERIVE                        // (timing-only switch, tools/build_variants.sh)
        {
            // the lane's LDS address follows from its slot and predictor: derived again for every tile -- kept across the piece
            // they were spilled and came back through scratch loads the tile had to wait for.  Round 12: from the hardware's
            // lane number and the wave's number in a scalar register; at 128 VGPRs `lane` itself is a spilled value.
            // (the count's start value is opaque, or hipcc forms the lane number once per piece and spills THAT)
            unsigned zero = 0;
            asm volatile("" : "+s"(zero));
            const int l = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, zero));
            grp = wave_u * CPW + l / LPC;
            p = CPW == 4 ? (l & (LPC - 1)) >> 1 : (l & (LPC - 1));
        }
#endif
        // The lane's one LDS address: rows, pre-scan words and records are immediate offsets from it, and it moves on by two
        // frames per trip (TF is even and j is: S[1] is a frame of the tile; S[2] behind the tile's last pair is the padding
        // and the next channel slot's first frame, or s_tiles.end -- read, never used).
        Slot *S = &s_tile[buf].g[grp].f[0];
        // two row register sets, ping-pong: the LDS reads of frame j+1 are in flight during frame j
        Row RA, RB;
        read_row(S[0], RA);
#pragma unroll 1
        for (int j = 0; j < nf; j += 2, S += 2) {
            // (LDS answers in order: the frame's own pre-scan word is asked for BEFORE the next frame's six row reads)
            const uint32_t pre_a = read_pre(S[0]);
            read_row(S[1], RB);
            encode_one(RA, S[0], pre_a);
            if (j + 1 < nf) {
                const uint32_t pre_b = read_pre(S[1]);
                read_row(S[2], RA);
                encode_one(RB, S[1], pre_b);
            }
        }
    };
    if constexpr (SELF) {
        // ---- the self-served tile loop: no other wave touches this workgroup's LDS, and one wave's LDS operations complete
        // in the order it issued them -- a fence of wavefront scope (no instruction: the compiler keeps its LDS accesses on
        // either side) and s_waitcnt lgkmcnt(0) stand where the 2 + 1 shape has its workgroup barrier.
        auto own_lds_done = [&]() __attribute__((always_inline)) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_s_waitcnt(0xC07F);            // lgkmcnt(0); vmcnt and expcnt left alone
        };
        // the helper role's coefficient pairs: predictor q's pair is what the encoder role's lane (slot, q) holds
        auto prepare_self = [&](int tile, const uint32_t (&w)[7]) __attribute__((always_inline)) {
            // (negated for the numerator form, one packed subtract per tile; head_numer is the flag over the same eight channels)
            const uint32_t ncpk = pk_sub_sat_i16(0u, cpk);
            uint32_t ncp8[8];
#pragma unroll
            for (int q = 0; q < 8; q++) ncp8[q] = (uint32_t)__shfl((int)ncpk, (lane & 56) | q);
            int in[14];
#pragma unroll
            for (int i = 0; i < 7; i++) {
                in[2 * i] = (int)(int16_t)(w[i] & 0xFFFF);
                in[2 * i + 1] = (int)w[i] >> 16;
            }
            prepare_from(tile, w, in, ncp8, head_numer, [&](int q) { return (uint32_t)__shfl((int)cpk, (lane & 56) | q); });
        };
        uint32_t wn[7];                                    // the lane's frame of the NEXT tile, loaded a tile ahead
        int unused[14];
        if (tiles > 0) {
            load_frame(0, wn, unused);
            prepare_self(0, wn);
            own_lds_done();
        }
        for (int tile = 0; tile < tiles; tile++) {
            const bool more = tile + 1 < tiles;
            if (more) load_frame(tile + 1, wn, unused);    // in flight during the tile's frames
            encode_tile(tile);
            own_lds_done();                                // the winners' records
            flush(tile);
            if (more) prepare_self(tile + 1, wn);
            own_lds_done();
        }
    } else {
    __syncthreads();                                   // tile 0 prepared
    for (int tile = 0; tile < tiles; tile++) {
        encode_tile(tile);
        __syncthreads();                               // tile done: helper may flush it and refill this buffer later
    }
    }
    if (seg_state && !repair && live && l16 == 0) {   // one lane per channel
        int16_t *st = seg_state + ((int64_t)by * nch + ch) * 2;
        st[0] = (int16_t)pair_lo(hpk);
        st[1] = (int16_t)pair_hi(hpk);
    }
    if (lane == 0) {
        atomicAdd(&g_vga_gc_stats[3], (unsigned long long)frames_wg);
        atomicAdd(&g_vga_gc_stats[4], (unsigned long long)s_ncold[wave]);
        if (wave == 0) atomicAdd(&g_vga_gc_stats[6], 1ull);
    }
#ifdef VGA_DEBUG_TIMESTAMPS
    if (!repair && tid == 0 && gridDim.y != 1) g_vga_enc_ts[2 * ((blockIdx.y * gridDim.x + blockIdx.x) & 32767) + 1] = wall_clock64();
#endif
}


template <bool REPAIR, int CPW, bool RAGGED>
__global__ __launch_bounds__(ENC_THREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) void gc_encode_kernel(
    const int16_t *__restrict__ pcm, int64_t pcm_pitch, int nch, int total_samples, const Pieces seg,
    const int16_t *__restrict__ coefs, const int16_t *__restrict__ hist1,
    const int16_t *__restrict__ hist2, uint8_t *__restrict__ adpcm, int64_t adpcm_pitch, int16_t *__restrict__ seg_state,
    const int *__restrict__ first_open, const Ragged rg)
{
    gc_encode_piece<REPAIR, CPW, RAGGED>(blockIdx.x, blockIdx.y, pcm, pcm_pitch, nch, total_samples, seg, coefs, hist1, hist2, adpcm,
                                         adpcm_pitch, seg_state, first_open, rg);
}

// ---------------------------------------------------------------- seams of the time segments
__device__ __forceinline__ void store_frame_bytes(uint8_t *dst, uint32_t d0, uint32_t d1, int nbytes)
{
    const uint64_t bits = ((uint64_t)d1 << 32) | d0;
    for (int b = 0; b < nbytes; b++) dst[b] = (uint8_t)(bits >> (8 * b));
}

// Eight lanes per (channel, seam) -- one per predictor, as DspEncodeFrame's loop (:58-77).  seam_run: from the TRUE history
// (h0, h1) at the start of piece k encode again frame by frame, next to a replay of the reconstruction of the run whose
// bytes the piece holds (decoding its frames from ITS start history (g2, g1), before they are overwritten), until both
// histories coincide at a frame end: from there on the piece holds what the serial encoder writes.  Returns with
// open == true when the piece ended first; (h0, h1) is then the true history at the piece's end.
// LPC (round 6): lanes per channel.  8: a lane per predictor, the two speculative passes of a frame one after the other in the
// same lane (two chains for the instruction stream to interleave: the layout of the seams inside the persistent kernel,
// where every SIMD holds other waves).  16: a lane per (predictor, candidate) -- pass A (scale s1) in the even lane, pass B
// (s1 + 1) in the odd one, as the encoder's CPW = 4 layout -- half the instructions per frame on the frame's critical
// path: for the seam and chain launches of batches below 512 channels, whose run time IS their slowest seam's.
template <int LPC>
__device__ __forceinline__ void seam_run(const int16_t *__restrict__ src, uint8_t *__restrict__ dst, int c0, int c1, bool coef_ok,
                                         int pr, int ch, int k, int64_t f0, int total_samples, int piece_frames, int max_frames, int force_open,
                                         int &h0, int &h1, int g2, int g1, bool &open, int &frames_run)
{
    static_assert(LPC == 8 || LPC == 16, "a lane per predictor, or per (predictor, candidate)");
    const bool cand_b = LPC == 16 && (threadIdx.x & 1) != 0;
    const int full_frames = total_samples / 14;
    // The frame loop is one wave's dependent chain (nothing else runs on its SIMD for long: the slowest seam IS the
    // kernel's run time), so it is the encoder's fast path -- range pre-scan, the two speculative passes of the
    // (channel, predictor) layout, DPP argmin -- with the next frame's PCM and old bytes already in flight; the
    // reference's loop as written (resume_passes) only behind the same `rare` / `resume` conditions as there.
    const int64_t f_end = imin((int)imin((int)(f0 + piece_frames), (int)(f0 + max_frames)), full_frames);   // frames [f0, f_end)
    const int64_t f_last = full_frames > 0 ? full_frames - 1 : 0;
    // (Round 6, measured and taken out again: the frames a block of LPC at a time -- lane j of the group loading frame fb + j,
    // the next block in flight, a frame's nine dwords handed round through the crossbar.  Nothing gained, 5 % lost at 512
    // channels: the loop does not wait for its loads -- a frame of a seam run is ~1000 instructions of a lone wave at
    // 2.3 ns each (replay 200, pre-scan 160, passes 220-450, argmin / pack / store 120), profiles/r06_m_channel_scaling.log.)
    auto fetch = [&](int64_t f, uint32_t (&w)[7], uint2 &old) {
        const int64_t fc = f < f_last ? f : f_last;     // clamped: always a valid full frame (unconditional loads)
        const uint32_t *p32 = reinterpret_cast<const uint32_t *>(src + fc * 14);
#pragma unroll
        for (int i = 0; i < 7; i++) w[i] = p32[i];
        old = *reinterpret_cast<const uint2 *>(dst + fc * 8);
    };
    uint32_t w[7], wn[7];
    uint2 old, oldn;
    fetch(f0, w, old);
    for (int64_t f = f0; ; f++) {
        const bool in_range = f < f_end;
        if (!__any(open && in_range)) break;
        const bool act = open && in_range;
        frames_run += act ? 1 : 0;
        fetch(f + 1, wn, oldn);                         // in flight during this frame
        int x[16], mp[14];
        x[0] = h0;
        x[1] = h1;
        const uint32_t hpk = pack16(h0, h1);
#pragma unroll
        for (int i = 0; i < 7; i++) {
            x[2 + 2 * i] = (int)(int16_t)(w[i] & 0xFFFF);
            x[3 + 2 * i] = (int)w[i] >> 16;
        }
#pragma unroll
        for (int i = 0; i < 14; i++) mp[i] = x[2 + i] * 2048 + 1024;
        // the guessed run's reconstruction of this frame (GcAdpcmDecoder.cs:25-45), from its bytes before they change
        {
            const int ps = (int)(old.x & 0xFFu);
            const int scale = (1 << (ps & 0xF)) * 2048;
            const int pred = (ps >> 4) & 7;
            // that predictor's pair sits in lane `pred` (LPC = 16: lanes 2 pred, 2 pred + 1) of the group
            const int k1 = __shfl(c0, LPC == 16 ? 2 * pred : pred, LPC), k2 = __shfl(c1, LPC == 16 ? 2 * pred : pred, LPC);
            const uint64_t bits = ((uint64_t)old.y << 32) | old.x;            // byte b of the frame = bits >> 8b
#pragma unroll
            for (int s2 = 0; s2 < 14; s2++) {
                const int byte = (int)((bits >> (8 * (1 + (s2 >> 1)))) & 0xFFu);
                const int nib = (s2 & 1) ? (byte & 0xF) : (byte >> 4);
                const int v = clamp16i((k1 * g1 + k2 * g2 + scale * ((nib ^ 8) - 8) + 1024) >> 11);
                g2 = g1;
                g1 = v;
            }
        }
        // the true frame: pre-scan (:107-124), candidates A and B (:127-170), see encode_frame8
        int s1;
        {
            int dmax = 0, dmin = 0;
            prescan_range(x, c0, c1, 0, 14, dmax, dmin);
            s1 = first_scale_power_from_range(dmax, dmin);
            if (s1 == -100) s1 = first_scale_power_from_md(prescan_sequential(x, c0, c1));
        }
        const int sp_a = imin(s1, 12), sp_b = imin(s1 + 1, 12);
        PassOut r;
        int final_sp;
        bool fin = true;                               // LPC = 16: this lane's pass is the one the reference ends on
        if (LPC == 8) {
        // (the passes as they always were: without the f32 detour -- tried in round 5 -- a seam run is no faster, LABNOTES 9.7)
        // (at the cap from overflow 3 on, not 4 as until round 8: the sum in pairs is exact whatever its size only up to
        // overflow 2 there -- gc_encode_core.hpp E5 -- and this loop hands it to a 64-bit argmin as it is)
        const PassOut rb = pass_fast_core(w, hpk, mp, c0, c1, sp_b);
        const PassOut ra = pass_fast_core(w, hpk, mp, c0, c1, sp_a);
        const bool cap_a = sp_a >= 12, cap_b = sp_b >= 12;
        const bool rare = !coef_ok || (unsigned)ra.max_overflow > (cap_a ? 2u : 248u) || (unsigned)rb.max_overflow > (cap_b ? 2u : 248u);
        const int eff_a = cap_a ? 0 : ra.max_overflow, eff_b = cap_b ? 0 : rb.max_overflow;
        const bool fin_a = eff_a < 2;
        const bool resume = !fin_a && eff_b >= 2;
#pragma unroll
        for (int i = 0; i < 14; i++) r.q[i] = fin_a ? ra.q[i] : rb.q[i];
        r.total = fin_a ? ra.total : rb.total;
        r.hist_pair = fin_a ? ra.hist_pair : rb.hist_pair;
        final_sp = fin_a ? sp_a : sp_b;
        if (__any(rare || resume)) {
            if (rare || resume) {
                const PassOut rc = resume_passes(x, c0, c1, rare ? s1 - 1 : s1 + 1, final_sp);
#pragma unroll
                for (int i = 0; i < 14; i++) r.q[i] = rc.q[i];
                r.total = rc.total;
                r.hist_pair = rc.hist_pair;
            }
        }
        } else {
            // one pass per lane: A at s1 (even lane), B at s1 + 1 (odd lane); the pair decides from the two overflows which of
            // them the reference's loop ends on (encode_frame, CPW = 4); anything else -- both overflowed, a bump, an inexact
            // sum, hostile coefficients -- and the A lane walks the reference's loop as written, the B lane is out
            final_sp = cand_b ? sp_b : sp_a;
            r = pass_fast_core(w, hpk, mp, c0, c1, final_sp);
            const bool cap = final_sp >= 12;
            const bool rare_mine = !coef_ok || (unsigned)r.max_overflow > (cap ? 2u : 248u);
            const int eff = cap ? 0 : r.max_overflow;
            const int eff_other = dpp<DPP_QUAD_XOR1>(eff);
            // (the exchange on its own line: behind `rare_mine ||` it would run only in the lanes whose own flag is clear, and
            // read their partners -- the lanes it is there to hear from -- as inactive)
            const int rare_other = dpp<DPP_QUAD_XOR1>(rare_mine ? 1 : 0);
            const bool rare = rare_mine || rare_other != 0;
            const int eff_a = cand_b ? eff_other : eff, eff_b = cand_b ? eff : eff_other;
            const bool fin_a = eff_a < 2;
            const bool resume = !fin_a && eff_b >= 2;
            fin = cand_b ? !fin_a : fin_a;
            if (__any(rare || resume)) {
                if (rare || resume) {
                    fin = !cand_b;
                    if (!cand_b) r = resume_passes(x, c0, c1, rare ? s1 - 1 : s1 + 1, final_sp);
                }
            }
        }
        // totals are below 2^60 (14 squares of 17-bit errors): the predictor (LPC = 16: the lane of the group, predictor-major
        // -- one lane of a pair at most is in it) rides in the low bits
        const int lidx = LPC == 16 ? (int)(threadIdx.x & 15) : pr;
        uint64_t key = (act && fin) ? ((r.total << 4) | (uint64_t)lidx) : ~0ull;
#define VGA_MIN64_STAGE(CTRL)                                                          \
        {                                                                              \
            const unsigned olo = (unsigned)dpp<CTRL>((int)(uint32_t)key);              \
            const unsigned ohi = (unsigned)dpp<CTRL>((int)(uint32_t)(key >> 32));      \
            const uint64_t okey = ((uint64_t)ohi << 32) | olo;                         \
            key = okey < key ? okey : key;                                             \
        }
        VGA_MIN64_STAGE(DPP_QUAD_XOR1)
        VGA_MIN64_STAGE(DPP_QUAD_XOR2)
        VGA_MIN64_STAGE(DPP_ROW_HALF_MIRROR)
        if (LPC == 16) VGA_MIN64_STAGE(DPP_ROW_MIRROR)
#undef VGA_MIN64_STAGE
        const bool won = act && fin && lidx == (int)(key & 15u);
        unsigned pay = won ? r.hist_pair : 0u;
        pay |= (unsigned)dpp<DPP_QUAD_XOR1>((int)pay);
        pay |= (unsigned)dpp<DPP_QUAD_XOR2>((int)pay);
        pay |= (unsigned)dpp<DPP_ROW_HALF_MIRROR>((int)pay);
        if (LPC == 16) pay |= (unsigned)dpp<DPP_ROW_MIRROR>((int)pay);
        if (won) {
            uint32_t d0, d1;
            pack_frame(r.q, pr, final_sp, d0, d1);
            *reinterpret_cast<uint2 *>(dst + f * 8) = make_uint2(d0, d1);
        }
        if (act) {
            h0 = (int)(int16_t)(pay & 0xFFFF);          // :40-41
            h1 = (int)pay >> 16;
            if (h0 == g2 && h1 == g1 && !seam_forced_open(force_open, ch, k)) open = false;   // closed
        }
#pragma unroll
        for (int i = 0; i < 7; i++) w[i] = wn[i];
        old = oldn;
    }
}

// The zero-padded partial last frame of a stream (GcAdpcmEncoder.cs:32-38) from the true history (h0, h1), by the eight
// lanes of a channel exactly as seam_run encodes a frame; SampleCountToByteCount(tail) bytes are stored.  For the chain
// kernel: a run that is still apart at the very end of the stream has only this frame left to correct.
template <int LPC>
__device__ __forceinline__ void encode_tail_frame(const int16_t *__restrict__ src, uint8_t *__restrict__ dst, int c0, int c1,
                                                  bool coef_ok, int pr, int total_samples, int h0, int h1, bool act)
{
    const int full_frames = total_samples / 14, tail = total_samples - full_frames * 14;
    int x[16], mp[14];
    x[0] = h0;
    x[1] = h1;
    const uint32_t hpk = pack16(h0, h1);
#pragma unroll
    for (int i = 0; i < 14; i++) x[2 + i] = i < tail ? (int)src[(int64_t)full_frames * 14 + i] : 0;
#pragma unroll
    for (int i = 0; i < 14; i++) mp[i] = x[2 + i] * 2048 + 1024;
    int s1;
    {
        int dmax = 0, dmin = 0;
        prescan_range(x, c0, c1, 0, 14, dmax, dmin);
        s1 = first_scale_power_from_range(dmax, dmin);
        if (s1 == -100) s1 = first_scale_power_from_md(prescan_sequential(x, c0, c1));
    }
    const int sp_a = imin(s1, 12), sp_b = imin(s1 + 1, 12);
    uint32_t w[7];
    pack_row(x, w);
    const PassOut rb = pass_fast_core(w, hpk, mp, c0, c1, sp_b);
    const PassOut ra = pass_fast_core(w, hpk, mp, c0, c1, sp_a);
    const bool cap_a = sp_a >= 12, cap_b = sp_b >= 12;
    const bool rare = !coef_ok || (unsigned)ra.max_overflow > (cap_a ? 2u : 248u) || (unsigned)rb.max_overflow > (cap_b ? 2u : 248u);   // (2: as seam_run)
    const int eff_a = cap_a ? 0 : ra.max_overflow, eff_b = cap_b ? 0 : rb.max_overflow;
    const bool fin_a = eff_a < 2;
    const bool resume = !fin_a && eff_b >= 2;
    PassOut r;
#pragma unroll
    for (int i = 0; i < 14; i++) r.q[i] = fin_a ? ra.q[i] : rb.q[i];
    r.total = fin_a ? ra.total : rb.total;
    int final_sp = fin_a ? sp_a : sp_b;
    if (rare || resume) {
        const PassOut rc = resume_passes(x, c0, c1, rare ? s1 - 1 : s1 + 1, final_sp);
#pragma unroll
        for (int i = 0; i < 14; i++) r.q[i] = rc.q[i];
        r.total = rc.total;
    }
    // (LPC = 16: both lanes of a predictor hold the same frame -- the even one is in the argmin and stores)
    const bool in_it = act && (LPC == 8 || (threadIdx.x & 1) == 0);
    uint64_t key = in_it ? ((r.total << 3) | (uint64_t)pr) : ~0ull;
#define VGA_MIN64_STAGE(CTRL)                                                          \
    {                                                                                  \
        const unsigned olo = (unsigned)dpp<CTRL>((int)(uint32_t)key);                  \
        const unsigned ohi = (unsigned)dpp<CTRL>((int)(uint32_t)(key >> 32));          \
        const uint64_t okey = ((uint64_t)ohi << 32) | olo;                             \
        key = okey < key ? okey : key;                                                 \
    }
    VGA_MIN64_STAGE(DPP_QUAD_XOR1)
    VGA_MIN64_STAGE(DPP_QUAD_XOR2)
    VGA_MIN64_STAGE(DPP_ROW_HALF_MIRROR)
    if (LPC == 16) VGA_MIN64_STAGE(DPP_ROW_MIRROR)
#undef VGA_MIN64_STAGE
    if (in_it && pr == (int)(key & 7u)) {
        uint32_t d0, d1;
        pack_frame(r.q, pr, final_sp, d0, d1);
        const int nibbles = tail + 2;                                   // SampleCountToNibbleCount of the tail (GcAdpcmMath.cs:24-30)
        store_frame_bytes(dst + (int64_t)full_frames * 8, d0, d1, nibbles / 2 + (nibbles & 1));
    }
}

// All seams at once, each from the history the piece before ended on (seg_state: the real one provided THAT piece's own
// seam closes).  A seam still open at the end of its piece leaves a flag and the true history it arrived at
// (seam_flag / seam_end) and its index in first_open[channel]: gc_encode_chain_kernel carries on from there.
template <int LPC>
__device__ __forceinline__ void seam_piece(
    const int slot_raw, const int k, const int lane,
    const int16_t *__restrict__ pcm, int64_t pcm_pitch, int nch, int total_samples, const Pieces seg,
    const int16_t *__restrict__ coefs, uint8_t *adpcm, int64_t adpcm_pitch,
    const int16_t *seg_state, int *first_open, int *seam_flag, int *seam_end, int force_open, const Ragged &rg)
{
    const int pr = LPC == 16 ? (lane >> 1) & 7 : lane & 7;        // this lane's predictor
    const bool lead = (lane & (LPC - 1)) == 0;          // one lane per channel: flags, statistics
    const int64_t f0 = seg.first(k);
    const int slot = slot_raw < nch ? slot_raw : nch - 1;
    const int ch = rg.order ? rg.order[slot] : slot;
    if (rg.order) total_samples = rg.length[ch];        // ragged: the seam exists only where the channel reaches piece k
    const bool valid = slot_raw < nch && f0 * 14 < total_samples;
    const int16_t *src = pcm + (rg.order ? rg.pcm_off[ch] : (int64_t)ch * pcm_pitch);
    uint8_t *dst = adpcm + (rg.order ? rg.adpcm_off[ch] : (int64_t)ch * adpcm_pitch);
    const int16_t *cf = coefs + ch * 16;
    const int c0 = cf[2 * pr], c1 = cf[2 * pr + 1];
    const bool coef_ok = (c0 < 0 ? -c0 : c0) + (c1 < 0 ? -c1 : c1) <= 32767;
    int h0 = valid ? seg_state[((int64_t)(k - 1) * nch + ch) * 2] : 0;            // true history (x[0], x[1])
    int h1 = valid ? seg_state[((int64_t)(k - 1) * nch + ch) * 2 + 1] : 0;
    const int g2 = valid ? src[f0 * 14 - 2] : 0, g1 = valid ? src[f0 * 14 - 1] : 0;   // the guessed run's history (g1 = newest)
    bool open = valid;                                  // uniform inside a group of eight
    int frames_run = 0;
    seam_run<LPC>(src, dst, c0, c1, coef_ok, pr, ch, k, f0, total_samples, seg.frames(k), seg.frames(k), force_open, h0, h1, g2, g1, open, frames_run);
    // still open at the piece's end (half the seams close within nine frames, one in a hundred needs more than 400, a
    // few channels never meet)
    if (valid && lead) {
        atomicAdd(&g_vga_gc_stats[open ? 1 : 0], 1ull);
        atomicAdd(&g_vga_gc_stats[2], (unsigned long long)frames_run);
        seam_flag[(int64_t)(k - 1) * nch + ch] = open ? 1 : 0;
        if (open) {
            seam_end[(int64_t)(k - 1) * nch + ch] = (int)(((unsigned)h1 << 16) | ((unsigned)h0 & 0xFFFFu));
            atomicMin(&first_open[ch], k);
        }
    }
}

// Round 15, the self-served shape on uniform batches: open seams handed on inside the launch.  What gc_encode_chain_kernel
// does piece after piece in a launch of its own -- one wave per group of eight, alone on the chip, for as long as its
// slowest channel's runs take to meet -- happens here as soon as its inputs exist, underneath the other waves' items.
//
// The chain is serial in the pieces for a reason: the history a seam's own run starts from (T = seg_state[k - 1]) is the
// true one only when everything before it has been settled, so a seam's recorded end is "the truth provided a true run
// has met mine".  So a TOKEN walks every group's pieces in order, 2, 3, ...: per channel either "nothing enters piece p"
// or "V enters piece p: the true history there, which the piece's bytes were not encoded from".  The token for piece 2
// comes from seam 1's own run (piece 0 starts from the caller's history: that run is the true one).  Piece p then needs
// two things, and they arrive in either order on word[(p - 1) * groups + group]:
//   a) the own run of seam p has finished: its flag and end are written, the piece's bytes are its run from T;
//   b) the token for piece p has arrived: token / v[(p - 1) * nch + channel] are written.
// Whoever arrives second runs the continuation for the group's eight channels -- seam_run from V next to the replay from
// T for the channels that have a V, the others' lanes idle -- applies the chain launch's three rules (still apart: carry V
// on; met a run that was itself flagged: its recorded end is the truth; else nothing), and takes the token to piece p + 1
// by the same rule: it finds a) there and continues, or leaves b) and returns to the queue.  Nobody ever waits.  The
// fences are seam_count's: a device-scope fence between a party's stores and its add, another before the second party
// reads.  Behind the last piece the token becomes the channel's record (row segments - 1 of the same arrays): the chain
// launch then runs no seam_run for the channel, and encodes the partial last frame from V when a run was still apart
// there -- the one case that stays with it.  Nothing is written into seam_flag or first_open on the way (other waves read
// the one and atomicMin the other); the chain launch clears first_open as it always did.
constexpr int HAND_ARRIVED = 1;                // a token (or record) has been written
constexpr int HAND_V = 2;                      // ... and it carries a V
constexpr int HAND_EVER = 4;                   // ... the channel had an open seam somewhere before (statistics, [8])
struct Handover {
    int *word = nullptr;                       // null: no hand-over (the chain launch does it all)
    int *token = nullptr, *v = nullptr;
};

// The seams at the ends of the piece a wave of the self-served kernel has just encoded (seam_a, seam_b: 0 = not this wave's),
// and whatever continuations the hand-over brings it.  ONE copy of seam_run: the runs are steps of a loop.
template <class P>
__device__ __forceinline__ void self_served_seams(
    const int g, const int seam_a, const int seam_b, const int lane, const int groups, const int segments, const int rec_row,
    const int16_t *__restrict__ pcm, int64_t pcm_pitch, int nch, int total_samples, const P seg,
    const int16_t *__restrict__ coefs, uint8_t *adpcm, int64_t adpcm_pitch,
    const int16_t *seg_state, int *first_open, int *seam_flag, int *seam_end, int force_open, const Handover hand)
{
    const int pr = lane & 7;                            // this lane's predictor
    const bool lead = pr == 0;                          // one lane per channel: flags, statistics, tokens
    const int slot_raw = g * PLAN8_SLOTS + (lane >> 3);
    const bool live = slot_raw < nch;
    const int ch = live ? slot_raw : nch - 1;
    const int16_t *src = pcm + (int64_t)ch * pcm_pitch;
    uint8_t *dst = adpcm + (int64_t)ch * adpcm_pitch;
    const int16_t *cf = coefs + ch * 16;
    const int c0 = cf[2 * pr], c1 = cf[2 * pr + 1];
    const bool coef_ok = (c0 < 0 ? -c0 : c0) + (c1 < 0 ? -c1 : c1) <= 32767;
    auto second_on = [&](int piece) {                   // announce on piece's word; true: the other party was there first
        __threadfence();                                // this wave's stores are out before it says so
        int old = 0;
        if (lane == 0) old = atomicAdd(&hand.word[(int64_t)(piece - 1) * groups + g], 1);
        const bool second = __builtin_amdgcn_readfirstlane(old) == 1;
        if (second) __threadfence();                    // the other party's stores, before anything of them is read
        return second;
    };
    int own = 0;                                        // own runs taken so far
    int p = 0;                                          // != 0: both parties of piece p are here: continue into it
    int state = 0, v0 = 0, v1 = 0;                      // the token this wave carries: what enters piece p (then: piece k + 1)
    for (;;) {
        const bool cont = p != 0;
        int k;
        if (cont) k = p;
        else if (own == 0) { own = 1; k = seam_a; }
        else if (own == 1) { own = 2; k = seam_b; }
        else break;
        p = 0;
        if (k == 0) continue;
        const int64_t f0 = seg.first(k);
        const bool valid = live && f0 * 14 < total_samples;
        const int64_t idx = (int64_t)(k - 1) * nch + ch;
        const int t0 = valid ? seg_state[idx * 2] : 0, t1 = valid ? seg_state[idx * 2 + 1] : 0;   // T
        // own run: from T next to the guessed run (the two input samples before the piece); continuation: from V next to T
        int h0 = cont ? v0 : t0, h1 = cont ? v1 : t1;
        const int g2 = cont ? t0 : (valid ? src[f0 * 14 - 2] : 0), g1 = cont ? t1 : (valid ? src[f0 * 14 - 1] : 0);
        bool open = cont ? valid && (state & HAND_V) != 0 : valid;
        const bool ran = open;
        int frames_run = 0;
        if (__any(open))
            seam_run<8>(src, dst, c0, c1, coef_ok, pr, ch, k, f0, total_samples, seg.frames(k), seg.frames(k), force_open, h0, h1, g2, g1, open, frames_run);
        if (!cont) {                                    // (as seam_piece)
            if (valid && lead) {
                atomicAdd(&g_vga_gc_stats[open ? 1 : 0], 1ull);
                atomicAdd(&g_vga_gc_stats[2], (unsigned long long)frames_run);
                seam_flag[idx] = open ? 1 : 0;
                if (open) {
                    seam_end[idx] = (int)(((unsigned)h1 << 16) | ((unsigned)h0 & 0xFFFFu));
                    atomicMin(&first_open[ch], k);
                }
            }
            if (!hand.word) continue;
            if (k == 1) {                               // the run from the caller's history: the true one
                state = HAND_ARRIVED | (open ? HAND_V | HAND_EVER : 0);
                v0 = h0;
                v1 = h1;
            } else {
                if (second_on(k)) {                     // a): the token was waiting
                    state = hand.token[idx];
                    const int v = hand.v[idx];
                    v0 = (int)(int16_t)(v & 0xFFFF);
                    v1 = v >> 16;
                    p = k;
                }
                continue;
            }
        } else {
            if (valid && lead && frames_run) atomicAdd(&g_vga_gc_stats[2], (unsigned long long)frames_run);
            const bool flagged = valid && seam_flag[idx] != 0;
            if (ran && open) {                          // still apart at the piece's end: carry on into the next one
                v0 = h0;
                v1 = h1;
            } else if (flagged) {                       // met the run from T, whose own seam ran out of frames: its end is the truth
                const int ended = seam_end[idx];
                state |= HAND_V | HAND_EVER;
                v0 = (int)(int16_t)(ended & 0xFFFF);
                v1 = ended >> 16;
            } else
                state &= ~HAND_V;
        }
        // (state, v0, v1): what enters piece k + 1 -- or, behind the stream's last piece, the channel's record in row
        // rec_row (segments - 1; round 16: of the longer of the batch's two schedules) (the test hook's equal pieces can leave
        // piece indices behind the end of the stream: nobody encodes
        // those, and no token waits for them)
        const bool last = k + 1 >= segments || seg.first(k + 1) * 14 >= total_samples;
        const int64_t nidx = (int64_t)(last ? rec_row : k) * nch + ch;
        if (live && lead) {
            hand.v[nidx] = (int)(((unsigned)v1 << 16) | ((unsigned)v0 & 0xFFFFu));
            hand.token[nidx] = state;
            if (last && (state & HAND_EVER) != 0) atomicAdd(&g_vga_gc_stats[8], 1ull);
        }
        if (last) continue;
        if (second_on(k + 1)) p = k + 1;                // b): the piece's own run has finished
    }
}

template <int LPC>
__global__ __launch_bounds__(64) void gc_encode_seam_kernel(
    const int16_t *__restrict__ pcm, int64_t pcm_pitch, int nch, int total_samples, const Pieces seg,
    const int16_t *__restrict__ coefs, uint8_t *__restrict__ adpcm, int64_t adpcm_pitch,
    const int16_t *__restrict__ seg_state, int *__restrict__ first_open, int *__restrict__ seam_flag,
    int *__restrict__ seam_end, int force_open, const Ragged rg)
{
    seam_piece<LPC>(blockIdx.x * (64 / LPC) + (threadIdx.x / LPC), blockIdx.y + 1, threadIdx.x, pcm, pcm_pitch, nch, total_samples, seg, coefs, adpcm,
               adpcm_pitch, seg_state, first_open, seam_flag, seam_end, force_open, rg);
}

// The same work from a queue: as many workgroups as the chip holds at once (cus x 4: two encoder waves and a helper on
// every SIMD, placed once), each taking (channel group, piece) items -- piece-major, so the early items are the ones every
// channel has -- until none is left.  Measured at BASELINE configs[1] with one workgroup per item and four pieces per
// channel (profiles/r04_a_wave_ends.log): the four pieces of a channel group share a CU, the groups' frames differ in how
// often they take the third-trip block, and the CUs end between 136 and 162 ms (mean 147) -- the launch lasts as long as
// its slowest CU.  More, shorter pieces from a plain grid made it worse (212 ms with eight): workgroups of the second
// round land on whichever SIMD has a free slot and two encoder waves end up sharing one.  Persistent workgroups keep
// their SIMDs and balance at the granularity of an item.
//
// The seams travel with the items: a workgroup that has finished piece y of a group announces it on the counters of the
// seams at the piece's two ends (seam_count[seam - 1][group]); whoever finds the other side already there closes that
// seam at once -- its two encoder waves have the seam code's lane layout (8 channels x 8 predictors), the group's sixteen
// channels are theirs -- while the other workgroups carry on with their items.  What the separate seam launch cost at the
// end of the encode (8 ms at four pieces per channel, as long as its slowest seam; 36 ms at 64 pieces) runs underneath
// the other workgroups' items.  A seam reads what two other workgroups wrote (the piece state before it, the bytes
// after it): both sides put a device-scope fence between their stores / loads and the counter.
template <int CPW, bool RAGGED>
__global__ __launch_bounds__(ENC_THREADS) __attribute__((amdgpu_waves_per_eu(VGA_GC_PERSISTENT_WAVES_PER_EU))) void gc_encode_persistent_kernel(
    const int16_t *__restrict__ pcm, int64_t pcm_pitch, int nch, int total_samples, const Pieces seg,
    const int16_t *__restrict__ coefs, const int16_t *__restrict__ hist1,
    const int16_t *__restrict__ hist2, uint8_t *adpcm, int64_t adpcm_pitch, int16_t *seg_state,
    const Ragged rg, int groups, int segments, int *__restrict__ queue, int *__restrict__ seam_count, int *first_open,
    int *seam_flag, int *seam_end, int force_open)
{
    static_assert(CPW == 8, "the seams inside the persistent kernel use the (channel, predictor) layout");
    constexpr int CS = Lay<CPW>::CS;
    __shared__ int s_item;
    __shared__ int s_seam[2];
    const int items = RAGGED && rg.items ? rg.n_items : groups * segments;
#ifdef VGA_DEBUG_TIMESTAMPS
    if (threadIdx.x == 0) g_vga_enc_ts[2 * (blockIdx.x & 32767)] = wall_clock64();
#endif
    for (;;) {
        if (threadIdx.x == 0) s_item = atomicAdd(queue, 1);
        __syncthreads();
        const int item = s_item;
        __syncthreads();                               // everyone has read it before thread 0 takes the next one
        if (item >= items) {
#ifdef VGA_DEBUG_TIMESTAMPS
            if (threadIdx.x == 0) g_vga_enc_ts[2 * (blockIdx.x & 32767) + 1] = wall_clock64();
#endif
            return;
        }
        int g = item % groups, y = item / groups;      // piece-major ...
        if (RAGGED && rg.items) {                      // ... or the host's list: biggest items first
            const uint32_t v = rg.items[item];
            g = (int)(v & 0xFFFFFu);
            y = (int)(v >> 20);
        }
        gc_encode_piece<false, CPW, RAGGED>(g, y, pcm, pcm_pitch, nch, total_samples, seg, coefs, hist1, hist2, adpcm, adpcm_pitch,
                                            seg_state, (const int *)nullptr, rg);
        if (segments <= 1) continue;
        // ---- the seams at this piece's ends
        __threadfence();                               // this workgroup's bytes and piece state are out before it says so
        __syncthreads();
        if (threadIdx.x == 0) {
            // (pieces past the end of the group's longest channel do not exist: nobody waits for them)
            const int total_wg = RAGGED ? rg.length[rg.order[g * CS]] : total_samples;
            auto exists = [&](int piece) { return piece < segments && seg.first(piece) * 14 < total_wg; };
            int at_start = 0, at_end = 0;
            if (exists(y)) {
                if (y >= 1 && atomicAdd(&seam_count[(int64_t)(y - 1) * groups + g], 1) == 1) at_start = y;
                if (exists(y + 1) && atomicAdd(&seam_count[(int64_t)y * groups + g], 1) == 1) at_end = y + 1;
            }
            s_seam[0] = at_start;
            s_seam[1] = at_end;
        }
        __syncthreads();
        const int seam_a = s_seam[0], seam_b = s_seam[1];
        if ((seam_a | seam_b) != 0) {
            __threadfence();                           // the other workgroup's stores, before anything of them is read
            const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
            if (wave < SW) {
                const int slot = g * CS + wave * CPW + (lane >> 3);
                if (seam_a)
                    seam_piece<8>(slot, seam_a, lane, pcm, pcm_pitch, nch, total_samples, seg, coefs, adpcm, adpcm_pitch, seg_state,
                               first_open, seam_flag, seam_end, force_open, rg);
                if (seam_b)
                    seam_piece<8>(slot, seam_b, lane, pcm, pcm_pitch, nch, total_samples, seg, coefs, adpcm, adpcm_pitch, seg_state,
                               first_open, seam_flag, seam_end, force_open, rg);
            }
        }
    }
}

// Round 15: the order of the self-served queue on uniform batches (gc_plan8.hpp: plan8_slow_channel, plan8_slow_order) from
// the coefficients where they are -- on the device, on the encode's stream, never synchronised to the host:
// order[0 .. S) = the flagged groups of eight, ascending, order[S .. groups8) = the others, order[groups8] = S.
// Behind it a flag per group, order[groups8 + 1 + g] (round 16: flagged groups keep the coarse tail, plan_encode_pieces_on).
//
// Round 16: ONE launch in front of the self-served kernel does this and what three memsets did -- the queue's head with the
// seams' counters and words behind it (`zero`, zero_ints), the channels' records (`token_row`, nch) and first_open (nch x
// SEAM_NONE).  The table was one wave with 64 dependent loads per lane (127.7 us at 4096 channels); here workgroup 0 takes a
// lane per (group, predictor), 128 groups at a time, leaves the flags, and orders them with one scan.  Every workgroup
// shares the fills.
constexpr int PROLOGUE_THREADS = 1024;
__global__ __launch_bounds__(PROLOGUE_THREADS) void gc_self_served_prologue_kernel(
    const int16_t *__restrict__ coefs, int nch, int groups8, int *__restrict__ order, int *__restrict__ zero, int64_t zero_ints,
    int *__restrict__ token_row, int *__restrict__ first_open)
{
    const int64_t step = (int64_t)gridDim.x * PROLOGUE_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * PROLOGUE_THREADS + threadIdx.x; i < zero_ints; i += step) zero[i] = 0;
    for (int64_t i = (int64_t)blockIdx.x * PROLOGUE_THREADS + threadIdx.x; i < nch; i += step) {
        token_row[i] = 0;
        first_open[i] = SEAM_NONE;
    }
    if (blockIdx.x != 0 || order == nullptr) return;
    __shared__ int s_wave[PROLOGUE_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int *flag = order + groups8 + 1;
    // the flags: a lane per (group, predictor), a wave holds eight groups
    for (int base = 0; base < groups8; base += PROLOGUE_THREADS / 8) {
        const int g = base + (t >> 3), pr = t & 7;
        bool slow = false;
        if (g < groups8)
            for (int sl = 0; sl < PLAN8_SLOTS; sl++) {
                const int ch = g * PLAN8_SLOTS + sl;
                if (ch < nch) slow = plan8_slow_predictor(coefs[(int64_t)ch * 16 + 2 * pr], coefs[(int64_t)ch * 16 + 2 * pr + 1]) || slow;
            }
        const unsigned long long m = __ballot(slow);
        if (g < groups8 && pr == 0) flag[g] = ((m >> (lane & 56)) & 0xFFull) != 0 ? 1 : 0;
    }
    __syncthreads();                                    // (this workgroup's own stores: visible to it from here on)
    // the order: every thread a run of consecutive groups, an exclusive scan of the runs' counts
    const int run = (groups8 + PROLOGUE_THREADS - 1) / PROLOGUE_THREADS;
    const int g0 = imin(t * run, groups8), g1 = imin(g0 + run, groups8);
    int mine = 0;
    for (int g = g0; g < g1; g++) mine += flag[g];
    int inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < PROLOGUE_THREADS / 64; w++) {
        const int c = s_wave[w];
        before += w < wave ? c : 0;
        total += c;
    }
    int s = before + inc - mine;                        // flagged groups below g0
    for (int g = g0; g < g1; g++) {
        const int f = flag[g];
        order[f ? s : total + (g - s)] = g;
        s += f;
    }
    if (t == 0) order[groups8] = total;
}
// how many workgroups: one per 16 KiB of fills, at most 64
static int prologue_workgroups(int64_t zero_ints, int nch)
{
    const int64_t want = (zero_ints + 2 * (int64_t)nch + 4 * PROLOGUE_THREADS - 1) / (4 * PROLOGUE_THREADS);
    return want < 1 ? 1 : want > 64 ? 64 : (int)want;
}
// (test-only exports, include/vgaudio_hip_testing.h)
extern "C" int vga_testing_gc_slow_order_host(const int16_t *coefs, int nch, int *order)
{
    if (!coefs || !order || nch <= 0) return -1;
    const int groups8 = (nch + PLAN8_SLOTS - 1) / PLAN8_SLOTS;
    std::vector<unsigned char> flagged((size_t)groups8, 0);
    for (int ch = 0; ch < nch; ch++)
        if (plan8_slow_channel(coefs + (int64_t)ch * 16)) flagged[(size_t)(ch / PLAN8_SLOTS)] = 1;
    return plan8_slow_order(flagged.data(), groups8, order);
}
// The prologue on buffers of its own, every byte of them 0xFF beforehand: order_flags = the table, S and the flags
// (2 * groups8 + 1), *bad_words = the words of the fills that do not hold what the memsets left.  Returns S, or -1.
extern "C" int vga_testing_gc_prologue_device(const void *d_coefs, int nch, int zero_ints, int *order_flags, int *bad_words)
{
    if (!d_coefs || !order_flags || nch <= 0 || zero_ints < 0) return -1;
    const int groups8 = (nch + PLAN8_SLOTS - 1) / PLAN8_SLOTS;
    const size_t n_order = (size_t)2 * groups8 + 1, n_all = n_order + (size_t)zero_ints + 2 * (size_t)nch + 4;   // (+ 4 guard words)
    int *d = nullptr;
    if (hipMalloc(&d, n_all * sizeof(int)) != hipSuccess) return -1;
    std::vector<int> host(n_all);
    bool ok = hipMemset(d, 0xFF, n_all * sizeof(int)) == hipSuccess;
    int *d_zero = d + n_order, *d_token = d_zero + zero_ints, *d_open = d_token + nch;
    if (ok) {
        hipLaunchKernelGGL(gc_self_served_prologue_kernel, dim3(prologue_workgroups(zero_ints, nch)), dim3(PROLOGUE_THREADS), 0, (hipStream_t)0,
                           static_cast<const int16_t *>(d_coefs), nch, groups8, d, d_zero, (int64_t)zero_ints, d_token, d_open);
        ok = hipGetLastError() == hipSuccess && hipMemcpy(host.data(), d, n_all * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d);
    if (!ok) return -1;
    for (size_t i = 0; i < n_order; i++) order_flags[i] = host[i];
    int bad = 0;
    for (size_t i = 0; i < (size_t)zero_ints + (size_t)nch; i++) bad += host[n_order + i] != 0;
    for (int i = 0; i < nch; i++) bad += host[n_order + (size_t)zero_ints + (size_t)nch + (size_t)i] != SEAM_NONE;
    for (int i = 0; i < 4; i++) bad += host[n_all - 4 + (size_t)i] != -1;                  // (nothing written behind the end)
    if (bad_words) *bad_words = bad;
    return host[(size_t)groups8];
}
extern "C" int vga_testing_gc_slow_order_device(const void *d_coefs, int nch, int *order)
{
    if (!d_coefs || !order || nch <= 0) return -1;
    const int groups8 = (nch + PLAN8_SLOTS - 1) / PLAN8_SLOTS;
    std::vector<int> table((size_t)2 * groups8 + 1);
    const int s = vga_testing_gc_prologue_device(d_coefs, nch, 0, table.data(), nullptr);
    if (s < 0) return -1;
    for (int g = 0; g < groups8; g++) order[g] = table[(size_t)g];
    return s;
}

// Round 13: the same queue for the self-served shape (Lay<8, true>): a workgroup is one wave, items are (group of EIGHT
// channel slots, piece) -- gc_plan8.hpp -- and cus x 12 workgroups put three waves on every SIMD, all alike.  The piece
// schedule is the one planned for groups of sixteen, so a channel has the seams it has with the 2 + 1 shape; they close on
// the one wave (seam_piece<8> is per wave).  What was shared through LDS is a readfirstlane.  As there, no wave ever waits
// for another workgroup.
template <bool RAGGED>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) void gc_encode_self_served_kernel(
    const int16_t *__restrict__ pcm, int64_t pcm_pitch, int nch, int total_samples, const std::conditional_t<RAGGED, Pieces, TailPieces> seg,
    const int16_t *__restrict__ coefs, const int16_t *__restrict__ hist1,
    const int16_t *__restrict__ hist2, uint8_t *adpcm, int64_t adpcm_pitch, int16_t *seg_state,
    const Ragged rg, int groups, int items, int segments, int *__restrict__ queue, int *__restrict__ seam_count, int *first_open,
    int *seam_flag, int *seam_end, int force_open, const Handover hand, const int *__restrict__ slow_order, const TailPieces segc,
    int segments_c)
{
    constexpr int CS = PLAN8_SLOTS;
    static_assert(Lay<8, true>::CS == CS && Lay<8, true>::THREADS == 64, "one wave, eight channel slots");
    const int lane = threadIdx.x;
    const uint32_t *host_items = RAGGED ? rg.items : nullptr;
    // (uniform batches: the groups likely to close their seams slowly first, gc_self_served_prologue_kernel)
    const int *order = RAGGED ? nullptr : slow_order;
    const int slow = order ? order[groups] : 0;
    // Round 16 (segments_c > 0): the flagged groups have pieces of their own, segc -- the coarse tail -- and come first in the
    // queue as they did; a group's seams, counters, words and tokens are all indexed by the pieces of ITS schedule, and the
    // channel records stay in the row behind the last piece of the longer of the two
    const bool two = !RAGGED && order != nullptr && segments_c > 0;
    const int front = two ? slow * segments_c : 0;
    if (two) items = front + (groups - slow) * segments;
    const int rec_row = (two && segments_c > segments ? segments_c : segments) - 1;
#ifdef VGA_DEBUG_TIMESTAMPS
    if (lane == 0) g_vga_enc_ts[2 * (blockIdx.x & 32767)] = wall_clock64();
#endif
    for (;;) {
        int item = 0;
        if (lane == 0) item = atomicAdd(queue, 1);
        item = __builtin_amdgcn_readfirstlane(item);
        if (item >= items) {
#ifdef VGA_DEBUG_TIMESTAMPS
            if (lane == 0) g_vga_enc_ts[2 * (blockIdx.x & 32767) + 1] = wall_clock64();
#endif
            return;
        }
        int g, y;
        const bool coarse = two && item < front;
        if (!plan8_item(item, groups, nch, host_items, order, slow, two ? segments_c : segments, g, y)) continue;
        std::conditional_t<RAGGED, Pieces, TailPieces> sg = seg;
        int ns = segments;
        if constexpr (!RAGGED)
            if (coarse) {                               // (wave-uniform: a select of scalars)
                sg = segc;
                ns = segments_c;
            }
        gc_encode_piece<false, 8, RAGGED, true, std::conditional_t<RAGGED, Pieces, TailPieces>>(g, y, pcm, pcm_pitch, nch, total_samples, sg, coefs, hist1, hist2, adpcm, adpcm_pitch,
                                                seg_state, (const int *)nullptr, rg);
        if (ns <= 1) continue;
        // ---- the seams at this piece's ends
        __threadfence();                               // this wave's bytes and piece state are out before it says so
        int at_start = 0, at_end = 0;
        if (lane == 0) {
            // (pieces past the end of the group's longest channel do not exist: nobody waits for them)
            const int total_wg = RAGGED ? rg.length[rg.order[g * CS]] : total_samples;
            auto exists = [&](int piece) { return piece < ns && sg.first(piece) * 14 < total_wg; };
            if (exists(y)) {
                if (y >= 1 && atomicAdd(&seam_count[(int64_t)(y - 1) * groups + g], 1) == 1) at_start = y;
                if (exists(y + 1) && atomicAdd(&seam_count[(int64_t)y * groups + g], 1) == 1) at_end = y + 1;
            }
        }
        const int seam_a = __builtin_amdgcn_readfirstlane(at_start), seam_b = __builtin_amdgcn_readfirstlane(at_end);
        if ((seam_a | seam_b) != 0) {
            __threadfence();                           // the other workgroup's stores, before anything of them is read
            if constexpr (RAGGED) {
                const int slot = g * CS + (lane >> 3);
                if (seam_a)
                    seam_piece<8>(slot, seam_a, lane, pcm, pcm_pitch, nch, total_samples, seg, coefs, adpcm, adpcm_pitch, seg_state,
                               first_open, seam_flag, seam_end, force_open, rg);
                if (seam_b)
                    seam_piece<8>(slot, seam_b, lane, pcm, pcm_pitch, nch, total_samples, seg, coefs, adpcm, adpcm_pitch, seg_state,
                               first_open, seam_flag, seam_end, force_open, rg);
            } else                                     // (uniform batches: with the hand-over of open seams, round 15)
                self_served_seams(g, seam_a, seam_b, lane, groups, ns, rec_row, pcm, pcm_pitch, nch, total_samples, sg, coefs, adpcm,
                                  adpcm_pitch, seg_state, first_open, seam_flag, seam_end, force_open, hand);
        }
    }
}

// The channels with an open seam, piece after piece: where the true history V at the start of piece k is not the one the
// seam launch assumed there (T = seg_state[k - 1]), the piece's bytes are the run from T, so the same seam_run from V next
// to a replay from T finds where the two meet -- as a rule a few frames in, and the chain ends unless a later seam of the
// channel was left open too (then V is that seam's recorded end).  Only a run that is still apart at the very end of a
// stream with a partial last frame goes to the serial repair launch (first_open[channel] = last piece; seg_state gets
// that piece's true start), which also remains the fall-back when the scratch cannot hold the flags.
template <int LPC, class P>
__device__ __forceinline__ void chain_walk(
    const int16_t *__restrict__ pcm, int64_t pcm_pitch, int nch, int total_samples, const P seg, int segments,
    const int16_t *__restrict__ coefs, uint8_t *__restrict__ adpcm, int64_t adpcm_pitch,
    int16_t *__restrict__ seg_state, int *__restrict__ first_open, const int *__restrict__ seam_flag,
    const int *__restrict__ seam_end, int force_open, const Ragged &rg, const int *__restrict__ hand_token,
    const int *__restrict__ hand_v, const int rec_row)
{
    const int lane = threadIdx.x;
    const int pr = LPC == 16 ? (lane >> 1) & 7 : lane & 7;
    const bool lead = (lane & (LPC - 1)) == 0;          // one lane per channel
    const int slot_raw = blockIdx.x * (64 / LPC) + lane / LPC;
    const bool live = slot_raw < nch;
    const int slot = live ? slot_raw : nch - 1;
    const int ch = rg.order ? rg.order[slot] : slot;
    if (rg.order) total_samples = rg.length[ch];        // ragged: per lane from here on
    // Round 15: a channel whose chain the self-served kernel has walked itself (self_served_seams) has a record behind the last
    // piece: nothing of it is walked here -- only first_open is cleared, and the partial last frame encoded when the record
    // carries a V (a run still apart at the very end).  hand_token == nullptr, or a record of 0: as ever.
    const int64_t rec_idx = (int64_t)rec_row * nch + ch;
    const int record = hand_token && live ? hand_token[rec_idx] : 0;
    const bool resolved = record != 0;
    const int mine_raw = live ? first_open[ch] : SEAM_NONE;
    const int mine = resolved ? SEAM_NONE : mine_raw;
    int kmin = mine, kmin_raw = mine_raw;
#pragma unroll
    for (int o = LPC; o < 64; o <<= 1) {
        kmin = imin(kmin, __shfl_xor(kmin, o));
        kmin_raw = imin(kmin_raw, __shfl_xor(kmin_raw, o));
    }
    if (kmin_raw >= segments) return;                   // no open seam among this wave's channels
    const bool tail_left = resolved && (record & HAND_V) != 0 && total_samples % 14 != 0;
    if (live && lead && (mine < segments || tail_left)) atomicAdd(&g_vga_gc_stats[5], 1ull);
    int frames_run = 0;
    const int16_t *src = pcm + (rg.order ? rg.pcm_off[ch] : (int64_t)ch * pcm_pitch);
    uint8_t *dst = adpcm + (rg.order ? rg.adpcm_off[ch] : (int64_t)ch * adpcm_pitch);
    const int16_t *cf = coefs + ch * 16;
    const int c0 = cf[2 * pr], c1 = cf[2 * pr + 1];
    const bool coef_ok = (c0 < 0 ? -c0 : c0) + (c1 < 0 ? -c1 : c1) <= 32767;
    bool have = false;                                  // V differs from what the seam launch assumed at this piece
    int v0 = 0, v1 = 0;                                 // V (x[0], x[1])
    int last_k = 0;
    for (int k = kmin; k < segments; k++) {
        const int64_t f0 = seg.first(k);
        // pieces past a channel's end do not exist (ragged batches: per lane -- such a lane keeps what it had at its
        // own end, for the partial last frame below)
        const bool exists = f0 * 14 < total_samples;
        if (!__any(exists)) break;
        last_k = k;
        const bool is_last = seg.first(k + 1) * 14 >= total_samples || k == segments - 1;
        const int64_t idx = (int64_t)(k - 1) * nch + ch;
        const bool flagged = live && !resolved && exists && seam_flag[idx] != 0;
        const int ended = seam_end[idx];
        const bool ran = live && have && exists;
        bool open = ran;
        int h0 = v0, h1 = v1;
        if (__any(ran)) {
            const int g2 = seg_state[idx * 2], g1 = seg_state[idx * 2 + 1];      // T: what the piece's bytes were encoded from
            if (ran && lead && is_last) {                                     // the repair launch would start here
                seg_state[idx * 2] = (int16_t)v0;
                seg_state[idx * 2 + 1] = (int16_t)v1;
            }
            seam_run<LPC>(src, dst, c0, c1, coef_ok, pr, ch, k, f0, total_samples, seg.frames(k), seg.frames(k), force_open, h0, h1, g2, g1, open, frames_run);
        }
        if (!exists) {
        } else if (ran && open) {                       // still apart at the piece's end: carry on into the next one
            v0 = h0;
            v1 = h1;
        } else if (flagged) {                           // met the run from T, whose own seam ran out of frames: its end is the truth
            have = true;
            v0 = (int)(int16_t)(ended & 0xFFFF);
            v1 = ended >> 16;
        } else
            have = false;
    }
    if (tail_left) {                                    // (the kernel's record: its run arrived at the stream's end with this V)
        const int v = hand_v[rec_idx];
        have = true;
        v0 = (int)(int16_t)(v & 0xFFFF);
        v1 = v >> 16;
    }
    // apart to the very end: only the partial last frame is left to encode from V -- here, by the channel's eight lanes (the
    // serial repair launch that used to take over re-ran the whole last piece: 4.9 ms of a 256-channel encode's 31)
    if (__any(live && have && total_samples % 14 != 0))
        encode_tail_frame<LPC>(src, dst, c0, c1, coef_ok, pr, total_samples, v0, v1, live && have && total_samples % 14 != 0);
    (void)last_k;
    if (live && lead && frames_run) atomicAdd(&g_vga_gc_stats[2], (unsigned long long)frames_run);
    if (live && lead) first_open[ch] = SEAM_NONE;
}
template <int LPC>
__global__ __launch_bounds__(64) void gc_encode_chain_kernel(
    const int16_t *__restrict__ pcm, int64_t pcm_pitch, int nch, int total_samples, const Pieces seg, int segments,
    const int16_t *__restrict__ coefs, uint8_t *__restrict__ adpcm, int64_t adpcm_pitch,
    int16_t *__restrict__ seg_state, int *__restrict__ first_open, const int *__restrict__ seam_flag,
    const int *__restrict__ seam_end, int force_open, const Ragged rg, const int *__restrict__ hand_token,
    const int *__restrict__ hand_v)
{
    chain_walk<LPC, Pieces>(pcm, pcm_pitch, nch, total_samples, seg, segments, coefs, adpcm, adpcm_pitch, seg_state, first_open, seam_flag, seam_end,
                            force_open, rg, hand_token, hand_v, segments - 1);
}
// Round 16, behind the self-served kernel on a uniform batch whose tail descends: a wave here is a group of eight, and a
// flagged group (slow_flag, the prologue kernel's; nullptr: nobody has the flags, one schedule for all) has the coarse
// pieces.  The channels' records are in row rec_row, behind the last piece of the longer schedule.
__global__ __launch_bounds__(64) void gc_encode_chain_tail_kernel(
    const int16_t *__restrict__ pcm, int64_t pcm_pitch, int nch, int total_samples, const TailPieces seg, int segments,
    const int16_t *__restrict__ coefs, uint8_t *__restrict__ adpcm, int64_t adpcm_pitch,
    int16_t *__restrict__ seg_state, int *__restrict__ first_open, const int *__restrict__ seam_flag,
    const int *__restrict__ seam_end, int force_open, const int *__restrict__ hand_token,
    const int *__restrict__ hand_v, int rec_row, const int *__restrict__ slow_flag, const TailPieces segc, int segments_c)
{
    const bool coarse = slow_flag != nullptr && slow_flag[blockIdx.x] != 0;
    chain_walk<8, TailPieces>(pcm, pcm_pitch, nch, total_samples, coarse ? segc : seg, coarse ? segments_c : segments, coefs, adpcm, adpcm_pitch,
                              seg_state, first_open, seam_flag, seam_end, force_open, Ragged{}, hand_token, hand_v, rec_row);
}

// A piece must be longer than the slowest seam of the batch takes to close, or that channel's seams all stay open and the
// chain kernel ends up walking the whole channel serially: channels 64..95 of the synthetic set hold one whose seams need
// ~3000 frames (profiles/r03_b_encode_pieces.log: 96 channels x 60 s in 20.9 ms with 64 pieces of 3214 frames, 60.8 ms
// with 128, 150 ms with 256; without such a channel more pieces only help: 64 channels 6.7 / 5.5 / 4.0 ms).  Round 2 cut
// pieces down to 512 frames.
// Round 15 / 16: this is the floor of every shape whose open seams go to the chain launch -- the plain grid, the 2 + 1 shape,
// ragged batches.  The self-served shape on uniform batches continues an open seam inside its launch (self_served_seams) and
// runs the slow-closing groups first and on coarse pieces, so its other groups' tail pieces go down to
// SELF_SERVED_MIN_TAIL_FRAMES: a short piece there is no longer a seam for the chain launch.
// (3072 until round 4: at 128 channels that made 66 pieces of 3117 frames and the slow channel's seams stayed open -- 33.5 ms
// against 21.2 ms with 64 pieces of 3215)
constexpr int MIN_PIECE_FRAMES = 3584;

// Ragged batches cut their channels into pieces of ONE length (a channel has as many as it reaches into); with a few
// times more workgroups than the chip holds at once, the ones that end early (short channels, short last pieces) make
// room for the rest instead of leaving their SIMDs idle.
constexpr int RAGGED_OVERSUBSCRIPTION = 4;
// Persistent workgroups from one channel group per 32 workgroups on (512 channels on an MI355X): 512 channels 30.3 ms
// against 34.1 for the plain grid with the same 32 pieces, 1024 channels 42.9 against 47.1 (16 pieces) -- the seams run
// inside instead of in a launch of their own; 256 channels and fewer: no difference or slower (25.0 grid, 26.8 persistent;
// profiles/r04_a_encode_persistent.log).  The two-size schedule only from one group per 8 workgroups on (2048 channels):
// below, a channel has to be cut into so many pieces to fill the queue's rounds that its seams cost more than the balance
// gains (1024 channels: 46-62 ms over the schedules tried; profiles/r04_a_encode_schedules.log).
constexpr int PERSISTENT_MIN_GROUPS_FACTOR = 32;
constexpr int PERSISTENT_SCHEDULE_GROUPS_FACTOR = 8;
constexpr int PERSISTENT_ITEMS_PER_WORKGROUP = 4;      // uniform pieces (the test hook's mode 2 without a schedule): items per workgroup
constexpr int PERSISTENT_BIG_ROUNDS = 3;       // a workgroup's share of the frames in this many big items ...
constexpr int PERSISTENT_SMALL_ROUNDS = 2;     // ... followed by this many rounds of short items
constexpr int PERSISTENT_SMALL_FRAMES = 4096;  // ... of this many frames
// The self-served shape (uniform batches): four big rounds and ONE round of short items -- its items are half the size, and
// until round 15 every short piece more was a seam that a slow-closing channel could leave open for the chain launch (one
// sweep on the synthetic set, profiles/r13_encode_ab.log: big,small rounds 4,1 108.4 ms; 2,1 108.8; 2,2 109.3; 3,1 109.4; 5,2 112.8;
// 4,2 114.2; 4,3 116.5; 3,3 117.1; 3,2 115.7-117.7; the 2 + 1 shape's pieces as they are 110.5-110.8; parent 111.4-111.8).
constexpr int SELF_SERVED_BIG_ROUNDS = 4;
constexpr int SELF_SERVED_SMALL_ROUNDS = 1;
// Round 16: since round 15 a seam that outlives its piece is continued inside the launch, so for the self-served shape on
// uniform batches a short piece is no longer a seam for the chain launch, and the tail may descend: rounds of items of
// SELF_SERVED_TAIL_FRAMES, none shorter than SELF_SERVED_MIN_TAIL_FRAMES.  The groups gc_self_served_prologue_kernel flags (their
// seams need 1000-3000 frames) keep the two-size schedule above, tail pieces of SELF_SERVED_COARSE_FRAMES: cut finer,
// every one of their tail seams would stay open and the token walk would re-encode the channel's tail serially.
constexpr int SELF_SERVED_TAIL_ROUNDS[3] = {1, 1, 1};
constexpr int SELF_SERVED_TAIL_FRAMES[3] = {4096, 2048, 1024};
constexpr int SELF_SERVED_MIN_TAIL_FRAMES = 1024;
constexpr int SELF_SERVED_COARSE_FRAMES = 4096;
constexpr int MAX_PIECES = 1024;               // what encode_scratch_bytes() and the ragged item list (capi_gcadpcm_v.hip) are sized for

// The piece schedule (see Pieces, gcadpcm_kernels.hpp).  Plain grid: as many equal pieces as put two encoder waves on
// every SIMD, each at least MIN_PIECE_FRAMES long.  Persistent workgroups: a workgroup's share of the frames in
// PERSISTENT_BIG_ROUNDS big items followed by PERSISTENT_SMALL_ROUNDS rounds of short ones -- with items of one size d
// the workgroups end spread over the last d of the launch (152 ms at configs[1] with 16 pieces of 35 ms: mean life
// 136 ms + d / 2).
// persistent workgroups per compute unit: four.  What the number rests on: the kernel is built for three waves per SIMD
// (amdgpu_waves_per_eu(3, 3), 166 VGPRs), a workgroup is three waves, so four workgroups put exactly two encoder waves and a
// helper on every SIMD -- the wave slots themselves force the even placement.  Round 12 built the kernel for four waves per
// SIMD (128 VGPRs, no scratch instruction in the frame loop; -DVGA_GC_PERSISTENT_WAVES_PER_EU=4,4) and ran it at four and at
// five workgroups: all five start together, but the launch takes 122-125 ms against 113.5 -- most workgroups end near 104 ms,
// a few near 121 (four) or 134 (five): with a free fourth slot nothing keeps three or four encoder waves off one SIMD, and the
// launch lasts as long as its slowest workgroup (LABNOTES 17).
static int persistent_wgs_per_cu()
{
#ifdef VGA_TUNING   // tools/time_corun.py: fewer workgroups leave registers and LDS for another kernel's waves; 5: for a four-waves build
    if (const char *e = std::getenv("VGA_HIP_GC_WGS_PER_CU")) return imin(imax(std::atoi(e), 1), 5);
#endif
    return 4;
}

int plan_encode_pieces(int groups, int frames, int64_t group_frames, bool ragged, bool *persistent_out, Pieces *seg_out, int layout)
{
    return plan_encode_pieces_on(device_cu_count(), groups, frames, group_frames, ragged, persistent_out, seg_out, layout);
}

// (the schedule as a function of the compute-unit count: no device needed, the CPU suite walks it through
// vga_testing_gc_plan_pieces)
int plan_encode_pieces_on(int cus, int groups, int frames, int64_t group_frames, bool ragged, bool *persistent_out, Pieces *seg_out, int layout)
{
    // (two sizes: for the self-served shape on uniform batches the schedule of the groups that keep the coarse tail, which is
    // the only one wherever the tail does not descend)
    TailPieces seg;
    const int segments = plan_encode_tail_pieces_on(cus, groups, frames, group_frames, ragged, persistent_out, &seg, layout, true);
    *seg_out = seg.two();
    return segments;
}

int plan_encode_tail_pieces_on(int cus, int groups, int frames, int64_t group_frames, bool ragged, bool *persistent_out, TailPieces *seg_out,
                               int layout, bool coarse)
{
    // persistent workgroups taking (channel group, piece) items from a queue (gc_encode_persistent_kernel) once the batch
    // has enough channel groups; test hook: 1 = never, 2 = always
    // layout 1, the self-served shape (forced by the test hook or the launcher's choice): it exists as persistent workgroups
    // only, and its queue holds groups of EIGHT channel slots for twelve workgroups per compute unit -- the rounds below are
    // counted in those (`groups` stays the count of groups of sixteen)
    const bool self = layout == 1;
    const int pmode = encoder_persistent_mode();
    const bool persistent = self || (layout != 4 && (pmode == 2 || (pmode == 0 && (ragged || groups * PERSISTENT_MIN_GROUPS_FACTOR >= cus * 4))));
    int segments = cus * 4 / (groups > 0 ? groups : 1);   // = SW encoder waves on every SIMD
    if (persistent && (pmode == 2 || ragged)) segments = (cus * 4 * PERSISTENT_ITEMS_PER_WORKGROUP + groups - 1) / groups;
    if (ragged) {
        // pieces of total / (items wanted) frames for every channel; `segments` = what the longest channel needs
        const int64_t want = (int64_t)cus * 4 * (persistent ? PERSISTENT_ITEMS_PER_WORKGROUP : RAGGED_OVERSUBSCRIPTION);
        int64_t piece = (group_frames + want - 1) / want;
        if (piece < MIN_PIECE_FRAMES) piece = MIN_PIECE_FRAMES;
        segments = (int)((frames + piece - 1) / piece);
    }
    if (segments > frames / MIN_PIECE_FRAMES) segments = frames / MIN_PIECE_FRAMES;
    if (segments < 1) segments = 1;
    if (segments > MAX_PIECES) segments = MAX_PIECES;
    if (encoder_segments_override() > 0) segments = imin(imin(imax(frames / 64, 1), encoder_segments_override()), MAX_PIECES);   // test hook
    TailPieces seg;
    seg.big = (frames + segments - 1) / segments;
    seg.nb = segments;
    seg.small = seg.big;
    // (the test hook's schedule -- the self-served shape on uniform batches only -- applies at any size)
    const int *forced = self && !ragged ? gc_schedule_override() : nullptr;
    if (persistent && encoder_segments_override() <= 0 &&
        (forced || (frames >= 4 * MIN_PIECE_FRAMES && (ragged || groups * PERSISTENT_SCHEDULE_GROUPS_FACTOR >= cus * 4)))) {
        // (ragged batches, mixed-lengths set of bench.py: 4 rounds 151.7 ms, 3: 158.2, 6: 154.5, 8: 169.5; profiles/r04_a_ragged_schedules.log)
        int big_rounds = ragged ? PERSISTENT_BIG_ROUNDS + 1 : PERSISTENT_BIG_ROUNDS;
        // the tail: up to three levels of (rounds of items, frames), descending; `floor`: no tail piece is shorter
        int rounds[3] = {PERSISTENT_SMALL_ROUNDS, 0, 0}, size[3] = {PERSISTENT_SMALL_FRAMES, 0, 0}, count[3] = {-1, -1, -1}, floor = MIN_PIECE_FRAMES;
        if (self && !ragged) {                                                              // (ragged: not swept, kept)
            big_rounds = SELF_SERVED_BIG_ROUNDS;
            rounds[0] = SELF_SERVED_SMALL_ROUNDS;
            if (!coarse) {
                for (int i = 0; i < 3; i++) { rounds[i] = SELF_SERVED_TAIL_ROUNDS[i]; size[i] = SELF_SERVED_TAIL_FRAMES[i]; }
                floor = SELF_SERVED_MIN_TAIL_FRAMES;
            }
        }
#ifdef VGA_TUNING   // tools/build_variants.sh only: the product never reads its schedule from the environment
        if (const char *e = std::getenv("VGA_HIP_GC_SCHEDULE"))
            if (!coarse) std::sscanf(e, "%d,%d,%d,%d,%d,%d,%d", &big_rounds, &rounds[0], &size[0], &rounds[1], &size[1], &rounds[2], &size[2]);
#endif
        if (forced) {                                   // piece counts as given, not rounds
            big_rounds = forced[0];
            floor = forced[7];
            for (int i = 0; i < 3; i++) { count[i] = forced[1 + i]; size[i] = forced[4 + i]; rounds[i] = 0; }
            if (coarse) {                               // one level, no shorter than 4096 frames unless the floor is a test's
                floor = size[0] = imax(size[0], imin(SELF_SERVED_COARSE_FRAMES, 4 * floor));
                count[1] = count[2] = 0;
            }
        }
        big_rounds = imax(big_rounds, 1);
        const int wgs = cus * (self ? PLAN8_WGS_PER_CU : persistent_wgs_per_cu());
        const int queue_groups = self ? 2 * groups : groups;
        const int64_t per_wg = group_frames * (self ? 2 : 1) / wgs + 1;                     // a workgroup's share of the frames
        int64_t tail = 0, tail_share = 0;               // frames of a channel in tail pieces; of a workgroup's share in tail items
        for (int i = 0; i < 3; i++) {
            size[i] = imax(size[i], floor);
            if (i > 0) size[i] = imin(size[i], size[i - 1]);
            const bool given = count[i] >= 0;
            if (!given) count[i] = (rounds[i] * wgs + queue_groups / 2) / queue_groups;     // piece indices that make rounds[i] rounds of items
            if (tail + (int64_t)count[i] * size[i] > frames / 2) count[i] = (int)((frames / 2 - tail) / size[i]);
            tail += (int64_t)count[i] * size[i];
            tail_share += given ? (int64_t)count[i] * size[i] * queue_groups / wgs : (int64_t)rounds[i] * size[i];
        }
        const int small = size[0];
        int big = (int)imax((int)((per_wg - tail_share) / big_rounds), small);
        int nb = (int)((frames - tail + big - 1) / big);
        if (nb < 1) nb = 1;
        if (!ragged) big = (int)((frames - tail + nb - 1) / nb);                            // equal big pieces
        if (big < small) big = small;
        seg = TailPieces{};
        seg.big = big;
        seg.nb = nb;
        seg.small = small;
        // (the last level in use has no end: the pieces cover whatever rounding leaves)
        if (count[2] > 0) { seg.n1 = count[0]; seg.s2 = size[1]; seg.n2 = count[1]; seg.s3 = size[2]; }
        else if (count[1] > 0) { seg.n1 = count[0]; seg.s2 = size[1]; }
        segments = nb + count[0] + count[1] + count[2];
        while (segments > 1 && seg.first(segments - 1) >= frames) segments--;
        if (segments > MAX_PIECES) {
            // A long channel in a batch of few groups: the sizes would need more pieces than the scratch arrays and the
            // host's item list hold.  Equal pieces instead -- the pieces must COVER the channel (nobody encodes what lies
            // past seg.first(segments)).
            segments = MAX_PIECES;
            seg = TailPieces{};
            seg.big = seg.small = (frames + segments - 1) / segments;
            seg.nb = segments;
            while (segments > 1 && seg.first(segments - 1) >= frames) segments--;
        }
    }
    if (seg.first(segments) < frames) {                // (every branch above covers; should one ever not: equal pieces do)
        seg = TailPieces{};
        seg.big = seg.small = (frames + segments - 1) / segments;
        seg.nb = segments;
    }
    *persistent_out = persistent;
    *seg_out = seg;
    return segments;
}

// Which batches the self-served shape encodes when nothing is forced: those of the two-size schedule (from one group of
// sixteen per 8 workgroups of the 2 + 1 shape on: 2048 channels on an MI355X) and ragged batches.  LABNOTES 18.
#ifndef VGA_GC_SELF_SERVED_DEFAULT
#define VGA_GC_SELF_SERVED_DEFAULT 1
#endif
static bool self_served_shape(int layout_hook, int groups16, int cus, bool ragged)
{
    if (layout_hook == 1) return true;
    if (layout_hook != 0 || encoder_persistent_mode() != 0) return false;    // (a forced layout or queue mode means the 2 + 1 shape)
    return VGA_GC_SELF_SERVED_DEFAULT != 0 && (ragged || groups16 * PERSISTENT_SCHEDULE_GROUPS_FACTOR >= cus * 4);
}
// (for the host's plan of a ragged batch, gc_capi.hpp: the layout to hand to plan_encode_pieces)
int encoder_plan_layout(int groups16, bool ragged) { return self_served_shape(encoder_layout(), groups16, device_cu_count(), ragged) ? 1 : 8; }

template <int CPW, bool RAGGED>
static int launch_encode_layout(const int16_t *d_pcm, int64_t pcm_pitch, int nch, int sample_count, const int16_t *d_coefs,
                                const int16_t *d_hist1, const int16_t *d_hist2, uint8_t *d_adpcm, int64_t adpcm_pitch,
                                hipStream_t stream, void *d_scratch, size_t scratch_bytes, const Ragged &rg)
{
    constexpr int CS = Lay<CPW>::CS;
    if (RAGGED) sample_count = rg.max_length;
    if (nch <= 0 || sample_count <= 0) return VGA_OK;
    // two encoder waves per SIMD fill the chip: fewer channels than that are cut into time pieces (each at least
    // MIN_PIECE_FRAMES frames: a seam re-encodes a few dozen as a rule; the ones that take longer than their piece go to
    // the chain launch)
    const int groups = (nch + CS - 1) / CS;
    const int cus = device_cu_count();
    const int frames = (sample_count + 13) / 14;
    // the piece schedule: planned by the host for ragged batches (with the item list), here otherwise
    bool persistent = false;
    Pieces seg;
    int segments;
    const bool want_self = CPW == 8 && self_served_shape(encoder_layout(), groups, cus, RAGGED);
    if (RAGGED && rg.items) {
        persistent = rg.persistent != 0;
        seg = rg.seg;
        segments = rg.segments;
    } else {
        segments = plan_encode_pieces(groups, frames, RAGGED ? rg.total_frames / CS : (int64_t)groups * frames, RAGGED, &persistent, &seg,
                                      want_self ? 1 : CPW);
    }
    // the self-served shape takes the pieces in groups of eight channel slots (gc_plan8.hpp)
    const bool self = want_self && persistent;
    // Round 16: the self-served kernel on a uniform batch takes its pieces as TailPieces (tseg: the tail may descend); `seg` stays
    // what every other launch reads (with a descending tail nobody does: the repair launch returns before it looks).
    TailPieces tseg, segc;
    int segments_c = 0;
    if (self && !RAGGED) {
        bool p = false;
        segments = plan_encode_tail_pieces_on(cus, groups, frames, (int64_t)groups * frames, false, &p, &tseg, 1, false);
        seg = tseg.two();
    }
    const Plan8 p8 = self ? plan_groups_of_eight(cus, nch, segments, RAGGED && rg.items ? rg.n_items : -1) : Plan8{};
    const int seam_groups = self ? p8.groups : groups;
    AsyncBuf scratch;                                  // freed (stream-ordered) on every exit path
    int16_t *seg_state = nullptr;
    int *first_open = nullptr, *seam_flag = nullptr, *seam_end = nullptr, *queue = nullptr, *seam_count = nullptr;
    // open seams handed on inside the self-served kernel (self_served_seams): uniform batches; the test hook switches it off
    // Round 16: the groups the order table flags keep the coarse tail (plan_encode_tail_pieces_on); `rows`: the pieces of the
    // longer of the two schedules, what the scratch arrays are sized for.  Without the hand-over nobody has the flags: one schedule.
    const bool handover = self && !RAGGED && segments > 1 && !gc_seam_handover_off();
    if (handover) {
        bool p = false;
        segments_c = plan_encode_tail_pieces_on(cus, groups, frames, (int64_t)groups * frames, false, &p, &segc, 1, true);
        if (segments_c == segments && segc.same_as(tseg)) segments_c = 0;     // (nothing to tell apart)
    }
    const bool tail_chain = self && !RAGGED && (segments_c > 0 || !tseg.two_sizes());
    const int rows = imax(segments, segments_c);
    Handover hand;
    int *slow_order = nullptr;
    if (segments > 1 || persistent) {
        const size_t state_bytes = segments > 1 ? (size_t)round_up((int64_t)rows * nch * 2 * (int64_t)sizeof(int16_t), 16) : 0;
        const size_t open_bytes = (size_t)round_up((int64_t)nch * (int64_t)sizeof(int), 16);
        const size_t count_bytes = persistent && segments > 1 ? (size_t)round_up((int64_t)(rows - 1) * seam_groups * (int64_t)sizeof(int), 16) : 0;
        // (the hand-over: a word per seam and group behind seam_count's, then a token and a V per piece and channel)
        const size_t order_bytes = handover ? (size_t)round_up((int64_t)(2 * seam_groups + 1) * (int64_t)sizeof(int), 16) : 0;   // (gc_self_served_prologue_kernel's table and flags)
        const size_t need = 3 * state_bytes + open_bytes + 16 + count_bytes + (handover ? count_bytes + 2 * state_bytes + order_bytes : 0);
        // the caller's scratch when it brought one (the host pipeline: hipMallocAsync next to busy copy streams stalled
        // its launching thread for up to 300 ms per call), a stream-ordered allocation otherwise
        unsigned char *base = static_cast<unsigned char *>(d_scratch);
        if (!base || scratch_bytes < need) {
            VGA_HIP_TRY(scratch.alloc(need, stream));
            base = scratch.as<unsigned char>();
        }
        seam_flag = reinterpret_cast<int *>(base + state_bytes);
        seam_end = reinterpret_cast<int *>(base + 2 * state_bytes);
        first_open = reinterpret_cast<int *>(base + 3 * state_bytes);
        queue = reinterpret_cast<int *>(base + 3 * state_bytes + open_bytes);
        // (with the hand-over all the fills below are the prologue kernel's, one launch: gc_self_served_prologue_kernel)
        if (segments > 1) {
            seg_state = reinterpret_cast<int16_t *>(base);
            if (!handover) VGA_HIP_TRY(fill_no_open_seams(first_open, nch, stream));
        } else
            seg_state = nullptr;
        seam_count = queue + 4;
        if (persistent && !handover) VGA_HIP_TRY(hipMemsetAsync(queue, 0, 16 + count_bytes, stream));    // the queue's head and every seam's counter
        if (handover) {
            unsigned char *words = base + 3 * state_bytes + open_bytes + 16 + count_bytes;
            hand.word = reinterpret_cast<int *>(words);
            hand.token = reinterpret_cast<int *>(words + count_bytes);
            hand.v = reinterpret_cast<int *>(words + count_bytes + state_bytes);
            slow_order = reinterpret_cast<int *>(words + count_bytes + 2 * state_bytes);
            // (the channels' records, the row behind the last piece: "not walked" unless the kernel says otherwise)
            if constexpr (CPW == 8 && !RAGGED) {
                const int64_t zero_ints = (int64_t)(16 + 2 * count_bytes) / (int64_t)sizeof(int);    // the queue's head, every seam's counter and word
                hipLaunchKernelGGL(gc_self_served_prologue_kernel, dim3(prologue_workgroups(zero_ints, nch)), dim3(PROLOGUE_THREADS), 0, stream,
                                   d_coefs, nch, p8.groups, slow_order, queue, zero_ints, hand.token + (size_t)(rows - 1) * nch, first_open);
                VGA_HIP_TRY(hipGetLastError());
            }
        }
    }
    if (self) {
        if constexpr (CPW == 8) {
            std::conditional_t<RAGGED, Pieces, TailPieces> self_seg;
            if constexpr (RAGGED) self_seg = seg; else self_seg = tseg;
            hipLaunchKernelGGL((gc_encode_self_served_kernel<RAGGED>), dim3(p8.wgs), dim3(Lay<8, true>::THREADS), 0, stream, d_pcm, pcm_pitch,
                               nch, sample_count, self_seg, d_coefs, d_hist1, d_hist2, d_adpcm, adpcm_pitch, seg_state, rg, p8.groups, p8.items,
                               segments, queue, seam_count, first_open, seam_flag, seam_end, force_open_seams(), hand, (const int *)slow_order, segc,
                               segments_c);
        }
    } else if (persistent) {
        const int items = RAGGED && rg.items ? rg.n_items : groups * segments;
        const int wgs = imin(items, cus * persistent_wgs_per_cu());
        if constexpr (CPW == 8)
            hipLaunchKernelGGL((gc_encode_persistent_kernel<CPW, RAGGED>), dim3(wgs), dim3(ENC_THREADS), 0, stream, d_pcm, pcm_pitch, nch,
                               sample_count, seg, d_coefs, d_hist1, d_hist2, d_adpcm, adpcm_pitch, seg_state, rg, groups, segments, queue,
                               seam_count, first_open, seam_flag, seam_end, force_open_seams());
    } else
        hipLaunchKernelGGL((gc_encode_kernel<false, CPW, RAGGED>), dim3(groups, segments), dim3(ENC_THREADS), 0, stream, d_pcm, pcm_pitch, nch,
                           sample_count, seg, d_coefs, d_hist1, d_hist2, d_adpcm, adpcm_pitch, seg_state,
                           (const int *)nullptr, rg);
    VGA_HIP_TRY(hipGetLastError());
    if (segments > 1) {
        if (!persistent) {                             // (the persistent workgroups close the seams themselves)
            // The seam runs in the lane-per-candidate layout (seam_run<16>) where the launch lasts as long as its slowest seam
            // and a batch is likely to hold one: more than 64 channels of the encoder's CPW = 4 layout.  Measured at 60 s per
            // channel (profiles/r06_m_channel_scaling.log): 96 channels 18.3 -> 16.4 ms (seam launch 4.8 + chain 4.6 ms, the
            // synthetic set's slow-closing tone among them), 256: 23.2 -> 23.4, 384: 25.5 -> 25.1; 1 / 8 / 64 channels lose
            // 0.2-0.4 ms (3.06 -> 3.47, 3.48 -> 3.84, 6.79 -> 7.00) and keep the lane-per-predictor runs.
#ifdef VGA_GC_SEAM16_ALWAYS                                          // (debug builds)
            const bool wide = CPW == 4;
#else
            const bool wide = CPW == 4 && nch > 64;
#endif
            if (wide)
                hipLaunchKernelGGL(gc_encode_seam_kernel<16>, dim3((nch + 3) / 4, segments - 1), dim3(64), 0, stream, d_pcm, pcm_pitch, nch,
                                   sample_count, seg, d_coefs, d_adpcm, adpcm_pitch, seg_state, first_open, seam_flag, seam_end,
                                   force_open_seams(), rg);
            else
                hipLaunchKernelGGL(gc_encode_seam_kernel<8>, dim3((nch + 7) / 8, segments - 1), dim3(64), 0, stream, d_pcm, pcm_pitch, nch,
                                   sample_count, seg, d_coefs, d_adpcm, adpcm_pitch, seg_state, first_open, seam_flag, seam_end,
                                   force_open_seams(), rg);
            VGA_HIP_TRY(hipGetLastError());
        }
        // the seams that were still open at the end of their piece, chained piece after piece (none: every wave returns)
        if (tail_chain)                                // (the self-served shape on a uniform batch whose tail descends)
            hipLaunchKernelGGL(gc_encode_chain_tail_kernel, dim3((nch + 7) / 8), dim3(64), 0, stream, d_pcm, pcm_pitch, nch, sample_count, tseg,
                               segments, d_coefs, d_adpcm, adpcm_pitch, seg_state, first_open, seam_flag, seam_end, force_open_seams(),
                               (const int *)hand.token, (const int *)hand.v, rows - 1,
                               (const int *)(segments_c > 0 ? slow_order + seam_groups + 1 : nullptr), segc, segments_c);
        else
#ifdef VGA_GC_SEAM16_ALWAYS
        if (CPW == 4)
#else
        if (CPW == 4 && nch > 64)
#endif
            hipLaunchKernelGGL(gc_encode_chain_kernel<16>, dim3((nch + 3) / 4), dim3(64), 0, stream, d_pcm, pcm_pitch, nch, sample_count,
                               seg, segments, d_coefs, d_adpcm, adpcm_pitch, seg_state, first_open, seam_flag, seam_end,
                               force_open_seams(), rg, (const int *)hand.token, (const int *)hand.v);
        else
            hipLaunchKernelGGL(gc_encode_chain_kernel<8>, dim3((nch + 7) / 8), dim3(64), 0, stream, d_pcm, pcm_pitch, nch, sample_count,
                               seg, segments, d_coefs, d_adpcm, adpcm_pitch, seg_state, first_open, seam_flag, seam_end,
                               force_open_seams(), rg, (const int *)hand.token, (const int *)hand.v);
        VGA_HIP_TRY(hipGetLastError());
        // repair: the same encoder, serially over the last piece, for a channel the chain could not finish (a partial
        // last frame after a run that never met; none: every workgroup returns)
        hipLaunchKernelGGL((gc_encode_kernel<true, CPW, RAGGED>), dim3(groups, 1), dim3(ENC_THREADS), 0, stream, d_pcm, pcm_pitch, nch, sample_count,
                           seg, d_coefs, d_hist1, d_hist2, d_adpcm, adpcm_pitch, seg_state, (const int *)first_open, rg);
        VGA_HIP_TRY(hipGetLastError());
    }
    return VGA_OK;
}

// upper bound of what launch_encode wants as scratch for nch channels (1024 pieces x (state, flag, end) + 4 B per channel, + alignment)
// (+ the persistent kernels' queue and seam counters: 4 B per channel group and seam)
// (groups of eight, the self-served shape: 4 B per seam and 8 channels = 512 B per channel)
// (the hand-over of the self-served shape: a token and a V per piece and channel, 8 B, and a second word per seam and group)
size_t encode_scratch_bytes(int nch) { return (size_t)(nch > 0 ? nch : 0) * (1024 * 20 + 4 + 1024 + 1) + 8192 + 32; }

int launch_encode(const int16_t *d_pcm, int64_t pcm_pitch, int nch, int sample_count, const int16_t *d_coefs,
                  const int16_t *d_hist1, const int16_t *d_hist2, uint8_t *d_adpcm, int64_t adpcm_pitch,
                  hipStream_t stream, void *d_scratch, size_t scratch_bytes, const Ragged *rg)
{
    if (rg)                                            // ragged batches: the (channel, predictor) layout only
        return launch_encode_layout<8, true>(d_pcm, 0, nch, 0, d_coefs, d_hist1, d_hist2, d_adpcm, 0, stream, d_scratch,
                                             scratch_bytes, *rg);
    // The wave layout: (channel, predictor) lanes run the two scale candidates of a pair back to back -- fewer instructions
    // per channel, the layout of every batch that fills the chip (and of the persistent workgroups).  A batch too small for
    // those is a few hundred workgroups on 1024 SIMDs, each alone on its SIMD and as fast as its own instruction stream: with a
    // lane per (channel, predictor, candidate) that stream is half as long per frame and there are twice the workgroups
    // (60 s channels: 1 channel 3.0 ms against 4.8, 96: 18.5 / 21.8, 256: 23.3 / 25.7, 384: 25.5 / 31.5, 512: 28.9 / 28.2 with
    // persistent workgroups; tools/time_layouts_small.py).
    int layout = encoder_layout();
    if (layout == 0)                                   // (the test hook that forces persistent workgroups needs their layout)
        layout = encoder_persistent_mode() != 2 && ((nch + 15) / 16) * PERSISTENT_MIN_GROUPS_FACTOR < device_cu_count() * 4 ? 4 : 8;
    if (layout == 4)
        return launch_encode_layout<4, false>(d_pcm, pcm_pitch, nch, sample_count, d_coefs, d_hist1, d_hist2, d_adpcm, adpcm_pitch, stream,
                                              d_scratch, scratch_bytes, Ragged{});
    return launch_encode_layout<8, false>(d_pcm, pcm_pitch, nch, sample_count, d_coefs, d_hist1, d_hist2, d_adpcm, adpcm_pitch, stream,
                                          d_scratch, scratch_bytes, Ragged{});
}

}  // namespace gc
}  // namespace vga
