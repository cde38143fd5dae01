// adx_kernels.hip -- CRI ADX 4-bit ADPCM encode / decode for gfx950.
//
// Replaces VGAudio/Codecs/CriAdx/CriAdxCodec.cs:56-147 (Encode, EncodeFrame, CalculateScale,
// ScaleShortToNibble) and :9-54 (Decode), bit-exact (C# int32 wrap-around via -fwrapv, the one
// f64 multiply `(int)(rawDistance * gain)` kept literally, no FMA contraction).
//
// ADX is a serial recurrence per channel with a single predictor and no retry loop, so the
// decomposition is lane = channel (the reference's Parallel.For over channels,
// Formats/CriAdx/CriAdxFormat.cs:67 / :37).  Frame size is a run-time parameter.
#include "common.hpp"
#include "adx_kernels.hpp"
#include "adx_device.hpp"
#include "seams.hpp"

#include <cstdlib>
#include <type_traits>

namespace vga {
namespace adx {

// Encode (CriAdxCodec.cs:56-105) and Decode (:9-54) for any frame size and padding: lane = channel, the rows at a pitch
// (adx_encode_channel / adx_decode_channel, adx_device.hpp).
__global__ __launch_bounds__(64) void adx_encode_kernel(
    const int16_t *__restrict__ pcm, int64_t pcm_pitch, int nch, int pcm_length, AdxDeviceParams p,
    uint8_t *__restrict__ out, int64_t out_pitch, int16_t *__restrict__ history_out)
{
    const int ch = blockIdx.x * 64 + threadIdx.x;
    if (ch >= nch) return;
    adx_encode_channel(pcm + (int64_t)ch * pcm_pitch, pcm_length, p, reinterpret_cast<uint16_t *>(out + (int64_t)ch * out_pitch),
                       history_out ? history_out + ch : nullptr);
}

__global__ __launch_bounds__(64) void adx_decode_kernel(
    const uint8_t *__restrict__ adpcm, int64_t in_pitch, int nch, int sample_count, AdxDeviceParams p,
    int16_t *__restrict__ pcm, int64_t pcm_pitch, int *__restrict__ status)
{
    const int ch = blockIdx.x * 64 + threadIdx.x;
    if (ch >= nch) return;
    adx_decode_channel(adpcm + (int64_t)ch * in_pitch, sample_count, p, pcm + (int64_t)ch * pcm_pitch, status);
}

// ---------------------------------------------------------------- 18-byte frames: lane = channel, one wave per 64 channels and piece
// CriAdxCodec.Decode (CriAdxCodec.cs:9-54) for the common shape (18-byte frames, no padding), without helper waves.
// Time segments (blockIdx.y), as in gc_decode_kernel.hip: a channel's stream is cut into pieces of `seg_frames` frames (an
// even number: frame parity decides the load alignment) decoded side by side, every piece but the first from a guessed
// history -- (0, 0), 512 frames before the piece (see the warm-up below); adx_decode_fs18_fixup_kernel then closes the seams.
// A lane reads its own frames two at a time (36 contiguous bytes from a dword boundary, the next pair in flight during
// this one), takes the nibbles out of the loaded dwords with one v_bfe_i32 each, runs the recurrence (:36-45) and hands
// its samples to the wave's LDS block, from which they leave as whole lines (below).
// Rounds 1-2 had a serial wave + three helper waves here (the helpers unpacked scale * nibble into LDS tiles and wrote the
// samples out): 100 KB of LDS per 64 channels, so one workgroup per CU, four pieces per channel at 4096 channels and a
// quarter of the SIMDs busy -- 15.1 ms at configs[2].  This kernel: 8.0 ms, of which the recurrence is free: a build that
// skips it takes 7.7 ms: the kernel is bound by its stores -- 23.6 GB at 3.0 TB/s, 43 % of what a plain fill reaches on
// this box (tools/bench_fill.py): 65 536 slow sequential streams, one per channel and piece (LABNOTES.md 4.3).
template <bool V4, bool REPAIR>                       // (REPAIR: a name of its own in profiles, as gc_decode_direct_kernel's)
__global__ __launch_bounds__(64) void adx_decode_fs18_direct_kernel(
    const uint8_t *__restrict__ adpcm, int64_t in_pitch, int nch, int total_samples, int seg_frames, AdxDeviceParams p,
    int16_t *__restrict__ pcm, int64_t pcm_pitch, int *__restrict__ status, const int *__restrict__ first_open,
    const int *__restrict__ slow_seams)
{
    const int ch_raw = blockIdx.x * 64 + threadIdx.x;
    const bool live = ch_raw < nch;
    const int ch = live ? ch_raw : nch - 1;
    // REPAIR launch (round 5, as gc_decode_direct_kernel's): many seams of the batch would not close
    // (tones, clipped waves); the wave decodes its 64 channels again as one piece from the first piece any of them left
    // open, from the samples before it.
    constexpr bool repair = REPAIR;
    int repair_piece = 0;
    if (repair) {
        if (slow_seams[0] < slow_seams[1]) return;                        // few: adx_decode_fs18_tail_kernel has them
        const int k = wave_first_open(first_open, live, ch);
        if (!is_open(k)) return;
        repair_piece = k;
    }
    const int64_t first_frame = (int64_t)(repair ? repair_piece : (int)blockIdx.y) * seg_frames;   // even (seg_frames is)
    if (repair) seg_frames = 0x7fffff00 / 32;                              // ... to the end of the stream
    if (first_frame * 32 >= total_samples) return;
    const int sample_count = (int)((int64_t)total_samples - first_frame * 32 < (int64_t)seg_frames * 32
                                       ? (int64_t)total_samples - first_frame * 32 : (int64_t)seg_frames * 32);
    const int frame_count = (sample_count + 31) / 32;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(adpcm + (int64_t)ch * in_pitch + first_frame * 18);
    int16_t *dst = pcm + (int64_t)ch * pcm_pitch + first_frame * 32;
    int hist1 = blockIdx.y > 0 ? 0 : p.history, hist2 = hist1;             // later pieces: the guess (0, 0)
    if (repair) {
        hist1 = dst[-1];
        hist2 = dst[-2];
    }
    bool bad = false;
    // Output: lane = channel holds one 64-byte line per frame; stored as it is, every store instruction would touch 64
    // rows, 16 bytes of each (measured: 20 of the kernel's 23 ms).  TURN frames of every channel (TURN x 64 contiguous
    // bytes of its row) are collected in the wave's own LDS and written out turned: LPR lanes per row, 64 / LPR rows per
    // store instruction.  One wave per workgroup and LDS operations of a wave complete in order: no barrier.
    constexpr int TURN = 2;                                                // (4 and 8 frames per block: no faster)
    constexpr int LPR = TURN * 4;                                          // lanes (16 bytes each) per row
    constexpr int RPI = 64 / LPR;                                          // rows per store instruction
    __shared__ int4 s_turn[64 * (LPR + 1)];                                // rows one int4 apart from a multiple of 8: no conflicts
    const int lane = threadIdx.x;
    // Rows past the last channel: those lanes decode channel nch - 1 again (`ch` above), so their lines ARE that channel's
    // and go to its row once more -- which keeps the stores unconditional: behind a branch hipcc can no longer count them
    // and waits for ALL outstanding stores before it touches the prefetched frames (s_waitcnt vmcnt counts both).
    auto turned_row = [&](int i) {
        const int c = blockIdx.x * 64 + lane / LPR + RPI * i;
        return pcm + (int64_t)(c < nch ? c : nch - 1) * pcm_pitch + first_frame * 32 + (lane % LPR) * 8;
    };
    // one frame whose 18 bytes are w[0 .. 4] (adx_decode_frame), and where its samples go
    auto decode_frame = [&](const uint32_t (&w)[5], auto mode_tag, int frame, int valid, int skip = 0) {
        constexpr int MODE = decltype(mode_tag)::value;          // 0: whole frame, stored turned; 1: whole frame, stored by its lane; 2: partial
                                                                 // 4: samples [skip, valid) only: the frame in which a padded stream's samples begin
        int o[32];
        adx_decode_frame<V4, MODE == 4>(w, p, hist1, hist2, bad, o, skip);
        if (MODE == 0) {
            int4 *mine = s_turn + lane * (LPR + 1) + (frame % TURN) * 4;
#pragma unroll
            for (int q = 0; q < 4; q++) mine[q] = adx_pack8(o, q);
            if (frame % TURN == TURN - 1) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int i = 0; i < LPR; i++)            // read, wait, store -- one at a time: LPR stores back to back were
                    adx_store16(turned_row(i) + (int64_t)(frame - (TURN - 1)) * 32,                       // 5 ms slower
                                s_turn[(lane / LPR + RPI * i) * (LPR + 1) + lane % LPR]);
                asm volatile("" ::: "memory");
            }
        } else if (MODE == 1) {
            if (live) adx_store_frame(dst + (int64_t)frame * 32, o);
        } else if ((MODE == 2 || MODE == 4) && live) {
            int16_t *d = dst + (int64_t)frame * 32;
#pragma unroll
            for (int s2 = 0; s2 < 32; s2++)
                if (s2 >= skip && s2 < valid) d[s2] = (int16_t)o[s2];
        }
    };
    // ---- Round 6: the head of a PADDED stream (launch_decode: `pcm` arrives moved back by the padding and total_samples counts
    // it, as in the encoder): the frames before the one the padding ends in are not read at all, that frame is decoded from
    // its nibble p.padding % 32 on, from the stream's start history (CriAdxCodec.cs:21-33); a frame at a time up to the first
    // even frame behind it, where the pairs below take over.
    int head_frames = 0;
    if (!repair && blockIdx.y == 0 && p.padding > 0) {
        const int fp = p.padding / 32;
        head_frames = fp + 1 + ((fp + 1) & 1);
        if (head_frames > frame_count) head_frames = frame_count;
#pragma unroll 1
        for (int i = fp; i < head_frames; i++) {
            uint32_t w[5];
            adx_load_frame(src, i, w);
            const int valid = min(32, sample_count - i * 32);
            decode_frame(w, std::integral_constant<int, 4>{}, i, valid, i == fp ? p.padding % 32 : 0);
        }
    }
    // ---- warm-up of a later piece
    if (!repair && blockIdx.y > 0) adx_decode_warm_up<V4>(src, first_frame, p, hist1, hist2, bad);
    // ---- whole pairs of full frames: 36 bytes from a dword boundary, the next pair's loads in flight meanwhile
    const int full_pairs = (sample_count / 32) / TURN * (TURN / 2);          // whole blocks of TURN full frames
    uint32_t cur[9], nxt[9];
    const int first_pair = head_frames / 2;                                // (0 but for a padded stream's first piece)
    {
        const uint32_t *f = src + (int64_t)min(first_pair, max(full_pairs - 1, 0)) * 9;   // the first pair (or, with no pair at all,
        const int nq = full_pairs > 0 ? 9 : 5;                             // five dwords of the row's first frame: unused)
#pragma unroll
        for (int q = 0; q < 9; q++) cur[q] = q < nq ? f[q] : 0u;
        // the first pair is waited for HERE: left to the loop header, the wait would also sit on the back edge, where it
        // means "every store of the pair before has completed"
#pragma unroll
        for (int q = 0; q < 9; q++) asm volatile("" : "+v"(cur[q]));
    }
#pragma unroll 1
    for (int k = first_pair; k < full_pairs; k++) {
        const uint32_t *f = src + (int64_t)min(k + 1, full_pairs - 1) * 9;
#pragma unroll
        for (int q = 0; q < 9; q++) nxt[q] = f[q];
        uint32_t a[5], b[5];
        adx_split_pair(cur, a, b);
        decode_frame(a, std::integral_constant<int, 0>{}, 2 * k, 32);
        decode_frame(b, std::integral_constant<int, 0>{}, 2 * k + 1, 32);
#pragma unroll
        for (int q = 0; q < 9; q++) cur[q] = nxt[q];
    }
    // ---- what is left of the piece: fewer than TURN full frames and a partial one
#pragma unroll 1
    for (int i = max(2 * full_pairs, head_frames); i < frame_count; i++) {
        uint32_t w[5];
        adx_load_frame(src, i, w);
        const int valid = min(32, sample_count - i * 32);
        if (valid == 32) decode_frame(w, std::integral_constant<int, 1>{}, i, 32);
        else decode_frame(w, std::integral_constant<int, 2>{}, i, valid);
    }
    if (bad && live && status) atomicOr(status, 1);
}

// The ADX side of the seam protocol (seams.hpp): lane = channel at the dense pitch.  own_samples (the ragged entry point's
// length buckets, capi_adx.hip): the channel is a shorter stream padded to total_samples.
template <bool V4>
struct AdxDecodeSeams {
    static constexpr int FRAME_SAMPLES = 32, FRAME_BYTES = 18;
    static constexpr int SLOW_SEAM = ADX_DECODE_SLOW_SEAM, SLOW_POLL = 128, TAIL_BUDGET = ADX_DECODE_TAIL_BUDGET;
    static constexpr bool HAS_OWN = true;
    const uint8_t *adpcm; int64_t in_pitch; AdxDeviceParams p; int16_t *pcm; int64_t pcm_pitch; const int *own_samples;
    const uint8_t *src; int16_t *dst;                                    // (open)
    __device__ int channel(int slot) const { return slot; }
    __device__ int length(int, int total) const { return total; }
    __device__ int64_t own(int ch, int total) const { return own_samples ? (int64_t)own_samples[ch] : (int64_t)total; }
    __device__ void open(int ch)
    {
        src = adpcm + (int64_t)ch * in_pitch;
        dst = pcm + (int64_t)ch * pcm_pitch;
    }
    __device__ void decode(const uint8_t *fr, int valid, int &h1, int &h2, int16_t *o) const { adx_decode_frame_serial<V4>(fr, p, valid, h1, h2, o); }
};

template <bool V4>
__global__ __launch_bounds__(64) void adx_decode_fs18_fixup_kernel(
    const uint8_t *__restrict__ adpcm, int64_t in_pitch, int nch, int total_samples, int seg_frames, AdxDeviceParams p,
    int16_t *__restrict__ pcm, int64_t pcm_pitch, int *__restrict__ first_open, int *__restrict__ seam_open, int force_open,
    int *__restrict__ slow_seams, const int *__restrict__ own_samples)
{
    seam_fixup(AdxDecodeSeams<V4>{adpcm, in_pitch, p, pcm, pcm_pitch, own_samples}, nch, total_samples, seg_frames, first_open,
               seam_open, force_open, slow_seams);
}

template <bool V4>
__global__ __launch_bounds__(64) void adx_decode_fs18_tail_kernel(
    const uint8_t *__restrict__ adpcm, int64_t in_pitch, int nch, int total_samples, int seg_frames, int segments, AdxDeviceParams p,
    int16_t *__restrict__ pcm, int64_t pcm_pitch, int *__restrict__ first_open, const int *__restrict__ seam_open,
    int force_open, int *__restrict__ slow_seams, const int *__restrict__ own_samples)
{
    seam_tail(AdxDecodeSeams<V4>{adpcm, in_pitch, p, pcm, pcm_pitch, own_samples}, nch, total_samples, seg_frames, segments,
              first_open, seam_open, force_open, slow_seams);
}

// ---------------------------------------------------------------- 18-byte frames: lane = channel, one wave per 64 channels and piece
// CriAdxCodec.Encode / EncodeFrame (:56-147) for the common shape, one wave on its own (no helper waves, no LDS, no barrier).
// Time segments (blockIdx.y), as the decoder above has them: every piece but the first starts from a guessed history -- the
// two INPUT samples before it -- and adx_encode_fs18_fixup_kernel closes the seams afterwards; seg_state[piece][channel] gets
// each piece's final history.  A lane reads its own frames (two at a time: a 128-byte line, the next pair's loads in flight
// during this one) and writes eight frames at a time (144 bytes from a dword boundary).
// Every frame costs the same, so a plain grid with as many waves as the chip holds is balanced: the wave's ~900
// instructions per frame (pre-scan 8 per sample, adx_quantise_step 18) are what it runs at -- configs[2]: 12.1 ms with 32
// pieces per channel, 84 % of the VALU issue slots, 23.6 GB fetched and 11.0 GB written (23.6 and 9.6 GB algorithmic, the
// crumbs included; tools/pmc_adx_encode.sh).  The tiled kernel of rounds 2-4 -- one encoder wave and three helper waves per 64 channels, the
// tiles in LDS, hence two encoder waves per CU -- took 19.7 ms, 17.5 ms with this file's arithmetic.
// Crumbs: 8 bytes per frame and channel in a scratch array [frame][channel] -- what a seam run needs to know about the
// guessed run it replaces (see adx_encode_fs18_fixup_kernel).
// Round 6: PADDED streams (CriAdxFormat.cs:59-62: every looping file whose loop start is not a multiple of the alignment gets
// Padding = alignmentSamples, up to 63 zero samples in front) take these kernels too.  They work in STREAM positions: `pcm`
// arrives moved back by the padding (launch_encode), total_length counts the padding, and a position below p.padding is
// never read: the frames of piece 0 that reach into the padding are loaded a sample at a time -- those lying wholly inside
// it are skipped, their bytes zero (:84-86) -- and nothing else comes near it.  A frame of a padded stream starts at any
// 2-byte boundary, hence the 2-byte alignment of the 16-byte loads (the same global_load_dwordx4 either way).
// REPAIR (round 6, the decoders' scheme): a launch of ONE piece row after the fix-up.  When many seams of the batch stayed open
// to the end of their pieces (a batch of tones or clipped waves: the run from the true history and the guessed one stay one
// LSB apart for good, LABNOTES 8.7) the chained tail kernel would walk every such channel piece after piece with one lane
// (254 ms for 60 s of a 440 Hz tone in every channel).  Here a wave that holds such a channel encodes its 64 channels again as
// ONE piece, from the first piece any of them left open to the end of the stream, from seg_state of the piece before --
// the true history for all 64 (every seam before that piece closed) -- at this kernel's own rate: the serial floor.
template <bool V4, bool EXPONENTIAL, bool REPAIR = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void adx_encode_fs18_direct_kernel(
    const int16_t *__restrict__ pcm, int64_t pcm_pitch, int nch, int total_length, int seg_frames, AdxDeviceParams p,
    uint8_t *__restrict__ out, int64_t out_pitch, int16_t *__restrict__ history_out, int16_t *__restrict__ seg_state,
    uint2 *__restrict__ crumbs, const int *__restrict__ first_open, const int *__restrict__ open_seams, int many)
{
    const int ch = blockIdx.x * 64 + threadIdx.x;
    int k = blockIdx.y;
    if (REPAIR) {
        if (open_seams[0] < many) return;              // few: adx_encode_fs18_tail_kernel has chained them
        const int ko = wave_first_open(first_open, ch < nch, ch);
        if (!is_open(ko)) return;                      // no open seam among this wave's channels
        k = ko;
    }
    const int64_t f0 = (int64_t)k * seg_frames;
    if (ch >= nch || (k > 0 && f0 * 32 >= total_length)) return;
    AdxPitchedRows r{pcm, pcm_pitch, out, out_pitch, nch, total_length, p.padding, nullptr, crumbs};
    r.open(ch);
    int a = 0, b = 0;
    if (REPAIR) {                                      // the true history at the start of piece k
        const int16_t *st = seg_state + r.state(k - 1) * 2;
        a = st[0];
        b = st[1];
    } else if (k > 0) {                                // the guess: the input just before this piece
        a = r.src[f0 * 32 - 2];
        b = r.src[f0 * 32 - 1];
    } else {
        int hist = p.history;
        if (V4 && total_length > 0 && p.padding == 0) { a = b = r.src[0]; hist = a; }    // :69-74
        if (history_out) history_out[ch] = (int16_t)hist;
    }
    adx_encode_piece<V4, EXPONENTIAL, REPAIR>(r, k, seg_frames, p, a, b, seg_state);
}

// The fix-up launch (adx_encode_fixup) over (channel, seam) pairs.  own_frames (the ragged entry points' length buckets,
// capi_adx.hip): channel ch is a shorter stream zero-padded to total_length and only its first own_frames[ch] frames are
// anybody's output.
template <bool V4, bool EXPONENTIAL>
__global__ __launch_bounds__(64) void adx_encode_fs18_fixup_kernel(
    const int16_t *__restrict__ pcm, int64_t pcm_pitch, int nch, int total_length, int seg_frames, int segments, AdxDeviceParams p,
    uint8_t *__restrict__ out, int64_t out_pitch, const int16_t *__restrict__ seg_state, const uint2 *__restrict__ crumbs,
    int *__restrict__ first_open, int *__restrict__ seam_open, int *__restrict__ seam_end, int force_open, int *__restrict__ queue,
    const int *__restrict__ own_frames, int *__restrict__ open_seams)
{
    adx_encode_fixup<V4, EXPONENTIAL>(AdxPitchedRows{pcm, pcm_pitch, out, out_pitch, nch, total_length, p.padding, own_frames,
                                                     const_cast<uint2 *>(crumbs), pcm, out},
                                      seg_frames, segments, p, seg_state, first_open, seam_open, seam_end, force_open, queue, open_seams);
}

// The chained tail (adx_encode_tail): one lane per channel
template <bool V4, bool EXPONENTIAL>
__global__ __launch_bounds__(64) void adx_encode_fs18_tail_kernel(
    const int16_t *__restrict__ pcm, int64_t pcm_pitch, int nch, int total_length, int seg_frames, int segments, AdxDeviceParams p,
    uint8_t *__restrict__ out, int64_t out_pitch, const int16_t *__restrict__ seg_state, const int *__restrict__ first_open,
    const int *__restrict__ seam_open, const int *__restrict__ seam_end, int force_open, const int *__restrict__ own_frames,
    const int *__restrict__ open_seams, int many)
{
    const int ch = blockIdx.x * 64 + threadIdx.x;
    if (ch >= nch) return;
    adx_encode_tail<V4, EXPONENTIAL>(AdxPitchedRows{pcm, pcm_pitch, out, out_pitch, nch, total_length, p.padding, own_frames, nullptr}, ch,
                                     seg_frames, segments, p, seg_state, first_open, seam_open, seam_end, force_open, open_seams, many);
}

// The one-wave encoder's pieces: two waves on every SIMD, each piece at least this long (a seam takes 200 frames to close on
// average and 2500 for the longest of configs[2]'s 127 000, tests/host/analysis/adx_seam_stats.c; one still open at the end
// of its piece carries on in the tail kernel).  The fix-up's lanes take seams from a queue: one persistent wave per SIMD
// (profiles/r04_e_adx_parts.log: 512 / 1024 / 2048 waves 5.8 / 5.4 / 6.4 ms).  The pieces' figures are adx_host.hpp's
// ENCODE_* and DECODE_*, which the ragged plan reads too.
constexpr int ADX_FIXUP_WAVES_PER_SIMD = 1;

int launch_encode(const int16_t *d_pcm, int64_t pcm_pitch, int nch, int pcm_length, const AdxDeviceParams &p,
                  uint8_t *d_out, int64_t out_pitch, int16_t *d_history_out, hipStream_t stream, const int *d_own_frames)
{
    if (nch <= 0) return VGA_OK;
    const dim3 grid((nch + 63) / 64), block(64);
    // pcm rows must be 16-byte aligned for the vector loads, output rows 4-byte aligned for the dword stores
    // (and coefficients of the size the reference can produce: adx_quantise_step's 32-bit bound)
    // (padding: at most two frames of it -- CriAdxFormat.cs:59-62 never asks for more than 63 samples; the kernels see the
    // stream, i.e. the rows moved back by the padding and a length that counts it)
    const bool fast = p.frame_size == 18 && p.padding >= 0 && p.padding <= 64 && (pcm_pitch % 8) == 0 && ((uintptr_t)d_pcm % 16) == 0 &&
                      (out_pitch % 4) == 0 && ((uintptr_t)d_out % 4) == 0 && std::abs((int)p.coef0) <= 16384 &&
                      std::abs((int)p.coef1) <= 16384;
    note_adx_encode_path(fast ? 1 : 2);
    if (fast) {
        d_pcm -= p.padding;                            // from here on d_pcm / pcm_length are the STREAM's
        pcm_length += p.padding;
        const bool v4 = p.version == 4, ex = p.type == 4;
        // as many time segments as put ENCODE_WAVES_PER_SIMD waves on every SIMD, each an even number of frames and at
        // least ENCODE_MIN_PIECE_FRAMES long
        const int groups64 = (nch + 63) / 64;
        const int cus = device_cu_count();
        const int frames = (pcm_length + 31) / 32;
        const PiecePlan plan = plan_pieces(frames, cus * 4 * ENCODE_WAVES_PER_SIMD / groups64, ENCODE_MIN_PIECE_FRAMES, ENCODE_HOOK_FLOOR, PIECE_ALIGN_FRAMES);
        const int segments = plan.segments, seg_frames = plan.seg_frames;
        AsyncBuf scratch;                              // freed (stream-ordered) on every exit path
        int16_t *seg_state = nullptr;                  // [segments][nch][2] final histories, then [nch] first open seam
        int *first_open = nullptr, *seam_open = nullptr, *seam_end = nullptr, *queue = nullptr;
        uint2 *crumbs = nullptr;                       // [frames][nch]: 8 bytes per frame and channel (2.9 GB at configs[2])
        if (segments > 1) {
            const size_t state_bytes = round_up((size_t)segments * nch * 2 * sizeof(int16_t), 16);
            const size_t flag_bytes = (size_t)(segments - 1) * nch * sizeof(int);
            const size_t small_bytes = round_up(state_bytes + (size_t)nch * sizeof(int) + 2 * flag_bytes + 16, 16);   // (+ the fix-up's queue, the open seams' count)
            VGA_HIP_TRY(scratch.alloc(small_bytes + (size_t)frames * nch * sizeof(uint2), stream));
            seg_state = scratch.as<int16_t>();
            first_open = reinterpret_cast<int *>(scratch.as<unsigned char>() + state_bytes);
            seam_open = first_open + nch;
            seam_end = seam_open + (size_t)(segments - 1) * nch;
            queue = seam_end + (size_t)(segments - 1) * nch;
            crumbs = reinterpret_cast<uint2 *>(scratch.as<unsigned char>() + small_bytes);
            VGA_HIP_TRY(fill_no_open_seams(first_open, nch, stream));
            VGA_HIP_TRY(hipMemsetAsync(seam_open, 0, flag_bytes, stream));
            VGA_HIP_TRY(hipMemsetAsync(queue, 0, 2 * sizeof(int), stream));
        }
        int *open_seams = queue ? queue + 1 : nullptr; // seams still open at the end of their pieces
        // "many" as the decoders' threshold; test hook mode 3 = any
        const int many = force_open_seams() == 3 ? 1 : many_open_seams(nch, segments);
        // the fix-up's persistent waves: one per SIMD, fewer when there are not that many seams
        int fixup_waves = cus * 4 * ADX_FIXUP_WAVES_PER_SIMD;
#ifdef VGA_TUNING   // tools/build_variants.sh only
        if (const char *e = std::getenv("VGA_HIP_ADX_FIXUP_WAVES")) fixup_waves = std::max(1, std::atoi(e));
#endif
        fixup_waves = (int)std::min<int64_t>(fixup_waves, ((int64_t)nch * (segments - 1) + 63) / 64);
        if (fixup_waves < 1) fixup_waves = 1;
        const int rc = adx_with_version_and_type(v4, ex, [&](auto v, auto e) -> int {
            constexpr bool V = decltype(v)::value, E = decltype(e)::value;
            hipLaunchKernelGGL((adx_encode_fs18_direct_kernel<V, E>), dim3(groups64, segments), dim3(64), 0, stream, d_pcm, pcm_pitch, nch,
                               pcm_length, seg_frames, p, d_out, out_pitch, d_history_out, seg_state, crumbs, (const int *)nullptr,
                               (const int *)nullptr, 0);
            VGA_HIP_TRY(hipGetLastError());
            if (segments > 1) {
                hipLaunchKernelGGL((adx_encode_fs18_fixup_kernel<V, E>), dim3(fixup_waves), dim3(64), 0, stream, d_pcm, pcm_pitch, nch,
                                   pcm_length, seg_frames, segments, p, d_out, out_pitch, seg_state, crumbs, first_open, seam_open,
                                   seam_end, force_open_seams(), queue, d_own_frames, open_seams);
                VGA_HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL((adx_encode_fs18_tail_kernel<V, E>), dim3(groups64), dim3(64), 0, stream, d_pcm, pcm_pitch, nch,
                                   pcm_length, seg_frames, segments, p, d_out, out_pitch, seg_state, first_open, seam_open, seam_end,
                                   force_open_seams(), d_own_frames, open_seams, many);
                VGA_HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL((adx_encode_fs18_direct_kernel<V, E, true>), dim3(groups64, 1), dim3(64), 0, stream, d_pcm, pcm_pitch,
                                   nch, pcm_length, seg_frames, p, d_out, out_pitch, (int16_t *)nullptr, seg_state, (uint2 *)nullptr,
                                   (const int *)first_open, (const int *)open_seams, many);
            }
            return VGA_OK;
        });
        if (rc) return rc;
    } else {                                           // other frame sizes, padded (looping) streams, odd alignments
        hipLaunchKernelGGL(adx_encode_kernel, grid, block, 0, stream, d_pcm, pcm_pitch, nch, pcm_length, p, d_out, out_pitch,
                           d_history_out);
    }
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

int launch_decode(const uint8_t *d_adpcm, int64_t in_pitch, int nch, int sample_count, const AdxDeviceParams &p,
                  int16_t *d_pcm, int64_t pcm_pitch, int *d_status, hipStream_t stream, const int *d_own_samples)
{
    if (nch <= 0 || sample_count <= 0) return VGA_OK;
    // (padded streams: up to two frames of padding, equal-length batches, at least two frames of output)
    const bool fast = p.frame_size == 18 && (p.padding == 0 || (p.padding > 0 && p.padding <= 64 && !d_own_samples && sample_count >= 64)) &&
                      (pcm_pitch % 8) == 0 && ((uintptr_t)d_pcm % 16) == 0 && (in_pitch % 4) == 0 && ((uintptr_t)d_adpcm % 4) == 0;
    note_adx_decode_path(fast ? 1 : 2);
    if (fast) {
        if (p.padding > 0) {
            // The reference reads ceil(sampleCount / 32) frames from the frame the padding ends in and takes 32 - padding % 32
            // samples from the first of them (CriAdxCodec.cs:18-34): when that is not enough for sampleCount, the last samples
            // stay zero.  In stream positions: samples [padding, padding + decoded) are decoded, `pcm` moves back by the padding.
            const int out_count = sample_count;
            const int decoded = std::min(out_count, (out_count + 31) / 32 * 32 - p.padding % 32);
            if (decoded < out_count)
                VGA_HIP_TRY(hipMemset2DAsync(d_pcm + decoded, (size_t)pcm_pitch * sizeof(int16_t), 0,
                                             (size_t)(out_count - decoded) * sizeof(int16_t), (size_t)nch, stream));
            d_pcm -= p.padding;
            sample_count = decoded + p.padding;
        }
        // as many time pieces as put ONE wave on every SIMD (DECODE_WAVES_PER_SIMD; a wave = 64 channels of one piece), each at
        // least DECODE_MIN_PIECE_FRAMES (512) frames long and an even number of frames.  The kernel is bound by its stores, and what the memory system holds open is one
        // row position per (channel, piece): at configs[2] 8 / 16 / 32 / 64 pieces take 8.5 / 8.0 / 13.1 / 12.1 ms (and 12 or
        // 24, which leave some SIMDs with two waves and some with one, 11 ms)
        const int groups = (nch + 63) / 64;
        const int frames = (sample_count + 31) / 32;
        const PiecePlan plan = plan_pieces(frames, device_cu_count() * 4 * DECODE_WAVES_PER_SIMD / groups, DECODE_MIN_PIECE_FRAMES, DECODE_HOOK_FLOOR, PIECE_ALIGN_FRAMES);
        const int segments = plan.segments, seg_frames = plan.seg_frames;
        DecodeSeams ds;
        if (segments > 1)
            if (const int rc = ds.init(nch, segments, stream)) return rc;
        const int rc = adx_with_version(p.version == 4, [&](auto v) -> int {
            constexpr bool V = decltype(v)::value;
            hipLaunchKernelGGL((adx_decode_fs18_direct_kernel<V, false>), dim3(groups, segments), dim3(64), 0, stream, d_adpcm, in_pitch,
                               nch, sample_count, seg_frames, p, d_pcm, pcm_pitch, d_status, (const int *)nullptr, (const int *)nullptr);
            VGA_HIP_TRY(hipGetLastError());
            if (segments > 1) {
                hipLaunchKernelGGL(adx_decode_fs18_fixup_kernel<V>, dim3(groups, segments - 1), dim3(64), 0, stream, d_adpcm, in_pitch,
                                   nch, sample_count, seg_frames, p, d_pcm, pcm_pitch, ds.first_open, ds.seam_open, force_open_seams(),
                                   ds.slow_seams, d_own_samples);
                VGA_HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(adx_decode_fs18_tail_kernel<V>, dim3(groups), dim3(64), 0, stream, d_adpcm, in_pitch, nch,
                                   sample_count, seg_frames, segments, p, d_pcm, pcm_pitch, ds.first_open, ds.seam_open,
                                   force_open_seams(), ds.slow_seams, d_own_samples);
                VGA_HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL((adx_decode_fs18_direct_kernel<V, true>), dim3(groups, 1), dim3(64), 0, stream, d_adpcm, in_pitch, nch,
                                   sample_count, seg_frames, p, d_pcm, pcm_pitch, d_status, (const int *)ds.first_open,
                                   (const int *)ds.slow_seams);
            }
            return VGA_OK;
        });
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(adx_decode_kernel, dim3((nch + 63) / 64), dim3(64), 0, stream, d_adpcm, in_pitch, nch, sample_count, p,
                           d_pcm, pcm_pitch, d_status);
    }
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

}  // namespace adx
}  // namespace vga
