// gc_decode_kernel.hip -- GC-ADPCM decoder for gfx950.
//
// Replaces VGAudio/Codecs/GcAdpcm/GcAdpcmDecoder.cs:10-54, bit-exact.
//
// The decoder is a second-order IIR with saturation and a truncating shift per sample (:38-45): serial inside a
// channel.  Lane = channel; a channel's stream is cut into time pieces decoded side by side (every piece but the first
// from a guessed history), gc_decode_fixup_kernel closes the seams, gc_decode_tail_kernel chains the ones that stay
// open.  Rounds 1-2 split the work between a serial wave and three helper waves through LDS tiles (the helpers unpacked
// scale * nibble + 1024 and wrote the samples out); the tiles' 108 KB per 128 channels limited a CU to one workgroup and
// 4096 channels to eight pieces.  The kernel below needs no helpers: 9.9 -> 8.1 ms at configs[1] -- bound by its stores,
// 3 TB/s (LABNOTES.md 4.3) -- and 4.4 -> 1.2 ms for 256 channels.
#include "common.hpp"

#include <algorithm>
#include "gcadpcm_kernels.hpp"
#include "seams.hpp"

#include <cstdlib>

namespace vga {
namespace gc {

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// ---------------------------------------------------------------------------------------------------------------
// Lane = channel, one wave per 64 channels and time piece, as many pieces as put one wave on every SIMD (the ADX decoder
// in adx_kernels.hip has the measurements behind this shape).  A lane reads its own
// frames eight at a time (64 contiguous bytes, the next block in flight during this one), takes the nibbles out of the
// loaded dwords with one v_bfe_i32 each, looks its coefficient pair up in the wave's LDS table and runs the recurrence
// (:38-45).  The 8 x 28 bytes of samples a lane produces per block are contiguous in its row; they leave through the
// wave's LDS block turned, fourteen lanes per row, as 16-byte stores of whole 224-byte runs (TURNED; rows that are not
// 16-byte aligned are stored by their own lane, a dword at a time).  Later pieces start from the guess (0, 0) GC_DECODE_WARM
// frames early without storing, so that they have, as a rule, fallen into step with the true run where they begin and
// their seam closes on the first frame gc_decode_fixup_kernel checks.
constexpr int GC_DECODE_WARM = 512;                  // frames; a multiple of 8
constexpr int GC_DECODE_SLOW_SEAM = 2048;            // frames a seam may stay open before it counts as slow (a multiple of 256)
constexpr int GC_DECODE_TAIL_BUDGET = 4096;          // frames one lane of the tail kernel decodes again before it hands over
// RAGGED (the `*_v` entry points): lane i of workgroup x decodes channel order[64 x + i] (longest first), with its own
// length and offsets; a piece exists for a lane only as far as its channel reaches, the wave runs as many blocks as its
// longest lane has (lane 0) and every row of the turned store is guarded by its own block count.
// (REPAIR is a template parameter so that the launch carries a name of its own in profiles: it returns at once as a rule and
// would halve the kernel's average duration)
template <bool TURNED, bool RAGGED, bool REPAIR>
__global__ __launch_bounds__(64) void gc_decode_direct_kernel(
    const uint8_t *__restrict__ adpcm, int64_t adpcm_pitch, const int16_t *__restrict__ coefs, int nch,
    int total_samples, int seg_frames, const int16_t *__restrict__ hist1, const int16_t *__restrict__ hist2,
    int16_t *__restrict__ pcm, int64_t pcm_pitch, int *__restrict__ status, const Ragged rg,
    const int *__restrict__ first_open, const int *__restrict__ slow_seams)
{
    const int lane = threadIdx.x;
    const int slot_raw = blockIdx.x * 64 + lane;
    const bool live = slot_raw < nch;
    const int slot = live ? slot_raw : nch - 1;
    const int ch = RAGGED ? rg.order[slot] : slot;
    // REPAIR launch (round 5): the batch holds many seams that would not close -- pure tones, clipped
    // waves: a decoder run from a wrong history never falls into step when the predictor's poles sit on the unit circle.  The
    // wave decodes its 64 channels again as ONE piece, from the first piece any of them left open to the end of the stream,
    // from the samples before it (final: every earlier seam of every lane closed).  This is the serial floor -- a lone wave
    // needs ~57 ms for 60 s -- against 1.36 s for the chained tail kernel on a batch of 440 Hz sines (bench.py signal_sensitivity).
    constexpr bool repair = REPAIR;
    int repair_piece = 0;
    if (repair) {
        if (slow_seams[0] < slow_seams[1]) return;                        // few open seams: gc_decode_tail_kernel has them
        const int k = wave_first_open(first_open, live, ch);
        if (!is_open(k)) return;                                           // none of these channels has an open seam
        repair_piece = k;
    }
    const int64_t first_frame = (int64_t)(repair ? repair_piece : (int)blockIdx.y) * seg_frames;   // a multiple of 8 (seg_frames is)
    if (repair) seg_frames = 0x7fffff00 / 14;                              // ... to the end of the stream
    const int64_t first_sample = first_frame * 14;
    if (RAGGED) {
        if (first_sample >= rg.length[rg.order[blockIdx.x * 64]]) return;  // the wave's longest channel ends before this piece
        total_samples = rg.length[ch];
    } else if (first_sample >= total_samples)
        return;
    const bool exists = !RAGGED || first_sample < total_samples;           // this lane's channel reaches the piece
    const int sample_count = !exists ? 0 : (int)((int64_t)total_samples - first_sample < (int64_t)seg_frames * 14
                                                     ? (int64_t)total_samples - first_sample : (int64_t)seg_frames * 14);
    const int full_frames = sample_count / 14;
    const int tail = sample_count - full_frames * 14;
    // a lane without the piece points at its channel's first bytes (valid memory for its clamped loads) and stores nothing
    const uint8_t *src = adpcm + (RAGGED ? rg.adpcm_off[ch] : (int64_t)ch * adpcm_pitch) + (exists ? first_frame * 8 : 0);
    int16_t *dst = pcm + (RAGGED ? rg.pcm_off[ch] : (int64_t)ch * pcm_pitch) + (exists ? first_sample : 0);
    __shared__ uint32_t s_cf[8 * 64];                                      // [predictor][lane]: (coef1 & 0xFFFF) | coef2 << 16
    __shared__ int4 s_turn[64 * 15];                                       // 64 rows of 14 int4 (8 frames), one int4 apart from a multiple of 8
    __shared__ int64_t s_row[RAGGED ? 64 : 1];                             // RAGGED: a row's first sample of the piece, counted from pcm
    __shared__ int s_rowblocks[RAGGED ? 64 : 1];                           // ... and its whole blocks of eight frames
    if (RAGGED) {
        s_row[lane] = (int64_t)(dst - pcm);
        s_rowblocks[lane] = live ? full_frames / 8 : 0;
    }
#pragma unroll
    for (int q = 0; q < 8; q++)
        s_cf[q * 64 + lane] = (uint32_t)(uint16_t)coefs[ch * 16 + 2 * q] | ((uint32_t)(uint16_t)coefs[ch * 16 + 2 * q + 1] << 16);
    int h1 = 0, h2 = 0;
    if (repair) {
        if (exists) { h1 = dst[-1]; h2 = dst[-2]; }
    } else if (blockIdx.y == 0) {
        h1 = hist1 ? hist1[ch] : 0;
        h2 = hist2 ? hist2[ch] : 0;
    }
    bool bad_seen = false;
    bool bad = false;
    // one frame (bits = its 8 bytes, little-endian) -> 14 samples as 7 packed pairs
    auto decode_frame = [&](uint32_t lo, uint32_t hi, uint32_t (&o7)[7]) {
        const int ps = (int)(lo & 0xFF);
        const int sh = (ps & 0xF) + 11;                                    // scale = (1 << (ps & 0xF)) * 2048 (:26)
        int predictor = (ps >> 4) & 0xF;                                   // :27
        if (predictor > 7) { bad = true; predictor &= 7; }
        const uint32_t cf = s_cf[predictor * 64 + lane];
        const int c1 = (int)(int16_t)(cf & 0xFFFF), c2 = (int)cf >> 16;
        int o[14];
#pragma unroll
        for (int s = 0; s < 14; s++) {
            const int b = 1 + (s >> 1);                                    // the byte that holds sample s: high nibble first
            const uint32_t w = b < 4 ? lo : hi;
            const int nib = __builtin_amdgcn_sbfe((int)w, 8 * (b & 3) + ((s & 1) ? 0 : 4), 4);   // SignedNibbles (Helpers.cs:50)
            // :38-45: (coef1*hist1 + coef2*hist2 + scale*nibble + 1024) >> 11, clamped; int32 wrap like the reference
            int rest = __mul24(c2, h2) + (int)(((uint32_t)nib << sh) + 1024u);
            asm("" : "+v"(rest));
            const int t = __mul24(c1, h1) + rest;
            const int v = imin(imax(t >> 11, -32768), 32767);
            h2 = h1;
            h1 = v;
            o[s] = v;
        }
#pragma unroll
        for (int q = 0; q < 7; q++) o7[q] = (uint32_t)(o[2 * q] & 0xFFFF) | ((uint32_t)o[2 * q + 1] << 16);
    };
    auto turned_row = [&](int i, int l) {                                  // rows past the last channel: channel nch - 1 again,
        const int c = blockIdx.x * 64 + l / 14 + 4 * i;                    // whose samples those lanes hold -- unconditional stores
        return pcm + (int64_t)(c < nch ? c : nch - 1) * pcm_pitch + first_sample + (l % 14) * 8;
    };
    // ---- warm-up of a later piece (not stored)
    if (!repair && blockIdx.y > 0 && exists) {
        const int warm = (int)(first_frame < GC_DECODE_WARM ? first_frame : GC_DECODE_WARM);
        const uint2 *wsrc = reinterpret_cast<const uint2 *>(src) - warm;
#pragma unroll 1
        for (int k = 0; k < warm; k += 4) {                                // warm is a multiple of 8
            uint2 f[4];
#pragma unroll
            for (int j = 0; j < 4; j++) f[j] = wsrc[k + j];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t o7[7];
                decode_frame(f[j].x, f[j].y, o7);
            }
        }
    }
    bad_seen = bad;                                                        // (the warm-up reads real frames: a bad header there is a bad header)
    // ---- whole blocks of eight full frames
    const int my_blocks = full_frames / 8;
    const int blocks = RAGGED ? __shfl(my_blocks, 0) : my_blocks;          // lane 0 holds the wave's longest channel
    const uint4 *bsrc = reinterpret_cast<const uint4 *>(src);
    uint4 cur[4], nxt[4];
#pragma unroll
    for (int q = 0; q < 4; q++) cur[q] = blocks > 0 ? bsrc[q] : make_uint4(0, 0, 0, 0);
    // the first block is waited for HERE, not at the loop header (where the wait would also mean "every store of the
    // block before has completed")
#pragma unroll
    for (int q = 0; q < 4; q++) asm volatile("" : "+v"(cur[q].x), "+v"(cur[q].y), "+v"(cur[q].z), "+v"(cur[q].w));
#pragma unroll 1
    for (int k = 0; k < blocks; k++) {
        const uint4 *f = bsrc + (int64_t)(RAGGED ? imax(imin(k + 1, my_blocks - 1), 0) : imin(k + 1, blocks - 1)) * 4;
        const int keep1 = h1, keep2 = h2;                                  // RAGGED: a lane past its last block keeps its history
#pragma unroll
        for (int q = 0; q < 4; q++) nxt[q] = f[q];
#pragma unroll
        for (int half = 0; half < 2; half++) {
            uint32_t d28[28];                                              // four frames = 112 bytes = seven int4
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint4 v = cur[2 * half + (j >> 1)];
                uint32_t o7[7];
                decode_frame((j & 1) ? v.z : v.x, (j & 1) ? v.w : v.y, o7);
#pragma unroll
                for (int q = 0; q < 7; q++) d28[7 * j + q] = o7[q];
            }
            if (TURNED) {
#pragma unroll
                for (int q = 0; q < 7; q++)
                    s_turn[lane * 15 + half * 7 + q] = make_int4((int)d28[4 * q], (int)d28[4 * q + 1], (int)d28[4 * q + 2], (int)d28[4 * q + 3]);
            } else if (live && (!RAGGED || k < my_blocks)) {
                uint32_t *d32 = reinterpret_cast<uint32_t *>(dst + ((int64_t)k * 8 + half * 4) * 14);
#pragma unroll
                for (int q = 0; q < 28; q++) d32[q] = d28[q];
            }
        }
        if (TURNED) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const int l = imin(lane, 55);                                  // 4 rows x 14 lanes per store; the last eight lanes repeat lane 55's
#pragma unroll
            for (int i = 0; i < 16; i++) {                                 // read, store -- one at a time (see adx_kernels.hip)
                const int row = l / 14 + 4 * i;
                if (RAGGED) {
                    if (k < s_rowblocks[row])
                        *reinterpret_cast<int4 *>(pcm + s_row[row] + (l % 14) * 8 + (int64_t)k * 8 * 14) = s_turn[row * 15 + l % 14];
                } else
                    *reinterpret_cast<int4 *>(turned_row(i, l) + (int64_t)k * 8 * 14) = s_turn[row * 15 + l % 14];
            }
            asm volatile("" ::: "memory");
        }
        if (RAGGED && k >= my_blocks) {                                    // blocks past this lane's end decoded whatever was there
            bad = bad_seen;
            h1 = keep1;
            h2 = keep2;
        }
        bad_seen = bad;
#pragma unroll
        for (int q = 0; q < 4; q++) cur[q] = nxt[q];
    }
    // ---- what is left of the piece: fewer than eight full frames and a partial one
#pragma unroll 1
    for (int fr = my_blocks * 8; fr < full_frames + (tail ? 1 : 0); fr++) {
        uint32_t lo = 0, hi = 0;
        if (fr < full_frames) {
            const uint2 v = reinterpret_cast<const uint2 *>(src)[fr];
            lo = v.x;
            hi = v.y;
        } else {                                                           // partial last frame: only its bytes exist
            const int nbytes = (tail + 2 + 1) / 2;
            uint64_t bits = 0;
            for (int b = 0; b < nbytes; b++) bits |= (uint64_t)src[(int64_t)fr * 8 + b] << (8 * b);
            lo = (uint32_t)bits;
            hi = (uint32_t)(bits >> 32);
        }
        uint32_t o7[7];
        decode_frame(lo, hi, o7);
        if (!live) continue;
        int16_t *d = dst + (int64_t)fr * 14;
        if (fr < full_frames) {
#pragma unroll
            for (int q = 0; q < 7; q++) reinterpret_cast<uint32_t *>(d)[q] = o7[q];
        } else {
            for (int s2 = 0; s2 < tail; s2++) d[s2] = (int16_t)(o7[s2 >> 1] >> (16 * (s2 & 1)));
        }
    }
    if (bad && live && status) atomicOr(status, 1);
}

// One frame of GcAdpcmDecoder.Decode (:25-45) from the history (h1, h2) into o[0 .. valid).  A full frame is one 8-byte load
// (round 5: a byte at a time until then -- nine dependent loads a frame on a path that can walk a whole channel).
__device__ __forceinline__ void gc_decode_frame_serial(const uint8_t *fr, const int (&cf)[16], int valid, int &h1, int &h2,
                                                       int16_t *o)
{
    uint64_t bits = 0;
    if (valid == 14) {
        const uint2 v = *reinterpret_cast<const uint2 *>(fr);
        bits = ((uint64_t)v.y << 32) | v.x;
    } else {
        const int nbytes = (valid + 2 + 1) / 2;                             // the stream's last, partial frame: only its bytes exist
        for (int b = 0; b < nbytes; b++) bits |= (uint64_t)fr[b] << (8 * b);
    }
    const int ps = (int)(bits & 0xFF);
    const int scale = (1 << (ps & 0xF)) * 2048;
    const int predictor = (ps >> 4) & 7;
    int c1 = 0, c2 = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (predictor == i) { c1 = cf[2 * i]; c2 = cf[2 * i + 1]; }
    int16_t out14[14];
#pragma unroll
    for (int s = 0; s < 14; s++) {
        const int byte = (int)((bits >> (8 * (1 + (s >> 1)))) & 0xFF);
        const int nib = (s & 1) ? (byte & 0xF) : (byte >> 4);
        const int v = imin(imax((c1 * h1 + c2 * h2 + scale * ((nib ^ 8) - 8) + 1024) >> 11, -32768), 32767);
        if (s < valid) {
            h2 = h1;
            h1 = v;
        }
        out14[s] = (int16_t)v;
    }
    if (valid == 14) {
        uint32_t *o32 = reinterpret_cast<uint32_t *>(o);                    // rows and frames are 4-byte aligned (28-byte frames)
#pragma unroll
        for (int q = 0; q < 7; q++) o32[q] = (uint32_t)(uint16_t)out14[2 * q] | ((uint32_t)(uint16_t)out14[2 * q + 1] << 16);
    } else {
        for (int s = 0; s < valid; s++) o[s] = out14[s];
    }
}

// The GC-ADPCM side of the seam protocol (seams.hpp): a lane's channel is rg.order[slot] with its own length and offsets
// when the batch is ragged, the slot at the dense pitch otherwise.
struct GcDecodeSeams {
    static constexpr int FRAME_SAMPLES = 14, FRAME_BYTES = 8;
    static constexpr int SLOW_SEAM = GC_DECODE_SLOW_SEAM, SLOW_POLL = 256, TAIL_BUDGET = GC_DECODE_TAIL_BUDGET;
    static constexpr bool HAS_OWN = false;
    const uint8_t *adpcm; int64_t adpcm_pitch; const int16_t *coefs; int16_t *pcm; int64_t pcm_pitch; Ragged rg;
    const uint8_t *src; int16_t *dst; int cf[16];                        // (open)
    __device__ int channel(int slot) const { return rg.order ? rg.order[slot] : slot; }
    __device__ int length(int ch, int total) const { return rg.order ? rg.length[ch] : total; }
    __device__ int64_t own(int, int total) const { return total; }
    __device__ void open(int ch)
    {
        src = adpcm + (rg.order ? rg.adpcm_off[ch] : (int64_t)ch * adpcm_pitch);
        dst = pcm + (rg.order ? rg.pcm_off[ch] : (int64_t)ch * pcm_pitch);
#pragma unroll
        for (int i = 0; i < 16; i++) cf[i] = coefs[ch * 16 + i];
    }
    __device__ void decode(const uint8_t *fr, int valid, int &h1, int &h2, int16_t *o) const { gc_decode_frame_serial(fr, cf, valid, h1, h2, o); }
};

__global__ __launch_bounds__(64) void gc_decode_fixup_kernel(
    const uint8_t *__restrict__ adpcm, int64_t adpcm_pitch, const int16_t *__restrict__ coefs, int nch,
    int total_samples, int seg_frames, int16_t *__restrict__ pcm, int64_t pcm_pitch, int *__restrict__ first_open,
    int *__restrict__ seam_open, int force_open, const Ragged rg, int *__restrict__ slow_seams)
{
    seam_fixup(GcDecodeSeams{adpcm, adpcm_pitch, coefs, pcm, pcm_pitch, rg}, nch, total_samples, seg_frames, first_open, seam_open,
               force_open, slow_seams);
}

__global__ __launch_bounds__(64) void gc_decode_tail_kernel(
    const uint8_t *__restrict__ adpcm, int64_t adpcm_pitch, const int16_t *__restrict__ coefs, int nch,
    int total_samples, int seg_frames, int segments, int16_t *__restrict__ pcm, int64_t pcm_pitch,
    int *__restrict__ first_open, const int *__restrict__ seam_open, int force_open, const Ragged rg,
    int *__restrict__ slow_seams)
{
    seam_tail(GcDecodeSeams{adpcm, adpcm_pitch, coefs, pcm, pcm_pitch, rg}, nch, total_samples, seg_frames, segments, first_open,
              seam_open, force_open, slow_seams);
}

int launch_decode(const uint8_t *d_adpcm, int64_t adpcm_pitch, const int16_t *d_coefs, int nch, int sample_count,
                  const int16_t *d_hist1, const int16_t *d_hist2, int16_t *d_pcm, int64_t pcm_pitch, int *d_status,
                  hipStream_t stream, const Ragged *rgp)
{
    const Ragged rg = rgp ? *rgp : Ragged{};
    if (rgp) sample_count = rg.max_length;
    if (nch <= 0 || sample_count <= 0) return VGA_OK;
    // as many time pieces as put one wave on every SIMD (a wave = 64 channels of one piece), each at least 1024 frames long
    // and a multiple of eight frames
    const int frames = (sample_count + 13) / 14;
    const int groups = (nch + 63) / 64;
    const int cus = device_cu_count();
    int want = cus * 4 / groups;
    if (rgp) {
        // ragged: pieces of one length for every channel, twice as many waves as the chip holds at once (the short ones
        // make room), `want` = what the longest channel needs
        const int64_t waves = (int64_t)cus * 4 * 2;
        const int64_t piece = std::max<int64_t>((rg.total_frames + 64 * waves - 1) / (64 * waves), 1024);
        want = (int)((frames + piece - 1) / piece);
    }
    const PiecePlan plan = plan_pieces(frames, want, 1024, 8, 8);
    const int segments = plan.segments, seg_frames = plan.seg_frames;
    // rows of samples on 16-byte boundaries: whole 224-byte runs leave as 16-byte stores
    const bool turned = (pcm_pitch % 8) == 0 && ((uintptr_t)d_pcm % 16) == 0;
#define VGA_GC_DIRECT(TURNED_, RAGGED_, REPAIR_, PIECES_, OPEN_, SLOW_)                                                          \
    hipLaunchKernelGGL((gc_decode_direct_kernel<TURNED_, RAGGED_, REPAIR_>), dim3(groups, PIECES_), dim3(64), 0, stream, d_adpcm, \
                       adpcm_pitch, d_coefs, nch, sample_count, seg_frames, d_hist1, d_hist2, d_pcm, pcm_pitch, d_status, rg,     \
                       (const int *)(OPEN_), (const int *)(SLOW_))
    auto direct = [&](int pieces, const int *first_open, const int *slow_seams) {
        const bool repair = first_open != nullptr;
        if (rgp) {                                     // (the ragged layout keeps every row on a 16-byte boundary)
            if (repair) VGA_GC_DIRECT(true, true, true, pieces, first_open, slow_seams);
            else VGA_GC_DIRECT(true, true, false, pieces, nullptr, nullptr);
        } else if (turned) {
            if (repair) VGA_GC_DIRECT(true, false, true, pieces, first_open, slow_seams);
            else VGA_GC_DIRECT(true, false, false, pieces, nullptr, nullptr);
        } else {
            if (repair) VGA_GC_DIRECT(false, false, true, pieces, first_open, slow_seams);
            else VGA_GC_DIRECT(false, false, false, pieces, nullptr, nullptr);
        }
        return hipGetLastError();
    };
#undef VGA_GC_DIRECT
    VGA_HIP_TRY(direct(segments, nullptr, nullptr));
    if (segments > 1) {
        DecodeSeams ds;
        if (const int rc = ds.init(nch, segments, stream)) return rc;
        hipLaunchKernelGGL(gc_decode_fixup_kernel, dim3((nch + 63) / 64, segments - 1), dim3(64), 0, stream, d_adpcm, adpcm_pitch,
                           d_coefs, nch, sample_count, seg_frames, d_pcm, pcm_pitch, ds.first_open, ds.seam_open, force_open_seams(), rg,
                           ds.slow_seams);
        VGA_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(gc_decode_tail_kernel, dim3((nch + 63) / 64), dim3(64), 0, stream, d_adpcm, adpcm_pitch, d_coefs, nch,
                           sample_count, seg_frames, segments, d_pcm, pcm_pitch, ds.first_open, ds.seam_open, force_open_seams(), rg,
                           ds.slow_seams);
        VGA_HIP_TRY(hipGetLastError());
        VGA_HIP_TRY(direct(1, ds.first_open, ds.slow_seams));
    }
    return VGA_OK;
}

}  // namespace gc
}  // namespace vga
