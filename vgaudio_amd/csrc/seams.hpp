// seams.hpp -- the time-piece seam protocol of the GC-ADPCM and ADX decoders: fix-up (seam_fixup), tail (seam_tail) and the
// REPAIR launch's wave minimum (wave_first_open).  The encoders share the first_open encoding, that minimum and the piece plan.
#pragma once
#include "common.hpp"

#include <algorithm>
#include <climits>

namespace vga {

// first_open[channel]: the first piece whose seam stayed open.  A 0x7f byte fill gives SEAM_NONE ("no open seam"), which
// is also what a channel that is done holds; an open piece's index lies in (0, SEAM_OPEN_LIMIT).
constexpr int SEAM_NONE = 0x7f7f7f7f;
constexpr int SEAM_OPEN_LIMIT = 0x7f000000;
__host__ __device__ inline bool is_open(int k) { return k > 0 && k < SEAM_OPEN_LIMIT; }

inline hipError_t fill_no_open_seams(int *first_open, int nch, hipStream_t stream)
{
    return hipMemsetAsync(first_open, 0x7f, (size_t)nch * sizeof(int), stream);
}

// The first piece any lane of the wave has left open (lanes that are not `live` contribute none)
__device__ __forceinline__ int wave_first_open(const int *first_open, bool live, int ch)
{
    int k = live ? first_open[ch] : SEAM_OPEN_LIMIT;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) k = min(k, __shfl_xor(k, o));
    return k;
}

// "many" open seams: one in 64, and at least 8 (the synthetic set's handful of slow channels stays with the tail kernel,
// whose runs meet again after a while; a batch of tones has every seam open)
inline int many_open_seams(int nch, int segments)
{
    return (int)std::min<int64_t>(INT_MAX, std::max<int64_t>(8, (int64_t)nch * (segments - 1) / 64));
}

// Time pieces of a stream of `frames` frames: `want` of them, each at least `min_frames` long, at most 64 (every piece
// boundary is a seam that may stay open to the end of its piece, and the tail kernel then walks the next piece again);
// the test hook's count (encoder_segments_override) wins, down to pieces of `hook_floor` frames.  seg_frames is a
// multiple of `align`.
struct PiecePlan {
    int segments, seg_frames;
};
inline PiecePlan plan_pieces(int frames, int want, int min_frames, int hook_floor, int align)
{
    int segments = want;
    if (segments > frames / min_frames) segments = frames / min_frames;
    if (segments < 1) segments = 1;
    if (segments > 64) segments = 64;
    if (encoder_segments_override() > 0) segments = std::min(std::max(frames / hook_floor, 1), encoder_segments_override());
    return {segments, ((frames + segments - 1) / segments + align - 1) / align * align};
}

// The decoders' stream-ordered scratch, freed with this object: first_open[nch] (SEAM_NONE), seam_open[(segments - 1) * nch]
// (seam k stayed open: [(k - 1) * nch + ch] != 0) and slow_seams = {seams that stayed open, how many make "many"}.
struct DecodeSeams {
    AsyncBuf scratch;
    int *first_open = nullptr, *seam_open = nullptr, *slow_seams = nullptr;
    int init(int nch, int segments, hipStream_t stream)
    {
        const size_t flag_bytes = (size_t)(segments - 1) * nch * sizeof(int);
        VGA_HIP_TRY(scratch.alloc((size_t)nch * sizeof(int) + flag_bytes + 16, stream));
        first_open = scratch.as<int>();
        seam_open = first_open + nch;
        slow_seams = seam_open + (size_t)(segments - 1) * nch;
        VGA_HIP_TRY(fill_no_open_seams(first_open, nch, stream));
        VGA_HIP_TRY(hipMemsetAsync(seam_open, 0, flag_bytes + 16, stream));
        // (a fill, not a copy from this stack frame: a pageable host-to-device copy makes the call wait for the stream)
        VGA_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(slow_seams + 1), many_open_seams(nch, segments), 1, stream));
        return VGA_OK;
    }
};

// The fix-up and tail bodies take the codec as a policy C (GcDecodeSeams, AdxDecodeSeams): FRAME_SAMPLES / _BYTES; SLOW_SEAM
// (frames after which an open seam counts as slow) and SLOW_POLL (how often a lane then reads the count); TAIL_BUDGET; HAS_OWN
// (own(): the channel is a shorter stream padded to the batch's length); channel(slot), length(ch, total); open(ch) sets
// src / dst and whatever decode(fr, valid, h1, h2, o) -- one frame from the history (h1, h2) into o[0 .. valid) -- needs.

// Closes the seams between time pieces: one lane per (channel, seam), all seams at once.  From the history the piece
// before ended on (its last two samples: final provided THAT piece's own seam closes) decode again frame by frame over the
// guessed run's samples until both histories coincide at a frame end -- from there on the guessed run decoded exactly what
// the serial decoder would have.  A seam that does not close inside its piece records its index in first_open[channel];
// seam_tail then decodes that channel from the next piece on.  Always exact.
template <class C>
__device__ __forceinline__ void seam_fixup(C c, int nch, int total_samples, int seg_frames, int *__restrict__ first_open,
                                           int *__restrict__ seam_open, int force_open, int *__restrict__ slow_seams)
{
    constexpr int SPF = C::FRAME_SAMPLES;
    const int slot = blockIdx.x * 64 + threadIdx.x;
    const int k = blockIdx.y + 1;
    const int64_t f0 = (int64_t)k * seg_frames;
    if (slot >= nch) return;
    const int ch = c.channel(slot);
    total_samples = c.length(ch, total_samples);
    if (f0 * SPF >= total_samples) return;
    // own (HAS_OWN): a seam in the channel's padding is nobody's output, and neither is what a run does once it has passed
    // the channel's own samples (two runs through zero frames need never meet: -1 is a fixed point of the predictor's floor)
    const int64_t own = C::HAS_OWN ? c.own(ch, total_samples) : 0;
    if (C::HAS_OWN && f0 * SPF >= own) return;
    c.open(ch);
    const int full_frames = total_samples / SPF;
    // Seed = the last two samples of piece k-1, read while seam k-1's lane (another thread, all seams run at once) may
    // still be rewriting that piece.  Invariant that makes this safe: if seam k-1 CLOSES, the samples it rewrites past
    // its closing frame are untouched and the ones before it get the values of the serial run -- the tail of piece
    // k-1, which is what is read here, is identical before and after (a closing seam never reaches the last frame
    // without having matched the guessed run there, i.e. it rewrites those two samples with the values they hold);
    // if seam k-1 stays OPEN, first_open[ch] <= k-1 and seam_tail decodes pieces k.. again from the final samples,
    // overwriting whatever this lane produced from a possibly stale seed.  Either way the output is exact.
    int h1 = c.dst[f0 * SPF - 1], h2 = c.dst[f0 * SPF - 2];
    // Round 5: a seam still open after SLOW_SEAM frames counts as slow (slow_seams[0]); once the batch holds slow_seams[1]
    // of them -- a batch of tones: their seams never close -- the lanes stop walking their pieces (12 800 frames each for
    // GC-ADPCM at configs[1]) and leave everything from their piece on to the REPAIR launch of the direct kernel, which
    // decodes the affected waves as one piece.  Below that count nothing changes: a seam runs to its piece's end and
    // seam_tail chains the few that stay open.  (A lane only gives up when the count has been reached, so "somebody gave
    // up" implies the REPAIR launch runs.)
    int walked = 0;
    bool counted = false, gave_up = false;
    // (seams the test hook holds open are not counted -- modes 1 and 2 exercise the tail kernel as before -- unless it asks for it: 3)
    const bool countable = !seam_forced_open(force_open, ch, k) || force_open == 3;
    for (int64_t f = f0; f < f0 + seg_frames && f * SPF < total_samples; f++) {
        const int valid = f < full_frames ? SPF : total_samples - (int)(f * SPF);
        int16_t *o = c.dst + f * SPF;
        int g1 = 0, g2 = 0;                            // the guessed run's history at this frame's end
        if (valid == SPF) { g1 = o[SPF - 1]; g2 = o[SPF - 2]; }
        c.decode(c.src + f * C::FRAME_BYTES, valid, h1, h2, o);
        if (valid == SPF && h1 == g1 && h2 == g2 && !seam_forced_open(force_open, ch, k)) return;
        if (valid < SPF) return;                       // the stream's last, partial frame: nothing follows
        if (C::HAS_OWN && (f + 1) * SPF >= own) return;   // the channel's own samples are all final
        if (++walked == C::SLOW_SEAM && countable) {
            atomicAdd(&slow_seams[0], 1);
            counted = true;
        }
        if (walked >= C::SLOW_SEAM && (walked & (C::SLOW_POLL - 1)) == 0 &&
            __hip_atomic_load(&slow_seams[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= slow_seams[1]) {
            gave_up = true;
            break;
        }
    }
    const bool piece_follows = (f0 + seg_frames) * SPF < total_samples;
    if (!counted && piece_follows && countable) atomicAdd(&slow_seams[0], 1);   // (a piece shorter than the limit that never closed)
    if (piece_follows || gave_up) {                    // open (and a piece follows), or this piece itself is left unfinished
        if (piece_follows) seam_open[(int64_t)(k - 1) * nch + ch] = 1;
        atomicMin(&first_open[ch], k);
    }
}

// The channels with an open seam, piece after piece (one lane per channel; lanes without one leave at once).  A seam
// that ran out of frames has made ITS piece final, but the piece after it was seeded from samples that have changed
// since: that piece is decoded again from the final samples -- next to what it holds, which is a run of the same
// recurrence from some other history -- until both agree at a frame end; from there on the stored samples are the
// serial decoder's.  (Round 1 decoded the whole rest of the channel again: 220 ms for a 60 s GC-ADPCM channel.)  A run
// that does not meet by the end of a piece carries on into the next one; a later open seam of the channel starts the same
// again.
template <class C>
__device__ __forceinline__ void seam_tail(C c, int nch, int total_samples, int seg_frames, int segments, int *__restrict__ first_open,
                                          const int *__restrict__ seam_open, int force_open, int *__restrict__ slow_seams)
{
    constexpr int SPF = C::FRAME_SAMPLES;
    const int slot = blockIdx.x * 64 + threadIdx.x;
    if (slot >= nch) return;
    // many seams that would not close -- or a lane of this launch has handed a channel over (below): the REPAIR launch of the
    // direct kernel runs, and it takes every channel whose first_open is still set, this one included
    if (__hip_atomic_load(&slow_seams[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= slow_seams[1]) return;
    const int ch = c.channel(slot);
    total_samples = c.length(ch, total_samples);
    const int k0 = first_open[ch];
    if (!is_open(k0)) return;
    const int64_t own = C::HAS_OWN ? c.own(ch, total_samples) : 0;   // (see seam_fixup)
    int walked_total = 0;                              // frames this lane has decoded again (see TAIL_BUDGET)
    c.open(ch);
    const int full_frames = total_samples / SPF;
    bool carry = false;                                // the piece before ended on samples other than the ones this piece was seeded from
    int h1 = 0, h2 = 0;
    for (int k = k0; k < segments; k++) {
        const int64_t f0 = (int64_t)k * seg_frames;
        if (f0 * SPF >= total_samples || (C::HAS_OWN && f0 * SPF >= own)) break;
        const bool flagged = seam_open[(int64_t)(k - 1) * nch + ch] != 0;
        bool apart = false;
        if (carry) {
            apart = true;
            for (int64_t f = f0; f < f0 + seg_frames && f * SPF < total_samples; f++) {
                const int valid = f < full_frames ? SPF : total_samples - (int)(f * SPF);
                int16_t *o = c.dst + f * SPF;
                int g1 = 0, g2 = 0;
                if (valid == SPF) { g1 = o[SPF - 1]; g2 = o[SPF - 2]; }
                c.decode(c.src + f * C::FRAME_BYTES, valid, h1, h2, o);
                walked_total++;
                if (valid == SPF && h1 == g1 && h2 == g2 && !seam_forced_open(force_open, ch, k)) { apart = false; break; }
                if (C::HAS_OWN && (f + 1) * SPF >= own) { apart = false; break; }   // past the channel's own samples: as good as met
            }
        }
        const int64_t f1 = f0 + seg_frames;            // the next piece's first frame
        if (apart) {
            carry = true;                              // (h1, h2): the true samples at the end of this piece
            // A run that has not met after TAIL_BUDGET frames (a tone, a clipped wave: it never will) is not walked to the
            // end of the stream by ONE lane: the pieces up to this one are final now, the REPAIR launch decodes the channel's
            // wave from the next piece on at the direct kernel's speed (bench.py signal_sensitivity: 43 such ADX channels in
            // 4096 cost the tail kernel 347 ms).  Seams the test hook holds open do not count.
            if (walked_total >= C::TAIL_BUDGET && f1 * SPF < total_samples && (force_open == 0 || force_open == 3)) {
                first_open[ch] = k + 1;
                atomicMax(&slow_seams[0], slow_seams[1]);
                return;
            }
        } else if (flagged && f1 * SPF < total_samples) {
            carry = true;                              // this piece's own seam ran out of frames: the piece is final, its end the truth
            h1 = c.dst[f1 * SPF - 1];
            h2 = c.dst[f1 * SPF - 2];
        } else
            carry = false;
    }
    first_open[ch] = SEAM_NONE;                        // done: nothing of this channel is left for the REPAIR launch
}

}  // namespace vga
