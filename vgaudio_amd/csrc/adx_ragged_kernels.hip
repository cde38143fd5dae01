// adx_ragged_kernels.hip -- CRI ADX encode / decode of a PACKED batch of channels of different lengths for gfx950
// (include/vgaudio_hip/adx_ragged.h): the kernels of adx_kernels.hip with their rows, lengths and work items read from the
// object's tables instead of a pitch and one length.
//
// The plan (adx_host.hpp) is the GC-ADPCM ragged call's: work slot -> channel longest first, 64 slots = one group = the lanes
// of a wave, the longest channel cut into time pieces, and one wave per (group, piece) ITEM whose first frame lies inside the
// group's longest channel.  What is uniform over a wave in adx_kernels.hip and is per LANE here: the row pointers, the
// length and everything derived from it (frames, the last full frame, the end of the piece), the clamps of the prefetches
// -- which stay inside the lane's own row -- and where the row's stores end.  A lane whose channel has ended waits for the
// longest of its group; the slots are sorted, so the lanes of a group are of similar length.
// Shared with adx_kernels.hip, written once in adx_device.hpp: the encoder's piece, fix-up queue and tail lane -- the kernels
// here are their shells over AdxPackedRows -- and the decoder's frame arithmetic, pack, frame load, pair split and warm-up;
// the decoder's fix-up and tail are seams.hpp's.  Per file: the kernels' names and argument lists, how a wave finds its
// (group, piece), the start history, the general lane-per-channel kernels' row lookup, the launchers, and the decoder's
// outer pair loop, which here walks the wave's longest lane with the others frozen and stores through per-lane row tables.
#include "common.hpp"
#include "adx_kernels.hpp"
#include "adx_device.hpp"
#include "adx_host.hpp"
#include "seams.hpp"

#include <type_traits>

namespace vga {
namespace adx {

// ---------------------------------------------------------------- any frame size, padded streams: lane = slot
__global__ __launch_bounds__(64) void adx_encode_ragged_kernel(const int16_t *__restrict__ pcm, AdxRaggedTables t, AdxDeviceParams p,
                                                               uint8_t *__restrict__ out, int16_t *__restrict__ history_out)
{
    const int slot = blockIdx.x * 64 + threadIdx.x;
    const int ch = t.channel[slot];
    if (ch < 0) return;
    adx_encode_channel(pcm + t.pcm_off[slot], t.length[slot], p, reinterpret_cast<uint16_t *>(out + t.adx_off[slot]),
                       history_out ? history_out + ch : nullptr);
}

__global__ __launch_bounds__(64) void adx_decode_ragged_kernel(const uint8_t *__restrict__ adpcm, AdxRaggedTables t, AdxDeviceParams p,
                                                               int16_t *__restrict__ pcm, int *__restrict__ status)
{
    const int slot = blockIdx.x * 64 + threadIdx.x;
    const int ch = t.channel[slot];
    if (ch < 0 || t.length[slot] <= 0) return;
    adx_decode_channel(adpcm + t.adx_off[slot], t.length[slot], p, pcm + t.pcm_off[slot], status + ch);
}

// ---------------------------------------------------------------- 18-byte frames, no padding: the encoder's time pieces
// adx_encode_fs18_direct_kernel over the items.  seg_state is [piece][slot], the crumbs of group g are the block
// [group_frames[g]][64] at t.crumb_base[g]: 8 bytes per frame and lane of the group's longest channel, not of the batch's.
// History (:69-74): the object holds no channel of 0 samples when V4 (vga_adx_encode_device_v refuses it), and without V4
// every channel's is p.history, which the launcher fills in.
template <bool V4, bool EXPONENTIAL, bool REPAIR = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void adx_encode_fs18_direct_ragged_kernel(
    const int16_t *__restrict__ pcm, AdxRaggedTables t, const int2 *__restrict__ items, int seg_frames, AdxDeviceParams p,
    uint8_t *__restrict__ out, int16_t *__restrict__ history_out, int16_t *__restrict__ seg_state, uint2 *__restrict__ crumbs,
    const int *__restrict__ first_open, const int *__restrict__ open_seams, int many)
{
    int g = blockIdx.x, k = 0;
    if (!REPAIR) {
        const int2 it = items[blockIdx.x];
        g = it.x;
        k = it.y;
    }
    const int slot = g * 64 + threadIdx.x;
    if (REPAIR) {
        if (open_seams[0] < many) return;              // few: adx_encode_fs18_tail_ragged_kernel has chained them
        const int ko = wave_first_open(first_open, true, slot);
        if (!is_open(ko)) return;                      // no open seam among this wave's channels
        k = ko;
    }
    const int64_t f0 = (int64_t)k * seg_frames;
    if (f0 * 32 >= t.length[slot]) return;             // the channel ended before this piece (or holds nothing at all)
    AdxPackedRows r{pcm, t, out, crumbs};
    r.open(slot);
    int a = 0, b = 0;
    if (REPAIR) {                                      // the true history at the start of piece k
        const int16_t *st = seg_state + r.state(k - 1) * 2;
        a = st[0];
        b = st[1];
    } else if (k > 0) {                                // the guess: the input just before this piece
        a = r.src[f0 * 32 - 2];
        b = r.src[f0 * 32 - 1];
    } else if (V4) {
        a = b = r.src[0];                              // :69-74
        if (history_out) history_out[t.channel[slot]] = (int16_t)a;
    }
    adx_encode_piece<V4, EXPONENTIAL, REPAIR>(r, k, seg_frames, p, a, b, seg_state);
}

// adx_encode_fs18_fixup_kernel over (slot, seam) pairs: a seam exists where the LANE's own stream reaches piece k; its run
// ends with the lane's own frames.  (The queue also hands out the pairs of channels that ended earlier: a pop each.)
template <bool V4, bool EXPONENTIAL>
__global__ __launch_bounds__(64) void adx_encode_fs18_fixup_ragged_kernel(
    const int16_t *__restrict__ pcm, AdxRaggedTables t, int seg_frames, int segments, AdxDeviceParams p, uint8_t *__restrict__ out,
    const int16_t *__restrict__ seg_state, const uint2 *__restrict__ crumbs, int *__restrict__ first_open, int *__restrict__ seam_open,
    int *__restrict__ seam_end, int force_open, int *__restrict__ queue, int *__restrict__ open_seams)
{
    __builtin_assume(crumbs != nullptr);               // (launched where there are seams: the pieces have left crumbs)
    adx_encode_fixup<V4, EXPONENTIAL>(AdxPackedRows{pcm, t, out, const_cast<uint2 *>(crumbs), pcm, out, const_cast<uint2 *>(crumbs)}, seg_frames,
                                      segments, p, seg_state, first_open, seam_open, seam_end, force_open, queue, open_seams);
}

// adx_encode_fs18_tail_kernel: one lane per slot, on the lane's own row and length
template <bool V4, bool EXPONENTIAL>
__global__ __launch_bounds__(64) void adx_encode_fs18_tail_ragged_kernel(
    const int16_t *__restrict__ pcm, AdxRaggedTables t, int seg_frames, int segments, AdxDeviceParams p, uint8_t *__restrict__ out,
    const int16_t *__restrict__ seg_state, const int *__restrict__ first_open, const int *__restrict__ seam_open,
    const int *__restrict__ seam_end, int force_open, const int *__restrict__ open_seams, int many)
{
    adx_encode_tail<V4, EXPONENTIAL>(AdxPackedRows{pcm, t, out, nullptr}, blockIdx.x * 64 + threadIdx.x, seg_frames, segments, p, seg_state,
                                     first_open, seam_open, seam_end, force_open, open_seams, many);
}

// ---------------------------------------------------------------- 18-byte frames, no padding: the decoder's time pieces
// adx_decode_fs18_direct_kernel over the items.  The turned stores (LPR lanes write 64 x TURN bytes of ONE row together)
// are what ragged rows change: the lane that stores part of row r needs r's pointer and r's own end, so every lane keeps
// both for the LPR rows it stores to.  The wave walks the pairs of its longest lane; a lane whose row has ended keeps
// decoding its last pair (loads clamped to its own row, history and status frozen), and the store of a block that lies past
// its row's end goes to `sink`, a line of the workspace nobody reads -- the stores stay unconditional, so hipcc can still
// count them (see adx_decode_fs18_direct_kernel's turned_row), and a row that has ended is not written.
// The warm-up starts at most ADX_DECODE_WARM_FRAMES before the piece and never in front of the row (first_frame frames lie
// before it); lanes without frames in the piece skip it.
template <bool V4, bool REPAIR>
__global__ __launch_bounds__(64) void adx_decode_fs18_direct_ragged_kernel(
    const uint8_t *__restrict__ adpcm, AdxRaggedTables t, const int2 *__restrict__ items, int seg_frames, AdxDeviceParams p,
    int16_t *__restrict__ pcm, int *__restrict__ status, const int *__restrict__ first_open, const int *__restrict__ slow_seams,
    int4 *__restrict__ sink)
{
    const int lane = threadIdx.x;
    int g = blockIdx.x, k = 0;
    if (!REPAIR) {
        const int2 it = items[blockIdx.x];
        g = it.x;
        k = it.y;
    }
    const int slot = g * 64 + lane;
    if (REPAIR) {
        if (slow_seams[0] < slow_seams[1]) return;                        // few: adx_decode_fs18_tail_ragged_kernel has them
        k = wave_first_open(first_open, true, slot);
        if (!is_open(k)) return;
    }
    const int64_t first_frame = (int64_t)k * seg_frames;                   // even (seg_frames is)
    const int64_t piece_samples = REPAIR ? (int64_t)0x7fffff00 : (int64_t)seg_frames * 32;
    // what a row of `length` samples holds of this piece
    auto in_piece = [&](int length) -> int {
        const int64_t left = (int64_t)length - first_frame * 32;
        return (int)(left <= 0 ? 0 : (left < piece_samples ? left : piece_samples));
    };
    constexpr int TURN = 2;                                                // frames per turned block
    constexpr int LPR = TURN * 4;                                          // lanes (16 bytes each) per row
    constexpr int RPI = 64 / LPR;                                          // rows per store instruction
    __shared__ int4 s_turn[64 * (LPR + 1)];                                // rows one int4 apart from a multiple of 8: no conflicts
    const int sample_count = in_piece(t.length[slot]);
    const bool live = sample_count > 0;
    const int frame_count = (sample_count + 31) / 32;
    const int my_pairs = (sample_count / 32) / TURN * (TURN / 2);          // whole blocks of TURN full frames of this lane's row
    int wave_pairs = my_pairs;                                             // ... of the longest row of the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) wave_pairs = max(wave_pairs, __shfl_xor(wave_pairs, o));
    // (a lane without frames here stays at its row's start: nothing before the buffer, nothing far behind it is touched)
    const uint32_t *src = reinterpret_cast<const uint32_t *>(adpcm + t.adx_off[slot] + (live ? first_frame * 18 : 0));
    int16_t *dst = pcm + t.pcm_off[slot] + (live ? first_frame * 32 : 0);
    // the rows this lane stores to: row (lane / LPR + RPI * i) of the group, 16 bytes at (lane % LPR) * 8 of every block
    int64_t row_at[LPR];
    int row_pairs[LPR];
#pragma unroll
    for (int i = 0; i < LPR; i++) {
        const int r = g * 64 + lane / LPR + RPI * i;
        row_at[i] = t.pcm_off[r] + first_frame * 32 + (lane % LPR) * 8;
        row_pairs[i] = (in_piece(t.length[r]) / 32) / TURN * (TURN / 2);
    }
    int hist1 = k > 0 ? 0 : p.history, hist2 = hist1;                      // later pieces: the guess (0, 0)
    if (REPAIR && live) {
        hist1 = dst[-1];
        hist2 = dst[-2];
    }
    bool bad = false;
    // one frame whose 18 bytes are w[0 .. 4] (adx_decode_frame), and where its samples go
    auto decode_frame = [&](const uint32_t (&w)[5], auto mode_tag, int frame, int valid) {
        constexpr int MODE = decltype(mode_tag)::value;          // 0: whole frame, into the turn block; 1: whole frame, stored by its lane; 2: partial
        int o[32];
        adx_decode_frame<V4, false>(w, p, hist1, hist2, bad, o);
        if (MODE == 0) {
            int4 *mine = s_turn + lane * (LPR + 1) + (frame % TURN) * 4;
#pragma unroll
            for (int q = 0; q < 4; q++) mine[q] = adx_pack8(o, q);
        } else if (MODE == 1) {
            adx_store_frame(dst + (int64_t)frame * 32, o);
        } else if (MODE == 2) {
            int16_t *d = dst + (int64_t)frame * 32;
#pragma unroll
            for (int s2 = 0; s2 < 32; s2++)
                if (s2 < valid) d[s2] = (int16_t)o[s2];
        }
    };
    // ---- warm-up of a later piece (adx_decode_warm_up: never in front of the row)
    if (!REPAIR && k > 0 && live) {
        adx_decode_warm_up<V4>(src, first_frame, p, hist1, hist2, bad);
        bad = false;                                                       // (those frames belong to the piece before)
    }
    // ---- whole pairs of full frames: 36 bytes from a dword boundary, the next pair's loads in flight meanwhile; a lane
    // without a pair (left) reads the 36 bytes at its row's start / its last pair again: inside its row, or the rows and
    // the guard behind it
    uint32_t cur[9], nxt[9];
    {
#pragma unroll
        for (int q = 0; q < 9; q++) cur[q] = src[q];
#pragma unroll
        for (int q = 0; q < 9; q++) asm volatile("" : "+v"(cur[q]));       // waited for here, not on the loop's back edge
    }
#pragma unroll 1
    for (int j = 0; j < wave_pairs; j++) {
        const uint32_t *f = src + (int64_t)max(min(j + 1, my_pairs - 1), 0) * 9;
#pragma unroll
        for (int q = 0; q < 9; q++) nxt[q] = f[q];
        uint32_t a[5], b[5];
        adx_split_pair(cur, a, b);
        const int keep1 = hist1, keep2 = hist2;
        const bool keep_bad = bad;
        decode_frame(a, std::integral_constant<int, 0>{}, 0, 32);
        decode_frame(b, std::integral_constant<int, 0>{}, 1, 32);
        if (j >= my_pairs) {                                               // this lane's row has no such pair: what it decoded is nobody's
            hist1 = keep1;
            hist2 = keep2;
            bad = keep_bad;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < LPR; i++) {                                    // read, wait, store -- one at a time
            int16_t *q = j < row_pairs[i] ? pcm + row_at[i] + (int64_t)j * (TURN * 32) : reinterpret_cast<int16_t *>(sink + lane);
            adx_store16(q, s_turn[(lane / LPR + RPI * i) * (LPR + 1) + lane % LPR]);
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int q = 0; q < 9; q++) cur[q] = nxt[q];
    }
    // ---- what is left of the lane's piece: fewer than TURN full frames and a partial one
#pragma unroll 1
    for (int i = 2 * my_pairs; i < frame_count; i++) {
        uint32_t w[5];
        adx_load_frame(src, i, w);
        const int valid = min(32, sample_count - i * 32);
        if (valid == 32) decode_frame(w, std::integral_constant<int, 1>{}, i, 32);
        else decode_frame(w, std::integral_constant<int, 2>{}, i, valid);
    }
    if (bad && live && status) atomicOr(status + t.channel[slot], 1);
}

// The ragged ADX side of the seam protocol (seams.hpp): lane = slot on the packed rows, the slot's own length
template <bool V4>
struct AdxRaggedDecodeSeams {
    static constexpr int FRAME_SAMPLES = 32, FRAME_BYTES = 18;
    static constexpr int SLOW_SEAM = ADX_DECODE_SLOW_SEAM, SLOW_POLL = 128, TAIL_BUDGET = ADX_DECODE_TAIL_BUDGET;
    static constexpr bool HAS_OWN = false;
    const uint8_t *adpcm; AdxRaggedTables t; AdxDeviceParams p; int16_t *pcm;
    const uint8_t *src; int16_t *dst;                                    // (open)
    __device__ int channel(int slot) const { return slot; }
    __device__ int length(int slot, int) const { return t.length[slot]; }
    __device__ int64_t own(int, int total) const { return total; }
    __device__ void open(int slot)
    {
        src = adpcm + t.adx_off[slot];
        dst = pcm + t.pcm_off[slot];
    }
    __device__ void decode(const uint8_t *fr, int valid, int &h1, int &h2, int16_t *o) const { adx_decode_frame_serial<V4>(fr, p, valid, h1, h2, o); }
};

template <bool V4>
__global__ __launch_bounds__(64) void adx_decode_fs18_fixup_ragged_kernel(
    const uint8_t *__restrict__ adpcm, AdxRaggedTables t, int seg_frames, AdxDeviceParams p, int16_t *__restrict__ pcm,
    int *__restrict__ first_open, int *__restrict__ seam_open, int force_open, int *__restrict__ slow_seams)
{
    seam_fixup(AdxRaggedDecodeSeams<V4>{adpcm, t, p, pcm}, t.slots, 0, seg_frames, first_open, seam_open, force_open, slow_seams);
}

template <bool V4>
__global__ __launch_bounds__(64) void adx_decode_fs18_tail_ragged_kernel(
    const uint8_t *__restrict__ adpcm, AdxRaggedTables t, int seg_frames, int segments, AdxDeviceParams p, int16_t *__restrict__ pcm,
    int *__restrict__ first_open, const int *__restrict__ seam_open, int force_open, int *__restrict__ slow_seams)
{
    seam_tail(AdxRaggedDecodeSeams<V4>{adpcm, t, p, pcm}, t.slots, 0, seg_frames, segments, first_open, seam_open, force_open,
              slow_seams);
}

// ---------------------------------------------------------------- launchers
int launch_encode_ragged(const int16_t *d_pcm, const AdxRaggedTables &t, const AdxRaggedItems &plan, bool time_pieces, int cus,
                         const AdxDeviceParams &p, uint8_t *d_adx, int16_t *d_history_out, void *workspace, hipStream_t stream)
{
    if (t.nch <= 0) return VGA_OK;
    const int groups = t.slots / 64;
    if (!time_pieces) {
        hipLaunchKernelGGL(adx_encode_ragged_kernel, dim3(groups), dim3(64), 0, stream, d_pcm, t, p, d_adx, d_history_out);
        VGA_HIP_TRY(hipGetLastError());
        return VGA_OK;
    }
    const bool v4 = p.version == 4, ex = p.type == 4;
    const int segments = plan.segments, seg_frames = plan.seg_frames;
    // (without V4 every channel's history is the parameter set's: a fill, the kernel writes none)
    if (!v4 && d_history_out)
        VGA_HIP_TRY(hipMemsetD16Async(reinterpret_cast<hipDeviceptr_t>(d_history_out), (unsigned short)(int16_t)p.history, (size_t)t.nch, stream));
    if (plan.count <= 0) return VGA_OK;
    int16_t *seg_state = nullptr;
    int *first_open = nullptr, *seam_open = nullptr, *seam_end = nullptr, *queue = nullptr;
    uint2 *crumbs = nullptr;
    if (segments > 1) {
        unsigned char *ws = static_cast<unsigned char *>(workspace);
        int64_t lane_frames = 0;                       // (the crumbs follow the small arrays whatever their size)
        const EncodeWorkspace w = cut_encode_workspace(t.slots, segments, lane_frames);
        seg_state = reinterpret_cast<int16_t *>(ws + w.state_at);
        first_open = reinterpret_cast<int *>(ws + w.first_open_at);
        seam_open = reinterpret_cast<int *>(ws + w.seam_open_at);
        seam_end = reinterpret_cast<int *>(ws + w.seam_end_at);
        queue = reinterpret_cast<int *>(ws + w.queue_at);
        crumbs = reinterpret_cast<uint2 *>(ws + w.crumbs_at);
        VGA_HIP_TRY(fill_no_open_seams(first_open, t.slots, stream));
        VGA_HIP_TRY(hipMemsetAsync(seam_open, 0, w.flag_bytes, stream));
        VGA_HIP_TRY(hipMemsetAsync(queue, 0, 16, stream));
    }
    int *open_seams = queue ? queue + 1 : nullptr;     // seams still open at the end of their pieces
    const int many = force_open_seams() == 3 ? 1 : many_open_seams(t.nch, segments);
    int fixup_waves = (int)std::min<int64_t>((int64_t)cus * 4, ((int64_t)t.slots * (segments - 1) + 63) / 64);
    if (fixup_waves < 1) fixup_waves = 1;
    return adx_with_version_and_type(v4, ex, [&](auto v, auto e) -> int {
        constexpr bool V = decltype(v)::value, E = decltype(e)::value;
        hipLaunchKernelGGL((adx_encode_fs18_direct_ragged_kernel<V, E>), dim3(plan.count), dim3(64), 0, stream, d_pcm, t, plan.items,
                           seg_frames, p, d_adx, d_history_out, seg_state, crumbs, (const int *)nullptr, (const int *)nullptr, 0);
        VGA_HIP_TRY(hipGetLastError());
        if (segments > 1) {
            hipLaunchKernelGGL((adx_encode_fs18_fixup_ragged_kernel<V, E>), dim3(fixup_waves), dim3(64), 0, stream, d_pcm, t, seg_frames,
                               segments, p, d_adx, seg_state, crumbs, first_open, seam_open, seam_end, force_open_seams(), queue,
                               open_seams);
            VGA_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL((adx_encode_fs18_tail_ragged_kernel<V, E>), dim3(groups), dim3(64), 0, stream, d_pcm, t, seg_frames,
                               segments, p, d_adx, seg_state, first_open, seam_open, seam_end, force_open_seams(), open_seams, many);
            VGA_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL((adx_encode_fs18_direct_ragged_kernel<V, E, true>), dim3(groups), dim3(64), 0, stream, d_pcm, t,
                               plan.items, seg_frames, p, d_adx, (int16_t *)nullptr, seg_state, (uint2 *)nullptr,
                               (const int *)first_open, (const int *)open_seams, many);
            VGA_HIP_TRY(hipGetLastError());
        }
        return VGA_OK;
    });
}

int launch_decode_ragged(const uint8_t *d_adx, const AdxRaggedTables &t, const AdxRaggedItems &plan, bool time_pieces,
                         const AdxDeviceParams &p, int16_t *d_pcm, int *d_status, void *workspace, hipStream_t stream)
{
    if (t.nch <= 0) return VGA_OK;
    const int groups = t.slots / 64;
    if (!time_pieces) {
        hipLaunchKernelGGL(adx_decode_ragged_kernel, dim3(groups), dim3(64), 0, stream, d_adx, t, p, d_pcm, d_status);
        VGA_HIP_TRY(hipGetLastError());
        return VGA_OK;
    }
    if (plan.count <= 0) return VGA_OK;
    const int segments = plan.segments, seg_frames = plan.seg_frames;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    const DecodeWorkspace w = cut_decode_workspace(t.slots, segments);
    int *first_open = reinterpret_cast<int *>(ws + w.first_open_at);
    int *seam_open = reinterpret_cast<int *>(ws + w.seam_open_at);
    int *slow_seams = reinterpret_cast<int *>(ws + w.slow_at);
    int4 *sink = reinterpret_cast<int4 *>(ws + w.sink_at);
    if (segments > 1) {
        VGA_HIP_TRY(fill_no_open_seams(first_open, t.slots, stream));
        VGA_HIP_TRY(hipMemsetAsync(seam_open, 0, w.flag_bytes + 16, stream));
        VGA_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(slow_seams + 1), many_open_seams(t.nch, segments), 1, stream));
    }
    return adx_with_version(p.version == 4, [&](auto v) -> int {
        constexpr bool V = decltype(v)::value;
        hipLaunchKernelGGL((adx_decode_fs18_direct_ragged_kernel<V, false>), dim3(plan.count), dim3(64), 0, stream, d_adx, t, plan.items,
                           seg_frames, p, d_pcm, d_status, (const int *)nullptr, (const int *)nullptr, sink);
        VGA_HIP_TRY(hipGetLastError());
        if (segments > 1) {
            hipLaunchKernelGGL(adx_decode_fs18_fixup_ragged_kernel<V>, dim3(groups, segments - 1), dim3(64), 0, stream, d_adx, t,
                               seg_frames, p, d_pcm, first_open, seam_open, force_open_seams(), slow_seams);
            VGA_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(adx_decode_fs18_tail_ragged_kernel<V>, dim3(groups), dim3(64), 0, stream, d_adx, t, seg_frames, segments,
                               p, d_pcm, first_open, (const int *)seam_open, force_open_seams(), slow_seams);
            VGA_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL((adx_decode_fs18_direct_ragged_kernel<V, true>), dim3(groups), dim3(64), 0, stream, d_adx, t, plan.items,
                               seg_frames, p, d_pcm, d_status, (const int *)first_open, (const int *)slow_seams, sink);
            VGA_HIP_TRY(hipGetLastError());
        }
        return VGA_OK;
    });
}

}  // namespace adx
}  // namespace vga
