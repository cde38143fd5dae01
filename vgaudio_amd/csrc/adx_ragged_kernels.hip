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
// These are separate kernels: the equal-length instantiations of adx_kernels.hip are what they were.
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
    const int total_length = t.length[slot];           // this lane's own
    const int64_t f0 = (int64_t)k * seg_frames;
    if (f0 * 32 >= total_length) return;               // the channel ended before this piece (or holds nothing at all)
    if (REPAIR) {
        seg_frames = 0x7fffff00 / 32 - (int)f0;        // ... to the end of the lane's stream
        crumbs = nullptr;
    }
    const int16_t *src = pcm + t.pcm_off[slot];
    uint8_t *dst = out + t.adx_off[slot];
    uint2 *crumb_row = crumbs ? crumbs + t.crumb_base[g] + threadIdx.x : nullptr;      // [frame][lane]
    const int c0 = p.coef0, c1 = p.coef1;
    const int filter_bits = p.type == 2 ? ((p.filter << 5) & 0xff) : 0;
    int a = 0, b = 0;
    if (REPAIR) {                                      // the true history at the start of piece k
        a = seg_state[((int64_t)(k - 1) * t.slots + slot) * 2];
        b = seg_state[((int64_t)(k - 1) * t.slots + slot) * 2 + 1];
    } else if (k > 0) {                                // the guess: the input just before this piece
        a = src[f0 * 32 - 2];
        b = src[f0 * 32 - 1];
    } else if (V4) {
        a = b = src[0];                                // :69-74
        if (history_out) history_out[t.channel[slot]] = (int16_t)a;
    }
    const int64_t frames = ((int64_t)total_length + 31) / 32, full_frames = total_length / 32;
    const int64_t fe = f0 + seg_frames < frames ? f0 + seg_frames : frames;
    auto fetch2 = [&](int64_t f, uint4 (&px)[8]) {     // unconditional, clamped to the last full frames OF THIS ROW
        const int64_t fc = f + 1 < full_frames ? f : (full_frames >= 2 ? full_frames - 2 : 0);
        if (full_frames >= 2) {
#pragma unroll
            for (int i = 0; i < 8; i++) px[i] = adx_load16(src + fc * 32 + 8 * i);
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) px[i] = make_uint4(0, 0, 0, 0);
        }
    };
    auto encode_x = [&](int64_t f, const uint32_t (&xw)[16], uint32_t &hdr, uint32_t (&nib)[4]) {
        const int pm30 = adx_prescan30(xw, c0, c1);
        adx_encode_frame_packed<V4, EXPONENTIAL>(xw, a, b, c0, c1, filter_bits, pm30, hdr, nib);
        if (crumb_row && k > 0) crumb_row[f * 64] = make_uint2(((uint32_t)a & 0xFFFFu) | ((uint32_t)b << 16), (uint32_t)pm30);
    };
    auto encode = [&](int64_t f, const uint4 (&px)[8], auto half_c, uint32_t &hdr, uint32_t (&nib)[4]) {   // the pair's first or second frame
        constexpr int H = decltype(half_c)::value * 4;
        uint32_t xw[16];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            xw[4 * i] = px[H + i].x; xw[4 * i + 1] = px[H + i].y; xw[4 * i + 2] = px[H + i].z; xw[4 * i + 3] = px[H + i].w;
        }
        encode_x(f, xw, hdr, nib);
    };
    // groups of eight need full frames: a lane whose channel ends inside a group finishes with the slow frame
    const int64_t fe8 = fe < full_frames ? fe : full_frames;
    auto encode_slow = [&](int64_t f) {                 // a frame loaded a sample at a time (zero past the row's samples)
        uint32_t xw[16], hdr, nib[4];
        adx_load_frame_slow(src, f, total_length, xw, 0);
        encode_x(f, xw, hdr, nib);
        uint16_t *d = reinterpret_cast<uint16_t *>(dst + f * 18);
        d[0] = (uint16_t)hdr;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            d[1 + 2 * i] = (uint16_t)(nib[i] & 0xFFFFu);
            d[2 + 2 * i] = (uint16_t)(nib[i] >> 16);
        }
    };
    uint4 cur[8], nxt[8];
    int64_t f = f0;
    if (f + 8 <= fe8) fetch2(f, cur);
    for (; f + 8 <= fe8; f += 8) {
        uint32_t w[36];
        auto pair = [&](auto pr_c) __attribute__((always_inline)) {                    // (a lambda per pair: constant indices into w)
            constexpr int pr = decltype(pr_c)::value;
            uint32_t he, ho, ne[4], no[4];
            fetch2(f + 2 * pr + 2, nxt);
            encode(f + 2 * pr, cur, std::integral_constant<int, 0>{}, he, ne);
            encode(f + 2 * pr + 1, cur, std::integral_constant<int, 1>{}, ho, no);
            uint32_t *d = w + 9 * pr;                   // 36 bytes: header, 16 bytes of nibbles, header, 16 bytes of nibbles
            d[0] = he | (ne[0] << 16);
            d[1] = (ne[0] >> 16) | (ne[1] << 16);
            d[2] = (ne[1] >> 16) | (ne[2] << 16);
            d[3] = (ne[2] >> 16) | (ne[3] << 16);
            d[4] = (ne[3] >> 16) | (ho << 16);
            d[5] = no[0]; d[6] = no[1]; d[7] = no[2]; d[8] = no[3];
#pragma unroll
            for (int i = 0; i < 8; i++) cur[i] = nxt[i];
            __builtin_amdgcn_sched_barrier(0);          // (the next pair's work stays behind this one: registers)
        };
        pair(std::integral_constant<int, 0>{});
        pair(std::integral_constant<int, 1>{});
        pair(std::integral_constant<int, 2>{});
        pair(std::integral_constant<int, 3>{});
        adx_u32x4_a4 *d = reinterpret_cast<adx_u32x4_a4 *>(dst + f * 18);              // f - f0 is a multiple of 8, f0 even, the row 16-byte aligned
#pragma unroll
        for (int i = 0; i < 9; i++) {
            adx_u32x4_a4 v;
            v.x = w[4 * i]; v.y = w[4 * i + 1]; v.z = w[4 * i + 2]; v.w = w[4 * i + 3];
            d[i] = v;
        }
    }
    for (; f < fe; f++) encode_slow(f);                 // what is left of the lane's piece, the zero-padded last frame included
    if (seg_state && !REPAIR) {
        int16_t *st = seg_state + ((int64_t)k * t.slots + slot) * 2;
        st[0] = (int16_t)a;
        st[1] = (int16_t)b;
    }
}

// adx_encode_fs18_fixup_kernel over (slot, seam) pairs: a seam exists where the LANE's own stream reaches piece k; its run
// ends with the lane's own frames.  (The queue also hands out the pairs of channels that ended earlier: a pop each.)
template <bool V4, bool EXPONENTIAL>
__global__ __launch_bounds__(64) void adx_encode_fs18_fixup_ragged_kernel(
    const int16_t *__restrict__ pcm, AdxRaggedTables t, int seg_frames, int segments, AdxDeviceParams p, uint8_t *__restrict__ out,
    const int16_t *__restrict__ seg_state, const uint2 *__restrict__ crumbs, int *__restrict__ first_open, int *__restrict__ seam_open,
    int *__restrict__ seam_end, int force_open, int *__restrict__ queue, int *__restrict__ open_seams)
{
    const int lane = threadIdx.x;
    const int c0 = p.coef0, c1 = p.coef1;
    const int filter_bits = p.type == 2 ? ((p.filter << 5) & 0xff) : 0;
    const int nslots = t.slots;
    const int items = nslots * (segments - 1);
    bool active = false, have = false, drained = false;
    int slot = 0, k = 0, ta = 0, tb = 0, total_length = 0;
    int64_t f = 0, fend = 0, frames = 0, full_frames = 0;
    const int16_t *src = pcm;
    uint8_t *dst = out;
    const uint2 *crumb_row = crumbs;
    uint4 cur[4], nxt[4];
    uint2 ccr = make_uint2(0, 0), ncr = make_uint2(0, 0);
#pragma unroll
    for (int i = 0; i < 4; i++) cur[i] = nxt[i] = make_uint4(0, 0, 0, 0);
    for (;;) {
        const uint64_t idle = __ballot(!active);
        const int n_idle = __popcll(idle);
        if (!drained && (n_idle >= ADX_FIXUP_REFILL || n_idle == 64)) {
            int base = 0;
            if (lane == __ffsll((long long)idle) - 1) base = atomicAdd(queue, n_idle);
            base = __shfl(base, __ffsll((long long)idle) - 1);
            if (!active) {
                const int idx = base + (int)__popcll(idle & ((1ull << lane) - 1ull));
                if (idx < items) {                      // slot-fastest: neighbouring lanes start on neighbouring crumbs
                    k = 1 + idx / nslots;
                    slot = idx - (k - 1) * nslots;
                    total_length = t.length[slot];
                    frames = ((int64_t)total_length + 31) / 32;
                    full_frames = total_length / 32;    // (>= 2 where a seam exists: frames > k * seg_frames >= 2)
                    f = (int64_t)k * seg_frames;
                    fend = f + seg_frames < frames ? f + seg_frames : frames;
                    src = pcm + t.pcm_off[slot];
                    dst = out + t.adx_off[slot];
                    crumb_row = crumbs + t.crumb_base[slot >> 6] + (slot & 63);
                    ta = seg_state[((int64_t)(k - 1) * nslots + slot) * 2];
                    tb = seg_state[((int64_t)(k - 1) * nslots + slot) * 2 + 1];
                    active = f < frames;                // the channel ended before this piece: no seam
                    have = false;
                }
            }
            if (base + n_idle >= items) drained = true;
        }
        if (!__any(active)) {
            if (drained) return;
            continue;
        }
        if (active) {                                   // the frame after this one (a new seam: its first), clamped to the row
            const int64_t fl = have ? f + 1 : f;
            const int64_t fc = fl < full_frames ? fl : full_frames - 1;
#pragma unroll
            for (int i = 0; i < 4; i++) nxt[i] = adx_load16(src + fc * 32 + 8 * i);
            ncr = crumb_row[fc * 64];
        }
        if (active && have) {
            uint32_t xw[16];
            if (f < full_frames) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    xw[4 * i] = cur[i].x; xw[4 * i + 1] = cur[i].y; xw[4 * i + 2] = cur[i].z; xw[4 * i + 3] = cur[i].w;
                }
            } else {                                    // the zero-padded last frame: its own loads
                adx_load_frame_slow(src, f, total_length, xw);
                ccr = crumb_row[f * 64];
            }
            uint32_t fw[9];
            adx_encode_frame_words<V4, EXPONENTIAL>(xw, ta, tb, c0, c1, filter_bits, (int)ccr.y, fw);
            uint16_t *o = reinterpret_cast<uint16_t *>(dst + f * 18);
#pragma unroll
            for (int i = 0; i < 9; i++) o[i] = (uint16_t)fw[i];
            const int sa = (int)(int16_t)(ccr.x & 0xFFFFu), sb = (int)ccr.x >> 16;       // the guessed run's history after this frame
            f++;
            if (ta == sa && tb == sb && !seam_forced_open(force_open, slot, k)) {
                active = false;                         // closed: the rest of the piece stands
            } else if (f >= frames) {
                active = false;                         // the channel's frames are all written
            } else if (f >= fend) {
                // still open at the end of its piece: the chain launch carries on from the history reached here
                seam_open[(int64_t)(k - 1) * nslots + slot] = 1;
                seam_end[(int64_t)(k - 1) * nslots + slot] = (int)(((unsigned)tb << 16) | ((unsigned)ta & 0xFFFFu));
                atomicMin(&first_open[slot], k);
                if (!seam_forced_open(force_open, slot, k) || force_open == 3) atomicAdd(open_seams, 1);
                active = false;
            }
        }
        if (active) {
#pragma unroll
            for (int i = 0; i < 4; i++) cur[i] = nxt[i];
            ccr = ncr;
            have = true;
        }
    }
}

// adx_encode_fs18_tail_kernel: one lane per slot, on the lane's own row and length
template <bool V4, bool EXPONENTIAL>
__global__ __launch_bounds__(64) void adx_encode_fs18_tail_ragged_kernel(
    const int16_t *__restrict__ pcm, AdxRaggedTables t, int seg_frames, int segments, AdxDeviceParams p, uint8_t *__restrict__ out,
    const int16_t *__restrict__ seg_state, const int *__restrict__ first_open, const int *__restrict__ seam_open,
    const int *__restrict__ seam_end, int force_open, const int *__restrict__ open_seams, int many)
{
    const int slot = blockIdx.x * 64 + threadIdx.x;
    if (open_seams[0] >= many) return;                 // many seams that would not close: the REPAIR launch takes them all
    const int k0 = first_open[slot];
    if (k0 <= 0 || k0 >= SEAM_OPEN_LIMIT) return;
    const int total_length = t.length[slot];
    const int16_t *src = pcm + t.pcm_off[slot];
    uint8_t *dst = out + t.adx_off[slot];
    const int c0 = p.coef0, c1 = p.coef1;
    const int filter_bits = p.type == 2 ? ((p.filter << 5) & 0xff) : 0;
    bool carry = false;
    int ta = 0, tb = 0;
    for (int k = k0; k < segments; k++) {
        const int64_t f0 = (int64_t)k * seg_frames;
        if (f0 * 32 >= total_length) break;
        const int64_t idx = (int64_t)(k - 1) * t.slots + slot;
        bool apart = false;
        if (carry)
            apart = adx_encode_seam_run<V4, EXPONENTIAL>(src, dst, f0, seg_frames, total_length, c0, c1, filter_bits, ta, tb,
                                                         seg_state[idx * 2], seg_state[idx * 2 + 1], slot, k, force_open);
        if (apart) {
            carry = true;                              // (ta, tb): the true history at the end of this piece
        } else if (seam_open[idx] != 0) {
            carry = true;                              // this piece's own seam ran out of frames: its recorded end is the truth
            const int e = seam_end[idx];
            ta = (int)(int16_t)(e & 0xFFFF);
            tb = e >> 16;
        } else
            carry = false;
    }
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
    // one frame whose 18 bytes are w[0 .. 4] (little-endian dwords, two bytes of slack)
    auto decode_frame = [&](const uint32_t (&w)[5], auto mode_tag, int frame, int valid) {
        constexpr int MODE = decltype(mode_tag)::value;          // 0: whole frame, into the turn block; 1: whole frame, stored by its lane; 2: partial; 3: not stored (warm-up)
        const int hb0 = w[0] & 0xff, hb1 = (w[0] >> 8) & 0xff;
        int filter_num = ((hb0 >> 4) & 0xF) >> 1;
        int cf0, cf1;
        if (p.type == 2) {
            if (filter_num > 3) { bad = true; filter_num = 3; }
            cf0 = filter_num == 0 ? 0 : (filter_num == 1 ? 0x0F00 : (filter_num == 2 ? 0x1CC0 : 0x1880));
            cf1 = filter_num == 0 ? 0 : (filter_num == 1 ? 0 : (filter_num == 2 ? (int)(int16_t)0xF300 : (int)(int16_t)0xF240));
        } else {
            if (filter_num > 0) bad = true;
            cf0 = p.coef0;
            cf1 = p.coef1;
        }
        int scale = (int)(int16_t)(((hb0 << 8) | hb1) & 0x1FFF);
        scale = (int)(int16_t)(p.type == 4 ? (1 << ((12 - scale) & 31)) : scale + 1);
        int o[32];
#pragma unroll
        for (int s = 0; s < 32; s++) {
            const int b = 2 + (s >> 1);                                    // the byte that holds sample s: high nibble first
            const int nib = __builtin_amdgcn_sbfe((int)w[b >> 2], 8 * (b & 3) + ((s & 1) ? 0 : 4), 4);
            int sample;
            if (V4) {                                  // :38-39
                int rest = __mul24(hist2, cf1);
                asm("" : "+v"(rest));
                sample = __mul24(scale, nib) + ((__mul24(hist1, cf0) + rest) >> 12);
            } else {                                   // :41-42
                int rest = (__mul24(hist2, cf1) >> 12) + __mul24(scale, nib);
                asm("" : "+v"(rest));
                sample = (__mul24(hist1, cf0) >> 12) + rest;
            }
            const int fin = clamp16(sample);
            hist2 = hist1;                             // a partial last frame runs on: nothing reads the history after it
            hist1 = fin;
            o[s] = fin;
        }
        if (MODE == 0) {
            int4 *mine = s_turn + lane * (LPR + 1) + (frame % TURN) * 4;
#pragma unroll
            for (int q = 0; q < 4; q++)
                mine[q] = make_int4((o[8 * q] & 0xFFFF) | (o[8 * q + 1] << 16), (o[8 * q + 2] & 0xFFFF) | (o[8 * q + 3] << 16),
                                    (o[8 * q + 4] & 0xFFFF) | (o[8 * q + 5] << 16), (o[8 * q + 6] & 0xFFFF) | (o[8 * q + 7] << 16));
        } else if (MODE == 1) {
            int16_t *d = dst + (int64_t)frame * 32;
#pragma unroll
            for (int q = 0; q < 4; q++)
                adx_store16(d + 8 * q,
                            make_int4((o[8 * q] & 0xFFFF) | (o[8 * q + 1] << 16), (o[8 * q + 2] & 0xFFFF) | (o[8 * q + 3] << 16),
                                      (o[8 * q + 4] & 0xFFFF) | (o[8 * q + 5] << 16), (o[8 * q + 6] & 0xFFFF) | (o[8 * q + 7] << 16)));
        } else if (MODE == 2) {
            int16_t *d = dst + (int64_t)frame * 32;
#pragma unroll
            for (int s2 = 0; s2 < 32; s2++)
                if (s2 < valid) d[s2] = (int16_t)o[s2];
        }
    };
    // one frame of the row by its index (it starts on a dword for even i, two bytes after one for odd i)
    auto load_frame = [&](int i, uint32_t (&w)[5]) {
        const uint32_t *f = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint16_t *>(src) + (int64_t)i * 9 - (i & 1));
        uint32_t tt[5];
#pragma unroll
        for (int q = 0; q < 5; q++) tt[q] = f[q];
        if (i & 1) {
#pragma unroll
            for (int q = 0; q < 4; q++) w[q] = (tt[q] >> 16) | (tt[q + 1] << 16);
            w[4] = tt[4] >> 16;
        } else {
#pragma unroll
            for (int q = 0; q < 5; q++) w[q] = tt[q];
        }
    };
    // ---- warm-up of a later piece (see adx_decode_fs18_direct_kernel)
    if (!REPAIR && k > 0 && live) {
        const int warm = (int)(first_frame < ADX_DECODE_WARM_FRAMES ? first_frame : ADX_DECODE_WARM_FRAMES);      // even
        const uint32_t *wsrc = src - (int64_t)warm / 2 * 9;
#pragma unroll 1
        for (int j = 0; j < warm / 2; j++) {
            uint32_t c9[9];
#pragma unroll
            for (int q = 0; q < 9; q++) c9[q] = wsrc[(int64_t)j * 9 + q];
            const uint32_t a[5] = {c9[0], c9[1], c9[2], c9[3], c9[4]};
            const uint32_t b[5] = {(c9[4] >> 16) | (c9[5] << 16), (c9[5] >> 16) | (c9[6] << 16), (c9[6] >> 16) | (c9[7] << 16),
                                   (c9[7] >> 16) | (c9[8] << 16), c9[8] >> 16};
            decode_frame(a, std::integral_constant<int, 3>{}, 0, 32);
            decode_frame(b, std::integral_constant<int, 3>{}, 0, 32);
        }
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
        const uint32_t a[5] = {cur[0], cur[1], cur[2], cur[3], cur[4]};
        // the second frame starts two bytes into cur[4]
        const uint32_t b[5] = {(cur[4] >> 16) | (cur[5] << 16), (cur[5] >> 16) | (cur[6] << 16), (cur[6] >> 16) | (cur[7] << 16),
                               (cur[7] >> 16) | (cur[8] << 16), cur[8] >> 16};
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
        load_frame(i, w);
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
#define VGA_ADX_ENC_R(V, E)                                                                                              \
    {                                                                                                                    \
        hipLaunchKernelGGL((adx_encode_fs18_direct_ragged_kernel<V, E>), dim3(plan.count), dim3(64), 0, stream, d_pcm, t, \
                           plan.items, seg_frames, p, d_adx, d_history_out, seg_state, crumbs, (const int *)nullptr,     \
                           (const int *)nullptr, 0);                                                                     \
        VGA_HIP_TRY(hipGetLastError());                                                                                  \
        if (segments > 1) {                                                                                              \
            hipLaunchKernelGGL((adx_encode_fs18_fixup_ragged_kernel<V, E>), dim3(fixup_waves), dim3(64), 0, stream, d_pcm, t, \
                               seg_frames, segments, p, d_adx, seg_state, crumbs, first_open, seam_open, seam_end,      \
                               force_open_seams(), queue, open_seams);                                                   \
            VGA_HIP_TRY(hipGetLastError());                                                                              \
            hipLaunchKernelGGL((adx_encode_fs18_tail_ragged_kernel<V, E>), dim3(groups), dim3(64), 0, stream, d_pcm, t,  \
                               seg_frames, segments, p, d_adx, seg_state, first_open, seam_open, seam_end,               \
                               force_open_seams(), open_seams, many);                                                    \
            VGA_HIP_TRY(hipGetLastError());                                                                              \
            hipLaunchKernelGGL((adx_encode_fs18_direct_ragged_kernel<V, E, true>), dim3(groups), dim3(64), 0, stream, d_pcm, t, \
                               plan.items, seg_frames, p, d_adx, (int16_t *)nullptr, seg_state, (uint2 *)nullptr,        \
                               (const int *)first_open, (const int *)open_seams, many);                                  \
        }                                                                                                                \
    }
    if (v4 && ex) VGA_ADX_ENC_R(true, true)
    else if (v4) VGA_ADX_ENC_R(true, false)
    else if (ex) VGA_ADX_ENC_R(false, true)
    else VGA_ADX_ENC_R(false, false)
#undef VGA_ADX_ENC_R
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
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
#define VGA_ADX_DEC_R(V)                                                                                                 \
    {                                                                                                                    \
        hipLaunchKernelGGL((adx_decode_fs18_direct_ragged_kernel<V, false>), dim3(plan.count), dim3(64), 0, stream, d_adx, t, \
                           plan.items, seg_frames, p, d_pcm, d_status, (const int *)nullptr, (const int *)nullptr, sink); \
        VGA_HIP_TRY(hipGetLastError());                                                                                  \
        if (segments > 1) {                                                                                              \
            hipLaunchKernelGGL(adx_decode_fs18_fixup_ragged_kernel<V>, dim3(groups, segments - 1), dim3(64), 0, stream, d_adx, t, \
                               seg_frames, p, d_pcm, first_open, seam_open, force_open_seams(), slow_seams);             \
            VGA_HIP_TRY(hipGetLastError());                                                                              \
            hipLaunchKernelGGL(adx_decode_fs18_tail_ragged_kernel<V>, dim3(groups), dim3(64), 0, stream, d_adx, t, seg_frames, \
                               segments, p, d_pcm, first_open, (const int *)seam_open, force_open_seams(), slow_seams);  \
            VGA_HIP_TRY(hipGetLastError());                                                                              \
            hipLaunchKernelGGL((adx_decode_fs18_direct_ragged_kernel<V, true>), dim3(groups), dim3(64), 0, stream, d_adx, t, \
                               plan.items, seg_frames, p, d_pcm, d_status, (const int *)first_open, (const int *)slow_seams, \
                               sink);                                                                                    \
        }                                                                                                                \
    }
    if (p.version == 4) VGA_ADX_DEC_R(true)
    else VGA_ADX_DEC_R(false)
#undef VGA_ADX_DEC_R
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

}  // namespace adx
}  // namespace vga
