// adx_device.hpp -- the device-side pieces the CRI ADX kernel files share (adx_kernels.hip: equal-length rows at a pitch;
// adx_ragged_kernels.hip: packed rows of different lengths): the reference's arithmetic, one frame of the encoder and of
// the decoder, the 16-byte accesses on 2-byte boundaries and the encoder's seam run.
#pragma once
#include "common.hpp"
#include "adx_kernels.hpp"

#include <type_traits>

namespace vga {
namespace adx {

__device__ __forceinline__ int clamp16(int v) { return min(max(v, -32768), 32767); }
__device__ __forceinline__ int clamp4(int v) { return min(max(v, -8), 7); }

// Utilities/Helpers.cs:146-163 == floor(log2(v)) for v >= 1
__device__ __forceinline__ int log2_floor(int v) { return 31 - __builtin_clz((unsigned)v); }

// CriAdxCodec.cs:149-165
__device__ __forceinline__ int calculate_scale(int max_distance, bool exponential, double &gain, int &scale_to_write)
{
    int scale = (max_distance - 1) / 7 + 1;
    if (scale > 0x1000) scale = 0x1000;
    scale_to_write = scale - 1;
    if (exponential) {
        const int power = scale_to_write == 0 ? 0 : log2_floor(scale_to_write) + 1;
        scale = 1 << power;
        scale_to_write = 12 - power;
        max_distance = 8 * scale - 1;
    }
    gain = max_distance == 0 ? 0.0 : 32767.0 / (double)max_distance;
    return scale;
}

// (int)double the way RyuJIT x64 does it (cvttsd2si): out of range -> int.MinValue.  v_cvt_i32_f64 saturates,
// which differs for a POSITIVE overflow only (rawDistance * gain >= 2^31: needs max_distance <= 8 and a
// reconstruction far off the input -- not seen on audio, but the reference's answer is defined).
__device__ __forceinline__ int trunc_i32_ryujit(double v)
{
    const int i = (int)v;
    return v >= 2147483648.0 ? (int)0x80000000 : i;
}

// CriAdxCodec.cs:167-171
__device__ __forceinline__ int scale_short_to_nibble(int sample)
{
    const int sign = (sample > 0) - (sample < 0);
    sample = (sample + 2340 * sign) / 4681;     // short.MaxValue/14, short.MaxValue/7
    return clamp4(sample);
}

// One sample of the quantise recurrence (CriAdxCodec.cs:122-138) for the 18-byte-frame kernels, arranged so that the
// chain from the newest reconstructed sample `b` to the next one is ten instructions (the encoder wave's rate is what
// these kernels run at).  Returns u = q + 7 (0..14); (a, b) move on one sample.  Needs |c0|, |c1| <= 16384 (launch_encode
// checks; the reference's coefficients are at most 8192, CriAdxCodec.cs:173-191).
//  * rawDistance = (x - (a c1 >> 12)) - (b c0 >> 12) = (((x - (a c1 >> 12)) << 12) + 4095 - b c0) >> 12: subtracting a floor
//    is adding the ceiling of the negative, and ceil(n / 4096) = floor((n + 4095) / 4096); below 2^31 for such coefficients;
//  * ScaleShortToNibble (:167-171), truncating division of s + 2340 sign(s) by 4681, is floor((s + 2340) / 4681) for
//    either sign (-floor((|s| + 2340) / d) = ceil((s - 2340) / d) = floor((s - 2340 + d - 1) / d), d - 1 = 4680); with
//    t = s + 2340 + 7 * 4681 >= 2339 that is (t * 57346 >> 28) - 7: 57346 * 4681 = 2^28 + 1170, exact while
//    4680 * 57346 + 1170 k < 2^28 (k = t / 4681 <= 48; here <= 14), and t * 57346 < 2^32.  -7 .. 7: Clamp4 cannot bind, nor
//    the Clamp16 of scale * q (scale <= 4096);
//  * the sample is Clamp16(scale * q + predicted) = Clamp16(scale * u + (predicted - 7 scale)).
template <bool V4, bool GUARD>
__device__ __forceinline__ int adx_quantise_step(int x, int &a, int &b, int c0, int c1, double gain, int scale, int scale7)
{
    const int ac1 = __mul24(a, c1);                          // the older sample's share: ready a step early
    const int xb = x - (ac1 >> 12);
    const int k = (xb << 12) + 4095;
    const int raw = (__mul24(b, -c0) + k) >> 12;
    const double prod = (double)raw * gain;
    const int scaled = clamp16(GUARD ? trunc_i32_ryujit(prod) : (int)prod);
    const unsigned u = (unsigned)(__mul24(scaled, 57346) + 35107 * 57346) >> 28;
    const int predicted = V4 ? (__mul24(b, c0) + ac1) >> 12 : (__mul24(b, c0) >> 12) + (ac1 >> 12);
    const int rec = clamp16(__mul24(scale, (int)u) + (predicted - scale7));
    a = b;
    b = rec;
    return (int)u;
}

// 16 bytes to / from any 2-byte boundary (the rows of a padded stream, see adx_encode_fs18_direct_kernel): one
// global_store_dwordx4 / global_load_dwordx4 either way, the type only tells hipcc not to assume more
typedef int adx_i32x4_a2 __attribute__((ext_vector_type(4), aligned(2)));
__device__ __forceinline__ void adx_store16(int16_t *q, int4 v)
{
    adx_i32x4_a2 t;
    t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
    *reinterpret_cast<adx_i32x4_a2 *>(q) = t;
}

constexpr int ADX_DECODE_WARM_FRAMES = 512;           // even: a piece's frames keep their alignment
constexpr int ADX_DECODE_SLOW_SEAM = 1024;            // frames a seam may stay open before it counts as slow (a multiple of 128)
constexpr int ADX_DECODE_TAIL_BUDGET = 2048;          // frames one lane of the tail kernel decodes again before it hands over

// One frame of CriAdxCodec.Decode (:23-45) from the history (hist1, hist2) into o[0 .. valid).  `fr` = the frame's first byte:
// 2 bytes past a dword boundary for odd frames (rows are dword-aligned in these kernels); the 18 bytes arrive as five dword
// loads from the boundary at or before them and a whole frame leaves as four 16-byte stores (round 5: a byte load per two
// samples and a 2-byte store per sample until then -- 4 us a frame on a path that can walk a whole channel).
template <bool V4>
__device__ __forceinline__ void adx_decode_frame_serial(const uint8_t *fr, const AdxDeviceParams &p, int valid, int &hist1,
                                                        int &hist2, int16_t *o)
{
    const bool odd = (reinterpret_cast<uintptr_t>(fr) & 2) != 0;
    const uint32_t *f32 = reinterpret_cast<const uint32_t *>(fr - (odd ? 2 : 0));
    uint32_t t[5], w[5];
#pragma unroll
    for (int q = 0; q < 5; q++) t[q] = f32[q];
#pragma unroll
    for (int q = 0; q < 4; q++) w[q] = odd ? (t[q] >> 16) | (t[q + 1] << 16) : t[q];
    w[4] = odd ? t[4] >> 16 : t[4];
    const int hb0 = w[0] & 0xff, hb1 = (w[0] >> 8) & 0xff;
    int filter_num = ((hb0 >> 4) & 0xF) >> 1;
    int cf0, cf1;
    if (p.type == 2) {                                  // the fixed filters (CriAdxCodec.cs:186-191)
        if (filter_num > 3) filter_num = 3;
        cf0 = filter_num == 0 ? 0 : (filter_num == 1 ? 0x0F00 : (filter_num == 2 ? 0x1CC0 : 0x1880));
        cf1 = filter_num == 0 ? 0 : (filter_num == 1 ? 0 : (filter_num == 2 ? (int)(int16_t)0xF300 : (int)(int16_t)0xF240));
    } else {
        cf0 = p.coef0;
        cf1 = p.coef1;
    }
    int scale = (int)(int16_t)(((hb0 << 8) | hb1) & 0x1FFF);
    scale = (int)(int16_t)(p.type == 4 ? (1 << ((12 - scale) & 31)) : scale + 1);
    int out[32];
#pragma unroll
    for (int s2 = 0; s2 < 32; s2++) {
        const int b = 2 + (s2 >> 1);                    // the byte that holds sample s2: high nibble first
        int sample = __builtin_amdgcn_sbfe((int)w[b >> 2], 8 * (b & 3) + ((s2 & 1) ? 0 : 4), 4);
        if (V4) sample = scale * sample + ((hist1 * cf0 + hist2 * cf1) >> 12);
        else sample = scale * sample + ((hist1 * cf0) >> 12) + ((hist2 * cf1) >> 12);
        const int fin = clamp16(sample);
        if (s2 < valid) {
            hist2 = hist1;
            hist1 = fin;
        }
        out[s2] = fin;
    }
    if (valid == 32) {                                  // (a padded stream's frames start at any 2-byte boundary: adx_store16)
#pragma unroll
        for (int q = 0; q < 4; q++)
            adx_store16(o + 8 * q,
                        make_int4((out[8 * q] & 0xFFFF) | (out[8 * q + 1] << 16), (out[8 * q + 2] & 0xFFFF) | (out[8 * q + 3] << 16),
                                  (out[8 * q + 4] & 0xFFFF) | (out[8 * q + 5] << 16), (out[8 * q + 6] & 0xFFFF) | (out[8 * q + 7] << 16)));
    } else {
        for (int s2 = 0; s2 < valid; s2++) o[s2] = (int16_t)out[s2];
    }
}

// A frame's 32 input samples as the 16 dwords they are loaded as; sample j sign-extended (one v_bfe_i32 / v_ashrrev, or an
// SDWA operand, where it is used: 32 unpacked samples are 32 live registers)
__device__ __forceinline__ int adx_sample(const uint32_t (&xw)[16], int j)
{
    return (j & 1) ? (int)xw[j >> 1] >> 16 : (int)(int16_t)(xw[j >> 1] & 0xFFFFu);
}

// The pre-scan (CriAdxCodec.cs:112-118) of the 30 distances whose history is input only (samples 2..31): max |Clamp16(d)|
// from the two signed extremes (clamp and magnitude are monotone on either side of zero: two instructions per sample
// less than clamping each).  The encoder's pieces leave it in their crumbs, the seam runs take it from there.
__device__ __forceinline__ int adx_prescan30(const uint32_t (&xw)[16], int c0, int c1)
{
    int hi = 0, lo = 0;
#pragma unroll
    for (int j = 2; j < 32; j++) {
        // 16-bit x 16-bit: exact in 24 bits
        const int d = (adx_sample(xw, j) - (__mul24(adx_sample(xw, j - 1), c0) >> 12)) - (__mul24(adx_sample(xw, j - 2), c1) >> 12);
        hi = max(hi, d);
        lo = min(lo, d);
    }
    return max(clamp16(hi), -clamp16(lo));
}

// One frame of CriAdxCodec.EncodeFrame (:107-147) from the history (a, b); maths as adx_encode_kernel.  pm30 = adx_prescan30(xw).
// The frame leaves as its 16 header bits (low byte = the frame's first byte) and four dwords of nibbles in memory order
// (frame bytes 2..17: eight samples a dword, the first sample in the high nibble of the lowest byte).
template <bool V4, bool EXPONENTIAL>
__device__ __forceinline__ void adx_encode_frame_packed(const uint32_t (&xw)[16], int &a, int &b, int c0, int c1, int filter_bits, int pm30,
                                                        uint32_t &hdr, uint32_t (&nib)[4])
{
    int max_distance;
    {                                                    // the two distances that see the reconstructed history
        const int x0 = adx_sample(xw, 0), x1 = adx_sample(xw, 1);
        const int d0 = (x0 - (__mul24(b, c0) >> 12)) - (__mul24(a, c1) >> 12);
        const int d1 = (x1 - (__mul24(x0, c0) >> 12)) - (__mul24(b, c1) >> 12);
        max_distance = max(max(clamp16(max(d0, d1)), -clamp16(min(d0, d1))), pm30);
    }
    double gain;
    int scale_out;
    const int scale = calculate_scale(max_distance, EXPONENTIAL, gain, scale_out);
    hdr = (uint32_t)((((scale_out >> 8) & 0x1f) | filter_bits) & 0xff) | ((uint32_t)(scale_out & 0xff) << 8);
    // the quantise recurrence (:122-138) (adx_quantise_step), and the RyuJIT overflow semantics of the cast only for a frame
    // whose gain can push rawDistance past 2^31 (a wave-uniform, practically never taken branch).  Eight samples' u = q + 7
    // are gathered into a dword a nibble at a time (u <= 14: no carries), first sample on top; the nibble of q is
    // (u + 9) mod 16 = (u + 1) ^ 8 -- one add and one xor for all eight -- and memory order wants the bytes reversed.
    const int scale7 = 7 * scale;
    auto quantise = [&](auto guard_c) __attribute__((always_inline)) {
        constexpr bool GUARD = decltype(guard_c)::value;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            uint32_t acc = 0;
#pragma unroll
            for (int j = 8 * w; j < 8 * w + 8; j++)
                acc = (acc << 4) + (uint32_t)adx_quantise_step<V4, GUARD>(adx_sample(xw, j), a, b, c0, c1, gain, scale, scale7);
            nib[w] = __builtin_bswap32((acc + 0x11111111u) ^ 0x88888888u);
        }
    };
    const double raw_bound = 32770.0 + 8.0 * (double)((c0 < 0 ? -c0 : c0) + (c1 < 0 ? -c1 : c1));
    if (__any(gain * raw_bound >= 2147483648.0)) quantise(std::true_type{});
    else quantise(std::false_type{});
}

// The same as nine 16-bit words (low byte = the earlier byte of the frame): for the seam runs' 16-bit stores.
template <bool V4, bool EXPONENTIAL>
__device__ __forceinline__ void adx_encode_frame_words(const uint32_t (&xw)[16], int &a, int &b, int c0, int c1, int filter_bits, int pm30,
                                                       uint32_t (&fw)[9])
{
    uint32_t nib[4];
    adx_encode_frame_packed<V4, EXPONENTIAL>(xw, a, b, c0, c1, filter_bits, pm30, fw[0], nib);
#pragma unroll
    for (int w = 0; w < 4; w++) {
        fw[1 + 2 * w] = nib[w] & 0xFFFFu;
        fw[2 + 2 * w] = nib[w] >> 16;
    }
}

// A frame with fewer than 32 samples left (zero padded, :86-91), or any frame a sample at a time
// (first: the stream's first real sample -- the positions before it are the reference's untouched, zero, buffer slots of a
// padded stream, CriAdxCodec.cs:78-91, and `src` must not be read there)
__device__ __forceinline__ void adx_load_frame_slow(const int16_t *src, int64_t f, int total_length, uint32_t (&xw)[16], int first = 0)
{
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int64_t i0 = f * 32 + 2 * j;
        const uint32_t lo = (i0 >= first && i0 < total_length) ? (uint16_t)src[i0] : 0u;
        const uint32_t hi = (i0 + 1 >= first && i0 + 1 < total_length) ? (uint16_t)src[i0 + 1] : 0u;
        xw[j] = lo | (hi << 16);
    }
}

typedef uint32_t adx_u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t adx_u32x4_a2 __attribute__((ext_vector_type(4), aligned(2)));
__device__ __forceinline__ uint4 adx_load16(const int16_t *q)
{
    const adx_u32x4_a2 v = *reinterpret_cast<const adx_u32x4_a2 *>(q);
    return make_uint4(v.x, v.y, v.z, v.w);
}

// From the TRUE history (ta, tb) at the start of piece k: encode again frame by frame next to a replay of the run whose
// bytes the piece holds (decoded from ITS start history (sa, sb), before they are overwritten), until both histories
// coincide at a frame end.  Returns true when the piece ended first; (ta, tb) is then the true history at its end.
template <bool V4, bool EXPONENTIAL>
__device__ __forceinline__ bool adx_encode_seam_run(const int16_t *__restrict__ src, uint8_t *__restrict__ dst, int64_t f0, int seg_frames,
                                                    int total_length, int c0, int c1, int filter_bits, int &ta, int &tb, int sa, int sb,
                                                    int ch, int k, int force_open)
{
    // lane = channel, so every load of the wave touches 64 different rows: a frame is fetched as four 16-byte loads of PCM
    // and nine 16-bit loads of the old frame (instead of 32 + 18 scalar loads), one frame ahead of its use (clamped,
    // unconditional), and leaves as nine 16-bit stores.  All lanes of a wave are at the same frame (same seam index).
    const int64_t full_frames = total_length / 32;     // frames with all 32 samples (>= 64 here: pieces are that long at least)
    auto fetch = [&](int64_t f, uint4 (&px)[4], uint32_t (&fw)[9]) {
        const int64_t fc = f < full_frames ? f : full_frames - 1;
#pragma unroll
        for (int i = 0; i < 4; i++) px[i] = adx_load16(src + fc * 32 + 8 * i);
        const uint16_t *q = reinterpret_cast<const uint16_t *>(dst + fc * 18);
#pragma unroll
        for (int i = 0; i < 9; i++) fw[i] = q[i];
    };
    uint4 px[4], nx[4];
    uint32_t ow[9], nw[9];
    fetch(f0, px, ow);
    for (int64_t f = f0; f < f0 + seg_frames && f * 32 < total_length; f++) {
        fetch(f + 1, nx, nw);                           // in flight during this frame
        uint32_t xw[16];
        if (f < full_frames) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                xw[4 * i] = px[i].x; xw[4 * i + 1] = px[i].y; xw[4 * i + 2] = px[i].z; xw[4 * i + 3] = px[i].w;
            }
        } else {                                        // the zero-padded last frame: its own loads
            adx_load_frame_slow(src, f, total_length, xw);
            const uint16_t *q = reinterpret_cast<const uint16_t *>(dst + f * 18);
#pragma unroll
            for (int i = 0; i < 9; i++) ow[i] = q[i];
        }
        // the guessed run's reconstruction of this frame (CriAdxCodec.Decode :23-45)
        int scale = (int)(int16_t)((((ow[0] & 0xff) << 8) | (ow[0] >> 8)) & 0x1FFF);
        scale = (int)(int16_t)(EXPONENTIAL ? (1 << ((12 - scale) & 31)) : scale + 1);
#pragma unroll
        for (int j = 0; j < 32; j++) {
            const int bi = 2 + (j >> 1);                // frame byte
            const int byte = (int)((ow[bi >> 1] >> (8 * (bi & 1))) & 0xff);
            int v = (j & 1) ? (byte & 0xF) : (byte >> 4);
            v = (v ^ 8) - 8;
            if (V4) v = __mul24(scale, v) + ((__mul24(sb, c0) + __mul24(sa, c1)) >> 12);
            else v = __mul24(scale, v) + (__mul24(sb, c0) >> 12) + (__mul24(sa, c1) >> 12);
            sa = sb;
            sb = clamp16(v);
        }
        uint32_t fw[9];
        adx_encode_frame_words<V4, EXPONENTIAL>(xw, ta, tb, c0, c1, filter_bits, adx_prescan30(xw, c0, c1), fw);
        uint16_t *o = reinterpret_cast<uint16_t *>(dst + f * 18);
#pragma unroll
        for (int i = 0; i < 9; i++) o[i] = (uint16_t)fw[i];
        if (ta == sa && tb == sb && !seam_forced_open(force_open, ch, k)) return false;   // closed: the rest of the piece stands
#pragma unroll
        for (int i = 0; i < 4; i++) px[i] = nx[i];
#pragma unroll
        for (int i = 0; i < 9; i++) ow[i] = nw[i];
    }
    return true;
}

constexpr int ADX_FIXUP_REFILL = 8;

// Encode (CriAdxCodec.cs:56-105) of one channel, any frame size: the stream the frames are cut from is `padding` untouched
// (zero) buffer slots followed by the PCM, zero padded at the end; frames lying entirely inside
// the padding are skipped (their bytes stay zero, :86).
__device__ __forceinline__ void adx_encode_channel(const int16_t *__restrict__ src, int pcm_length, const AdxDeviceParams &p,
                                                   uint16_t *__restrict__ dst, int16_t *__restrict__ history_out)
{
    const int spf = (p.frame_size - 2) * 2;
    const int sample_count = pcm_length + p.padding;
    const int frame_count = (sample_count + spf - 1) / spf;
    const int c0 = p.coef0, c1 = p.coef1;
    const int words_per_frame = p.frame_size / 2;

    int h0 = 0, h1 = 0;                       // pcmBuffer[0], pcmBuffer[1]
    int hist = p.history;
    if (p.version == 4 && p.padding == 0 && pcm_length > 0) {
        h0 = h1 = src[0];                     // :69-74
        hist = src[0];
    }
    if (history_out) *history_out = (int16_t)hist;

    for (int i = 0; i < frame_count; i++) {
        uint16_t *frame = dst + (int64_t)i * words_per_frame;
        const int t0 = i * spf;                                   // first stream position of this frame
        if (min(t0 + spf, sample_count) <= p.padding) {           // whole frame is padding: skipped (:86)
            for (int w = 0; w < words_per_frame; w++) frame[w] = 0;
            continue;
        }
        // stream position t -> sample: 0 inside the padding and past the end
        auto sample_at = [&](int j) -> int {
            const int idx = t0 + j - p.padding;
            return (idx >= 0 && idx < pcm_length) ? (int)src[idx] : 0;
        };

        // pre-scan :112-118 (raw inputs, reconstructed history)
        int max_distance = 0;
        {
            int a = h0, b = h1;
            for (int j = 0; j < spf; j++) {
                const int x = sample_at(j);
                const int predicted = ((b * c0) >> 12) + ((a * c1) >> 12);
                int distance = clamp16(x - predicted);
                distance = distance < 0 ? -distance : distance;
                max_distance = max(max_distance, distance);
                a = b;
                b = x;
            }
        }
        double gain;
        int scale_out;
        const int scale = calculate_scale(max_distance, p.type == 4, gain, scale_out);

        // header :140-141, + filter bits for the Fixed type :95
        int b0 = (scale_out >> 8) & 0x1f;
        if (p.type == 2) b0 |= (p.filter << 5) & 0xff;
        frame[0] = (uint16_t)(b0 | ((scale_out & 0xff) << 8));

        // quantise :122-138
        int a = h0, b = h1;
        uint32_t word = 0;
        for (int j = 0; j < spf; j++) {
            const int x = sample_at(j);
            int predicted = ((b * c0) >> 12) + ((a * c1) >> 12);
            const int raw = x - predicted;
            const int scaled = clamp16(trunc_i32_ryujit((double)raw * gain));
            const int q = scale_short_to_nibble(scaled);
            const int decoded_distance = clamp16(scale * q);
            if (p.version == 4) predicted = (b * c0 + a * c1) >> 12;
            const int rec = clamp16(decoded_distance + predicted);
            a = b;
            b = rec;
            // bytes are (even<<4 | odd&15); two bytes per little-endian u16
            const int sh = ((j & 2) ? 8 : 0) + ((j & 1) ? 0 : 4);
            word |= (uint32_t)(q & 0xF) << sh;
            if ((j & 3) == 3) {
                frame[1 + (j >> 2)] = (uint16_t)word;
                word = 0;
            }
        }
        h0 = a;                                                    // :98-99
        h1 = b;
    }
}

// Decode (CriAdxCodec.cs:9-54) of one channel; a frame that names a filter the table lacks ORs 1 into *status
__device__ __forceinline__ void adx_decode_channel(const uint8_t *__restrict__ src, int sample_count, const AdxDeviceParams &p,
                                                   int16_t *__restrict__ dst, int *__restrict__ status)
{
    const int spf = (p.frame_size - 2) * 2;
    const int frame_count = (sample_count + spf - 1) / spf;

    int hist1 = p.history, hist2 = p.history;
    int current = 0;
    int start_sample = p.padding > 0 ? p.padding % spf : 0;
    int64_t in_index = (int64_t)(p.padding / spf) * p.frame_size;
    bool bad = false;

    for (int i = 0; i < frame_count; i++) {
        const int hb0 = src[in_index], hb1 = src[in_index + 1];
        int filter_num = ((hb0 >> 4) & 0xF) >> 1;
        int cf0, cf1;
        if (p.type == 2) {
            // CriAdxCodec.cs:186-191; an index past the table throws in the reference
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
        in_index += 2 + start_sample / 2;

        const int to_read = min(spf, sample_count - current);
        for (int s = start_sample; s < to_read; s++) {
            const int byte = src[in_index];
            int sample = (s & 1) ? (byte & 0xF) : (byte >> 4);
            if (s & 1) in_index++;
            sample = (sample ^ 8) - 8;
            if (p.version == 4)
                sample = scale * sample + ((hist1 * cf0 + hist2 * cf1) >> 12);
            else
                sample = scale * sample + ((hist1 * cf0) >> 12) + ((hist2 * cf1) >> 12);
            const int fin = clamp16(sample);
            hist2 = hist1;
            hist1 = fin;
            dst[current++] = (int16_t)fin;
        }
        start_sample = 0;
    }
    for (; current < sample_count; current++) dst[current] = 0;     // `new short[sampleCount]` tail
    if (bad && status) atomicOr(status, 1);
}

}  // namespace adx
}  // namespace vga
