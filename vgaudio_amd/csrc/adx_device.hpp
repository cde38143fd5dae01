// adx_device.hpp -- the device side of the CRI ADX kernels, each body written once: the reference's arithmetic, one frame of
// the encoder and of the decoder, the 16-byte accesses on 2-byte boundaries, the encoder's seam run -- and the 18-byte-frame
// time-piece bodies themselves: the encoder's piece, fix-up queue and tail lane, and the decoder's frame arithmetic, pack,
// frame load, pair split and warm-up.  The __global__ kernels of adx_kernels.hip (equal-length rows at a pitch) and
// adx_ragged_kernels.hip (packed rows of different lengths) are shells over them: a shell works out its lane's index and
// piece, the early returns and the start history, and hands the body a ROW POLICY (AdxPitchedRows / AdxPackedRows, as the
// decoders' seam policies of seams.hpp) that says where the lane's rows are and how long.
#pragma once
#include "common.hpp"
#include "adx_kernels.hpp"
#include "seams.hpp"

#include <type_traits>

#ifndef VGA_ADX_ABLATE                                  // timing-only builds of the encoder's piece (tools/time_adx_ablations.sh)
#define VGA_ADX_ABLATE 0
#endif

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

// ---- the decoders' frame-level pieces (adx_decode_fs18_direct_kernel and its ragged form, adx_decode_frame_serial)
// Samples o[8 q .. 8 q + 7] as the 16 bytes they are stored as
__device__ __forceinline__ int4 adx_pack8(const int (&o)[32], int q)
{
    return make_int4((o[8 * q] & 0xFFFF) | (o[8 * q + 1] << 16), (o[8 * q + 2] & 0xFFFF) | (o[8 * q + 3] << 16),
                     (o[8 * q + 4] & 0xFFFF) | (o[8 * q + 5] << 16), (o[8 * q + 6] & 0xFFFF) | (o[8 * q + 7] << 16));
}

// A whole frame's 64 bytes to any 2-byte boundary
__device__ __forceinline__ void adx_store_frame(int16_t *d, const int (&o)[32])
{
#pragma unroll
    for (int q = 0; q < 4; q++) adx_store16(d + 8 * q, adx_pack8(o, q));
}

// The 18 bytes of one frame as w[0 .. 4] (little-endian dwords, two bytes of slack) from `f`, the dword boundary at or before
// them: the frame starts there (even frames of a dword-aligned row) or two bytes behind it (odd ones)
__device__ __forceinline__ void adx_load_frame(const uint32_t *f, bool odd, uint32_t (&w)[5])
{
    uint32_t t[5];
#pragma unroll
    for (int q = 0; q < 5; q++) t[q] = f[q];
#pragma unroll
    for (int q = 0; q < 4; q++) w[q] = odd ? (t[q] >> 16) | (t[q + 1] << 16) : t[q];
    w[4] = odd ? t[4] >> 16 : t[4];
}
// ... frame i of a dword-aligned row
__device__ __forceinline__ void adx_load_frame(const uint32_t *row, int i, uint32_t (&w)[5])
{
    adx_load_frame(reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint16_t *>(row) + (int64_t)i * 9 - (i & 1)), (i & 1) != 0, w);
}

// An even frame and the one after it, 36 bytes from a dword boundary, as two frames: the second starts two bytes into c9[4]
__device__ __forceinline__ void adx_split_pair(const uint32_t (&c9)[9], uint32_t (&a)[5], uint32_t (&b)[5])
{
#pragma unroll
    for (int q = 0; q < 5; q++) a[q] = c9[q];
#pragma unroll
    for (int q = 0; q < 4; q++) b[q] = (c9[4 + q] >> 16) | (c9[5 + q] << 16);
    b[4] = c9[8] >> 16;
}

// The arithmetic of one frame of CriAdxCodec.Decode (:23-45) whose 18 bytes are w[0 .. 4]: the header, one v_bfe_i32 per
// nibble and the recurrence (:36-45), from the history (hist1, hist2) into o[0 .. 32).  `bad`: the frame names a filter the
// table lacks.  SKIP (the frame in which a padded stream's samples begin, :21-33): the samples below `skip` are not decoded
// at all -- they leave the history alone.  A partial last frame runs on: nothing reads the history after it.
template <bool V4, bool SKIP>
__device__ __forceinline__ void adx_decode_frame(const uint32_t (&w)[5], const AdxDeviceParams &p, int &hist1, int &hist2, bool &bad,
                                                 int (&o)[32], int skip = 0)
{
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
#pragma unroll
    for (int s = 0; s < 32; s++) {
        const int b = 2 + (s >> 1);                                        // the byte that holds sample s: high nibble first
        const int nib = __builtin_amdgcn_sbfe((int)w[b >> 2], 8 * (b & 3) + ((s & 1) ? 0 : 4), 4);
        int sample;
        if (V4) {                                      // :38-39
            int rest = __mul24(hist2, cf1);
            asm("" : "+v"(rest));
            sample = __mul24(scale, nib) + ((__mul24(hist1, cf0) + rest) >> 12);
        } else {                                       // :41-42
            int rest = (__mul24(hist2, cf1) >> 12) + __mul24(scale, nib);
            asm("" : "+v"(rest));
            sample = (__mul24(hist1, cf0) >> 12) + rest;
        }
        const int fin = clamp16(sample);
        if (!SKIP || s >= skip) {
            hist2 = hist1;
            hist1 = fin;
        }
        o[s] = fin;
    }
}

// The warm-up of a later piece: the ADX_DECODE_WARM_FRAMES frames before `src`, the piece's first frame (fewer where the row
// starts sooner: first_frame frames lie before the piece), are decoded from the history given -- the guess (0, 0) -- and not stored, so that the piece itself starts from a history that has, as a rule, already
// fallen into step with the true run (the decoder forgets a wrong history within 2000 samples on audio): its seam then closes
// on the first frame the fix-up launch checks (15 seams per channel at configs[2]: 3.7 ms of fix-up without this, against
// 7.9 ms for the decode itself)
template <bool V4>
__device__ __forceinline__ void adx_decode_warm_up(const uint32_t *src, int64_t first_frame, const AdxDeviceParams &p, int &hist1, int &hist2,
                                                   bool &bad)
{
    const int warm = (int)(first_frame < ADX_DECODE_WARM_FRAMES ? first_frame : ADX_DECODE_WARM_FRAMES);      // even
    const uint32_t *wsrc = src - (int64_t)warm / 2 * 9;
#pragma unroll 1
    for (int k = 0; k < warm / 2; k++) {
        uint32_t c9[9], a[5], b[5];
        int o[32];
#pragma unroll
        for (int q = 0; q < 9; q++) c9[q] = wsrc[(int64_t)k * 9 + q];
        adx_split_pair(c9, a, b);
        adx_decode_frame<V4, false>(a, p, hist1, hist2, bad, o);
        adx_decode_frame<V4, false>(b, p, hist1, hist2, bad, o);
    }
}

// One frame of CriAdxCodec.Decode (:23-45) from the history (hist1, hist2) into o[0 .. valid).  `fr` = the frame's first byte:
// 2 bytes past a dword boundary for odd frames (rows are dword-aligned in these kernels); the 18 bytes arrive as five dword
// loads from the boundary at or before them and a whole frame leaves as four 16-byte stores (round 5: a byte load per two
// samples and a 2-byte store per sample until then -- 4 us a frame on a path that can walk a whole channel).
template <bool V4>
__device__ __forceinline__ void adx_decode_frame_serial(const uint8_t *fr, const AdxDeviceParams &p, int valid, int &hist1,
                                                        int &hist2, int16_t *o)
{
    const bool odd = (reinterpret_cast<uintptr_t>(fr) & 2) != 0;
    uint32_t w[5];
    adx_load_frame(reinterpret_cast<const uint32_t *>(fr - (odd ? 2 : 0)), odd, w);
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
        adx_store_frame(o, out);
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

// ---------------------------------------------------------------- the rows of the 18-byte-frame encoder's lanes
// A row policy answers, for the lane index it was opened on (a channel, or a work slot), where the lane's PCM and ADX rows
// are, how long its stream is and where its crumbs and its (piece, lane) state live.  Passed by value; open() fills in what
// is per lane.  AdxPitchedRows: equal-length rows at a pitch -- all but the row pointers and `own` are expressions of kernel
// arguments, i.e. wave-uniform.  AdxPackedRows (below): the tables of a packed batch.
struct AdxPitchedRows {
    static constexpr bool HAS_OWN = true;              // own_frames: a channel may be a shorter stream zero-padded to total_length
    static constexpr bool PADDED = true;               // the stream may begin with `padding` positions that are never read
    const int16_t *pcm; int64_t pcm_pitch; uint8_t *adx; int64_t adx_pitch; int nch, total_length, padding;
    const int *own_frames; uint2 *crumbs;              // crumbs: [frame][channel]
    const int16_t *src; uint8_t *dst; int i; int64_t own;                               // (open)
    __device__ void open(int ch)
    {
        i = ch;
        own = own_frames ? (int64_t)own_frames[ch] : frames();
        src = pcm + (int64_t)ch * pcm_pitch;
        dst = adx + (int64_t)ch * adx_pitch;
    }
    __device__ int length() const { return total_length; }                              // in stream positions
    __device__ int64_t frames() const { return ((int64_t)total_length + 31) / 32; }
    __device__ int64_t full_frames() const { return total_length / 32; }                // frames with all 32 samples
    __device__ int first() const { return padding; }                                    // the first position that may be read
    __device__ int64_t own_end() const { return own; }                                  // the frames that are anybody's output
    __device__ int64_t state(int k) const { return (int64_t)k * nch + i; }              // seg_state / seam_open / seam_end of (piece, lane)
    __device__ bool has_crumbs() const { return crumbs != nullptr; }
    __device__ uint2 &crumb(int64_t f) const { return crumbs[f * nch + i]; }
    // what the fix-up queue hands out: (lane, seam) pairs lane-fastest, of the pieces that exist
    __device__ int lanes() const { return nch; }
    __device__ int seams(int seg_frames, int segments) const
    {
        const int pieces = (int)((frames() + seg_frames - 1) / seg_frames);
        return (pieces < segments ? pieces : segments) - 1;
    }
};

// slot = group * 64 + lane; the crumbs of a group are the block [group_frames][64] at t.crumb_base[group].  The queue also
// hands out the pairs of channels that ended before the seam: a pop each.
struct AdxPackedRows {
    static constexpr bool HAS_OWN = false, PADDED = false;
    const int16_t *pcm; AdxRaggedTables t; uint8_t *adx; uint2 *crumbs;
    const int16_t *src; uint8_t *dst; uint2 *crumb_row; int i, total_length; int64_t n_frames, n_full;   // (open)
    __device__ void open(int slot)
    {
        i = slot;
        total_length = t.length[slot];
        n_frames = ((int64_t)total_length + 31) / 32;
        n_full = total_length / 32;
        src = pcm + t.pcm_off[slot];
        dst = adx + t.adx_off[slot];
        crumb_row = crumbs ? crumbs + t.crumb_base[slot >> 6] + (slot & 63) : nullptr;
    }
    __device__ int length() const { return total_length; }
    __device__ int64_t frames() const { return n_frames; }
    __device__ int64_t full_frames() const { return n_full; }
    __device__ int first() const { return 0; }
    __device__ int64_t own_end() const { return n_frames; }
    __device__ int64_t state(int k) const { return (int64_t)k * t.slots + i; }
    __device__ bool has_crumbs() const { return crumb_row != nullptr; }
    __device__ uint2 &crumb(int64_t f) const { return crumb_row[f * 64]; }
    __device__ int lanes() const { return t.slots; }
    __device__ int seams(int, int segments) const { return segments - 1; }
};

// ---------------------------------------------------------------- the encoder's piece (adx_encode_fs18_direct_kernel, its ragged form)
// Piece k of the lane `r` is opened on, from the history (a, b): the frames [k seg_frames, (k + 1) seg_frames) of its stream --
// REPAIR: to the stream's end, no crumbs, no final history.  A lane reads its own frames two at a time and writes eight
// frames at a time; every length, end and clamp is the lane's own (uniform over the wave for AdxPitchedRows).
template <bool V4, bool EXPONENTIAL, bool REPAIR, class Rows>
__device__ __forceinline__ void adx_encode_piece(const Rows &r, int k, int seg_frames, const AdxDeviceParams &p, int a, int b,
                                                 int16_t *seg_state)
{
    const int16_t *src = r.src;
    uint8_t *dst = r.dst;
    const int total_length = r.length();
    const int64_t f0 = (int64_t)k * seg_frames;
    if (REPAIR) seg_frames = 0x7fffff00 / 32 - (int)f0;                                // ... to the end of the stream
    [[maybe_unused]] const bool leave_crumbs = !REPAIR && r.has_crumbs() && k > 0;
    const int c0 = p.coef0, c1 = p.coef1;
    const int filter_bits = p.type == 2 ? ((p.filter << 5) & 0xff) : 0;
    const int64_t frames = r.frames(), full_frames = r.full_frames();
    const int64_t fe = f0 + seg_frames < frames ? f0 + seg_frames : frames;
    // Two frames (one 128-byte line of the lane's row) are loaded together, the pair after them in flight meanwhile: the
    // halves of a line loaded a frame apart did not survive in the L1 between the two (30.5 GB fetched for 23.6).
    auto fetch2 = [&](int64_t f, uint4 (&px)[8]) {     // unconditional, clamped to the last full frames of this row
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
#if VGA_ADX_ABLATE & 4                                  // (timing-only builds: tools/build_variants.sh)
        const int pm30 = (int)(xw[5] & 0x7FFFu);
#else
        const int pm30 = adx_prescan30(xw, c0, c1);
#endif
        adx_encode_frame_packed<V4, EXPONENTIAL>(xw, a, b, c0, c1, filter_bits, pm30, hdr, nib);
        // the crumb of this frame, for the seam that may run over it: the history this run leaves it with and the part
        // of the pre-scan that does not depend on any history (a wave's 64 crumbs are 512 contiguous bytes)
#if !(VGA_ADX_ABLATE & 3)
        if (leave_crumbs) r.crumb(f) = make_uint2(((uint32_t)a & 0xFFFFu) | ((uint32_t)b << 16), (uint32_t)pm30);
#endif
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
    // Eight frames at a time: their 144 bytes leave as nine 16-byte stores (whole lines for the L2 to write back, where 36
    // bytes per pair of frames left partial ones: 17.0 GB written for 9.6).  Groups of eight need full frames: a lane whose
    // stream ends inside a group finishes with the slow frame.
    const int64_t fe8 = fe < full_frames ? fe : full_frames;
    auto encode_slow = [&](int64_t f) {                 // a frame loaded a sample at a time (zero outside the stream's samples)
        uint32_t xw[16], hdr, nib[4];
        adx_load_frame_slow(src, f, total_length, xw, r.first());
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
    if (Rows::PADDED && !REPAIR && k == 0 && r.first() > 0) {
        // the head of a padded stream: frames up to the first even one that lies wholly behind the padding
        int64_t fh = ((int64_t)r.first() + 31) / 32;
        fh += fh & 1;
        for (; f < fh && f < fe; f++) {
            const int64_t end = (f + 1) * 32 < total_length ? (f + 1) * 32 : total_length;
            if (end <= r.first()) {                     // wholly inside the padding: skipped, its bytes stay zero (:84-86)
                uint16_t *d = reinterpret_cast<uint16_t *>(dst + f * 18);
#pragma unroll
                for (int i = 0; i < 9; i++) d[i] = 0;
            } else
                encode_slow(f);
        }
    }
    if (f + 8 <= fe8) fetch2(f, cur);
    for (; f + 8 <= fe8; f += 8) {
        uint32_t w[36];
        auto pair = [&](auto pr_c) __attribute__((always_inline)) {                    // (a lambda per pair: constant indices into w)
            constexpr int pr = decltype(pr_c)::value;
            uint32_t he, ho, ne[4], no[4];
#if VGA_ADX_ABLATE & 8                                  // no loads after the first: the same frames over and over
            if (f == f0 && pr == 0) fetch2(f + 2, nxt);
#else
            fetch2(f + 2 * pr + 2, nxt);
#endif
            encode(f + 2 * pr, cur, std::integral_constant<int, 0>{}, he, ne);
            encode(f + 2 * pr + 1, cur, std::integral_constant<int, 1>{}, ho, no);
            // 36 bytes: header, 16 bytes of nibbles, header, 16 bytes of nibbles
            uint32_t *d = w + 9 * pr;
            d[0] = he | (ne[0] << 16);
            d[1] = (ne[0] >> 16) | (ne[1] << 16);
            d[2] = (ne[1] >> 16) | (ne[2] << 16);
            d[3] = (ne[2] >> 16) | (ne[3] << 16);
            d[4] = (ne[3] >> 16) | (ho << 16);
            d[5] = no[0]; d[6] = no[1]; d[7] = no[2]; d[8] = no[3];
#if !(VGA_ADX_ABLATE & 8)
#pragma unroll
            for (int i = 0; i < 8; i++) cur[i] = nxt[i];
#endif
            __builtin_amdgcn_sched_barrier(0);          // (the next pair's work stays behind this one: registers)
        };
        pair(std::integral_constant<int, 0>{});
        pair(std::integral_constant<int, 1>{});
        pair(std::integral_constant<int, 2>{});
        pair(std::integral_constant<int, 3>{});
#if VGA_ADX_ABLATE & 2
        if (w[0] == 0x12345678u && w[35] == 0x9abcdef0u && w[17] == 77u) dst[f * 18] = 1;
#else
        adx_u32x4_a4 *d = reinterpret_cast<adx_u32x4_a4 *>(dst + f * 18);              // f - f0 is a multiple of 8, f0 even, the row dword-aligned
#pragma unroll
        for (int i = 0; i < 9; i++) {
            adx_u32x4_a4 v;
            v.x = w[4 * i]; v.y = w[4 * i + 1]; v.z = w[4 * i + 2]; v.w = w[4 * i + 3];
            d[i] = v;
        }
#endif
    }
    for (; f < fe; f++) encode_slow(f);                 // what is left of the piece, the zero-padded last frame included
    if (seg_state && !REPAIR) {
        int16_t *st = seg_state + r.state(k) * 2;
        st[0] = (int16_t)a;
        st[1] = (int16_t)b;
    }
}

// ---------------------------------------------------------------- the encoder's fix-up queue (adx_encode_fs18_fixup_kernel, its ragged form)
// Every seam of the batch -- (lane, piece) pairs -- from a queue, a LANE at a time.
// A seam is a serial run of unknown length (at configs[2]: 200 frames on average, 2500 for the longest of 127 000; the
// lengths are close to exponentially distributed, tests/host/analysis/adx_seam_stats.c), so a wave that kept 64 seams
// until the last of them closed would run 1000 frames for 200 frames of work per lane.  Here a lane whose seam has closed
// takes the next one (the wave asks the queue when ADX_FIXUP_REFILL lanes are idle), and the launch lasts about as long as
// its longest seam run by a wave that has its SIMD to itself.
// The guessed run's crumbs stand in for a replay of its bytes (adx_encode_seam_run, which the tail kernel keeps): per frame
// one 8-byte load replaces nine 16-bit loads and the 32-sample decode, and the pre-scan is down to the two distances
// that see the history -- 650 instructions per frame instead of 1100.
// A lane's frame is loaded an iteration ahead (a lane that has just taken a seam sits its first iteration out).
// A seam exists where the lane's own stream reaches piece k, and its run ends with the lane's own frames (own_end(): what
// a seam does in the zero padding behind them is nobody's business -- and in digital silence the two runs need never meet:
// the run from the true history settles on a small non-zero fixed point of the predictor's floors, the guessed run on zero;
// round 5's ragged call of 10 008 files spent 100 ms per bucket chaining such seams through the padding of the bucket's
// shortest file).  `r` arrives with no lane opened: its row pointers at the bases.
template <bool V4, bool EXPONENTIAL, class Rows>
__device__ __forceinline__ void adx_encode_fixup(Rows r, int seg_frames, int segments, const AdxDeviceParams &p,
                                                 const int16_t *seg_state, int *first_open,
                                                 int *seam_open, int *seam_end, int force_open,
                                                 int *queue, int *open_seams)
{
    const int lane = threadIdx.x;
    const int c0 = p.coef0, c1 = p.coef1;
    const int filter_bits = p.type == 2 ? ((p.filter << 5) & 0xff) : 0;
    const int lanes = r.lanes();
    const int items = lanes * r.seams(seg_frames, segments);
    bool active = false, have = false, drained = false;
    int k = 0, ta = 0, tb = 0;
    int64_t f = 0, fend = 0;
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
                if (idx < items) {                      // lane-fastest: neighbouring lanes start on neighbouring crumbs
                    k = 1 + idx / lanes;
                    r.open(idx - (k - 1) * lanes);
                    f = (int64_t)k * seg_frames;
                    fend = f + seg_frames < r.frames() ? f + seg_frames : r.frames();
                    ta = seg_state[r.state(k - 1) * 2];
                    tb = seg_state[r.state(k - 1) * 2 + 1];
                    active = f < r.own_end();           // a seam behind the lane's own frames: nothing to do
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
            const int64_t fc = fl < r.full_frames() ? fl : r.full_frames() - 1;       // (>= 2 full frames where a seam exists)
#pragma unroll
            for (int i = 0; i < 4; i++) nxt[i] = adx_load16(r.src + fc * 32 + 8 * i);
            ncr = r.crumb(fc);
        }
        if (active && have) {
            uint32_t xw[16];
            if (f < r.full_frames()) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    xw[4 * i] = cur[i].x; xw[4 * i + 1] = cur[i].y; xw[4 * i + 2] = cur[i].z; xw[4 * i + 3] = cur[i].w;
                }
            } else {                                    // the zero-padded last frame: its own loads
                adx_load_frame_slow(r.src, f, r.length(), xw);
                ccr = r.crumb(f);
            }
            uint32_t fw[9];
            adx_encode_frame_words<V4, EXPONENTIAL>(xw, ta, tb, c0, c1, filter_bits, (int)ccr.y, fw);
            uint16_t *o = reinterpret_cast<uint16_t *>(r.dst + f * 18);
#pragma unroll
            for (int i = 0; i < 9; i++) o[i] = (uint16_t)fw[i];
            const int sa = (int)(int16_t)(ccr.x & 0xFFFFu), sb = (int)ccr.x >> 16;       // the guessed run's history after this frame
            f++;
            if (ta == sa && tb == sb && !seam_forced_open(force_open, r.i, k)) {
                active = false;                         // closed: the rest of the piece stands
            } else if (f >= r.own_end()) {
                active = false;                         // the lane's own frames are all written
            } else if (f >= fend) {
                // still open at the end of its piece: the chain launch carries on from the history reached here
                seam_open[r.state(k - 1)] = 1;
                seam_end[r.state(k - 1)] = (int)(((unsigned)tb << 16) | ((unsigned)ta & 0xFFFFu));
                atomicMin(&first_open[r.i], k);
                // (seams the test hook holds open count only in its REPAIR mode, 3: the chained tail has tests of its own)
                if (!seam_forced_open(force_open, r.i, k) || force_open == 3) atomicAdd(open_seams, 1);
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

// ---------------------------------------------------------------- the encoder's tail lane (adx_encode_fs18_tail_kernel, its ragged form)
// The lanes with an open seam, piece after piece (lanes without one leave at once) -- the encoder's counterpart of the
// decoders' chained tail kernels and of gc_encode_chain_kernel: where the true history at the start of piece k is not
// seg_state[k - 1], which the fix-up launch assumed, the piece holds the run from seg_state[k - 1]; the same seam run from
// the true history finds where the two meet.  A run that does not meet by the end of the piece carries on; a later open
// seam of the lane starts again from its recorded end.  (Round 1 encoded the rest of the channel serially: 0.7 s for a
// 60 s channel.)
template <bool V4, bool EXPONENTIAL, class Rows>
__device__ __forceinline__ void adx_encode_tail(Rows r, int i, int seg_frames, int segments, const AdxDeviceParams &p,
                                                const int16_t *seg_state, const int *first_open,
                                                const int *seam_open, const int *seam_end, int force_open,
                                                const int *open_seams, int many)
{
    if (open_seams[0] >= many) return;                 // many seams that would not close: the REPAIR launch takes them all
    const int k0 = first_open[i];
    if (k0 <= 0 || k0 >= SEAM_OPEN_LIMIT) return;      // (!is_open(k0), spelt out: the call compiles to another compare)
    r.open(i);
    const int c0 = p.coef0, c1 = p.coef1;
    const int filter_bits = p.type == 2 ? ((p.filter << 5) & 0xff) : 0;
    bool carry = false;
    int ta = 0, tb = 0;
    for (int k = k0; k < segments; k++) {
        const int64_t f0 = (int64_t)k * seg_frames;
        if (f0 * 32 >= r.length() || (Rows::HAS_OWN && f0 >= r.own_end())) break;
        const int64_t idx = r.state(k - 1);
        bool apart = false;
        if (carry)
            apart = adx_encode_seam_run<V4, EXPONENTIAL>(r.src, r.dst, f0, seg_frames, r.length(), c0, c1, filter_bits, ta, tb,
                                                         seg_state[idx * 2], seg_state[idx * 2 + 1], i, k, force_open);
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

// The kernels' compile-time switches from the parameter set: f(V4) / f(V4, EXPONENTIAL) with std::bool_constant tags
template <class F>
inline int adx_with_version(bool v4, F &&f)
{
    return v4 ? f(std::true_type{}) : f(std::false_type{});
}
template <class F>
inline int adx_with_version_and_type(bool v4, bool exponential, F &&f)
{
    return adx_with_version(v4, [&](auto v) { return exponential ? f(v, std::true_type{}) : f(v, std::false_type{}); });
}

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
