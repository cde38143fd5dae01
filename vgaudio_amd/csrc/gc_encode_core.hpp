// gc_encode_core.hpp -- per-lane arithmetic of the GC-ADPCM frame encoder, shared by
// the gfx950 kernel (gcadpcm_kernels.hip) and the host-side lane emulator that the
// CPU test-suite uses to check these shortcuts against the literal reference formula
// (tests/host/gc_encode_emulator.cpp).  No codec result is ever produced on the CPU in
// the product path; the host build of this header exists for testing only.
//
// Reference: VGAudio/Codecs/GcAdpcm/GcAdpcmEncoder.cs:96-171 (DspEncodeCoef).
//
// Three exact reformulations of the reference's arithmetic are used; each is proven in
// LABNOTES.md 4.1 ("GC-ADPCM encode: exact shortcuts") and exercised exhaustively by the tests:
//  (S1) pre-scan (:107-124): the signed maxDistance only needs max(d), min(d) over the
//       frame unless +M and -M both occur (rare; sequential rescan then), and the
//       halving loop has a closed form in clz().
//  (S2) quantise (:140-144): (int)((double)((float)d / 2^k) +- 0.4999999f) equals
//       (r + 2^(k-1) - 1 + (d < 0)) >> k  (arithmetic shift) with r = (int)(float)d.
//  (S3) totalDistance (:161-162) is an exact integer; 32-bit accumulation is exact under the
//       overflow bound checked per frame (pass_fast); otherwise the pass is redone literally
//       with a 64-bit sum.  Since round 8 the fast pass sums the squares of PAIRS of saturated 16-bit errors
//       (E1-E5 below): its sum is the exact one below 2^28 and "at least 2^28" otherwise.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VGA_HD __host__ __device__ __forceinline__
#else
#define VGA_HD inline
#endif

// 24-bit multiply (operands are 16/17-bit here) and optimisation barriers: VGA_OPAQUE hides a value's range or origin from
// hipcc (a 0/1 factor, a shift count it would otherwise fold per use), VGA_OPAQUE_S keeps a constant in a scalar register.
#if defined(__HIP_DEVICE_COMPILE__)
#define VGA_MUL24(a, b) __mul24((a), (b))
#define VGA_OPAQUE(v) asm("" : "+v"(v))
#define VGA_OPAQUE_S(v) asm("" : "+s"(v))
// e * e for |e| <= 65535 as an unsigned 32-bit value.  NOT __mul24: the device library writes that one as a signed C product,
// the compiler may then assume it stays below 2^31 -- it folded the first two squares of a 64-bit error sum into one 32-bit
// mad (round 5: every frame of a full-scale square came out with the wrong predictor).
static __device__ __forceinline__ uint32_t vga_square24(int e)
{
    uint32_t r;
    asm("v_mul_i32_i24 %0, %1, %1" : "=v"(r) : "v"(e));
    return r;
}
#else
#define VGA_MUL24(a, b) ((a) * (b))
#define VGA_OPAQUE(v) ((void)0)
#define VGA_OPAQUE_S(v) ((void)0)
#endif

namespace vga {
namespace gc {

VGA_HD int imin(int a, int b) { return a < b ? a : b; }
VGA_HD int imax(int a, int b) { return a > b ? a : b; }
VGA_HD int clamp16i(int v) { return imin(imax(v, -32768), 32767); }
VGA_HD int clamp4i(int v) { return imin(imax(v, -8), 7); }

// p / 2048 with C#'s truncation toward zero, three ops: sign bit, mad, shift
VGA_HD int div2048(int p)
{
    int sgn = (int)((unsigned)p >> 31);
    VGA_OPAQUE(sgn);                                   // keeps it a 0/1 factor: v_lshrrev, v_mad_u32_u24, v_ashrrev
    return (int)((unsigned)p + (unsigned)VGA_MUL24(sgn, 2047)) >> 11;
}

VGA_HD int bit_length(unsigned v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return v ? 32 - __builtin_clz(v) : 0;
#else
    int n = 0;
    while (v) { n++; v >>= 1; }
    return n;
#endif
}

// number of `maxDistance /= 2` steps of GcAdpcmEncoder.cs:119-123 for a signed maxDistance
// in [-32768, 32767]  (closed form of: while (sp <= 12 && (md > 7 || md < -8)) { md /= 2; sp++; })
VGA_HD int halvings(int md)
{
    if (md >= 0) {
        const int n = bit_length((unsigned)md) - 3;
        return n > 0 ? n : 0;
    }
    const unsigned a = (unsigned)(-md);            // truncating /2 on a negative = halving the magnitude
    int n = bit_length(a) - 4;
    if (n < 0) n = 0;
    if ((a >> n) > 8u) n++;
    return n;
}

// literal sequential pre-scan (GcAdpcmEncoder.cs:107-115); used for the rare +M/-M tie
VGA_HD int prescan_sequential(const int (&x)[16], int c0, int c1)
{
    int max_distance = 0;
    for (int s = 0; s < 14; s++) {
        const int predicted = (x[s] * c1 + x[s + 1] * c0) / 2048;
        int distance = clamp16i(x[s + 2] - predicted);
        const int ad = distance < 0 ? -distance : distance;
        const int am = max_distance < 0 ? -max_distance : max_distance;
        if (ad > am) max_distance = distance;
    }
    return max_distance;
}

// running max/min of the unclamped pre-scan distances of samples [s_begin, s_end)
VGA_HD void prescan_range(const int (&x)[16], int c0, int c1, int s_begin, int s_end, int &dmax, int &dmin)
{
    for (int s = s_begin; s < s_end; s++) {
        const int predicted = (x[s] * c1 + x[s + 1] * c0) / 2048;
        const int d = x[s + 2] - predicted;
        dmax = imax(dmax, d);
        dmin = imin(dmin, d);
    }
}

// Scale power of the FIRST quantise pass (value after the do-loop's first ++), given the
// frame-wide max/min of the unclamped distances.  Returns -100 when the signed maximum is
// ambiguous (+M and -M both present, M > 0): caller must use prescan_sequential().
// Round 9: one bit length instead of two.  With pos = clamp(dmax, 0, 32767) (but see F5), neg = clamp(-dmin, 0, 32768):
//  (F1) a positive maximum halves until pos < 8 * 2^n: n = max(bl(pos) - 3, 0), and the value after the first ++ is
//       max(n - 1, 0) = max(bl(pos) - 4, 0) = bl(pos | 15) - 4.
//  (F2) a negative one halves (its magnitude truncating) until neg < 9 * 2^n; the value wanted is the smallest m >= 0 with
//       neg < 9 * 2^(m + 1).  g(a) = (a * 58255) >> 16 is monotone and crosses 8 * 2^j exactly where a crosses 9 * 2^j, for
//       every j = 0..12: 58255 / 65536 = 8/9 + d with d = 0.778 / 65536, so g(9 * 2^j) >= 8 * 2^j, and g(9 * 2^j - 1) < 8 * 2^j
//       because 9 * 2^j * d <= 0.44 < 58255 / 65536 (the step the last unit of a is worth).  Hence neg < 9 * 2^(m+1) <=> g(neg) < 16 * 2^m,
//       and the value is bl(g(neg) | 15) - 4: the same expression as F1 on g(neg).  neg <= 32768: the product fits 31 bits.
//  (F3) the larger magnitude decides (the positive one only when strictly larger: on equal magnitudes with equal halving
//       counts either sign gives the same value); sum = pos - neg carries that sign.
//  (F4) the ambiguous case: pos == neg and the two halving counts differ, i.e. 8 * 2^j <= pos < 9 * 2^j for some j >= 0 --
//       the four leading bits of pos (of pos | 15) are 1000.  It needs sum == 0 first, so the kernel looks at it only behind
//       a wave-uniform test of sum (first_scale_power_nt + first_scale_tie); first_scale_power_from_range is the two together.
//  (F5) pos is floored at 1, not 0: a frame without a positive distance -- silence and every perfectly predicted frame have
//       dmax = dmin = 0 -- would otherwise have sum == 0 and send its wave to the tie test on every frame.  Nothing else sees
//       the difference: F1 reads pos | 15, F3 picks the negative side for dmin <= -1 either way (sum <= 0) and the positive
//       side for dmin = 0, both with the value 0, and F4 needs pos >= 8.
// Checked against the round-1 form (kept in tests/host/gc_first_scale_driver.cpp) on every pair of the callers' domain.
VGA_HD int first_scale_power_nt(int dmax, int dmin, int &sum, int &pos)
{
    pos = imin(imax(dmax, 1), 32767);                                 // F5: 1, not 0
    const int nd = imax(imin(dmin, 0), -32768);                       // -neg
    sum = pos + nd;
    const int gneg = (int)((uint32_t)VGA_MUL24(nd, -58255) >> 16);    // F2
    const int v = sum > 0 ? pos : gneg;
    return bit_length((unsigned)v | 15u) - 4;
}
// F4, for a lane with sum == 0
VGA_HD bool first_scale_tie(int pos)
{
    const int e = bit_length((unsigned)pos | 15u) - 4;
    return (pos >> e) == 8;
}
VGA_HD int first_scale_power_from_range(int dmax, int dmin)
{
    int sum, pos;
    const int s = first_scale_power_nt(dmax, dmin, sum, pos);
    // equal magnitudes with different halving counts: the sign of the reference's maxDistance depends on
    // which of +M / -M came first
    if (sum == 0 && first_scale_tie(pos)) return -100;
    return s;
}

VGA_HD int first_scale_power_from_md(int md)
{
    const int n = halvings(md);
    return n <= 1 ? 0 : n - 1;
}

// scalePower after the overflow bump loop of GcAdpcmEncoder.cs:166-168
VGA_HD int apply_bumps(int scale_power, int max_overflow)
{
    for (int v = max_overflow + 8; v > 256; v >>= 1)
        if (++scale_power >= 12) scale_power = 11;
    return scale_power;
}

struct PassOut {
    int q[14];           // the quantised samples, -8..7 (adpcmOut of GcAdpcmEncoder.cs:155)
    uint64_t total;      // totalDistance
    int max_overflow;
    int o12, o13;        // reconstructed samples 12, 13
    unsigned hist_pair;  // (o12 & 0xFFFF) | (o13 << 16): the next frame's history, as the kernel hands it on
    bool exact;          // false: the fast pass could not prove itself exact -> redo with pass_literal
                         // (true: `total` is the exact sum whatever its size; false: see E3)
};

VGA_HD uint32_t bswap32(uint32_t v)
{
    return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24);
}

// The 8 frame bytes as two little-endian dwords: byte 0 = header (predictor<<4 | scale),
// bytes 1..7 = nibbles hi-first (GcAdpcmEncoder.cs:83-93).  The nibbles are accumulated SIGNED
// (w = w*16 + q, one shift-add each); adding 0x888..8 turns the sum into the packing of the biased
// nibbles q+8 and the XOR with 0x888..8 un-biases them.
VGA_HD void pack_frame(const int (&q)[14], int predictor, int scale_power, uint32_t &d0, uint32_t &d1)
{
    uint32_t wa = 0, wb = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int s = 0; s < 14; s++) {
        if (s < 6) wa = (wa << 4) + (uint32_t)q[s];
        else       wb = (wb << 4) + (uint32_t)q[s];
    }
    wa = ((wa + 0x00888888u) ^ 0x00888888u) & 0x00FFFFFFu;
    wb = (wb + 0x88888888u) ^ 0x88888888u;
    const uint32_t header = (uint32_t)((predictor << 4) | (scale_power & 0xF));
    d0 = bswap32((header << 24) | wa);
    d1 = bswap32(wb);
}
VGA_HD void frame_words(const PassOut &r, int predictor, int scale_power, uint32_t &d0, uint32_t &d1)
{
    pack_frame(r.q, predictor, scale_power, d0, d1);
}

// Literal quantise pass: the reference's own float/double formula (:127-164), 64-bit total.
VGA_HD PassOut pass_literal(const int (&x)[16], int c0, int c1, int scale_power)
{
    PassOut r;
    const int k = scale_power + 11;
    const int scale = 1 << k;
    union { uint32_t u; float f; } inv;
    inv.u = (uint32_t)(127 - k) << 23;             // exact 2^-k: the f32 divide by 2^k is this multiply
    uint64_t total = 0;
    int max_overflow = 0;
    int o0 = x[0], o1 = x[1];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int s = 0; s < 14; s++) {
        const int predicted = o0 * c1 + o1 * c0;
        const int distance = x[s + 2] * 2048 - predicted;
        const float fq = (float)distance * inv.f;
        const double half = (distance > 0) ? (double)0.4999999f : -(double)0.4999999f;
        const int unclamped = (int)((double)fq + half);
        const int q = clamp4i(unclamped);
        const int ov = unclamped - q;
        max_overflow = imax(max_overflow, ov < 0 ? -ov : ov);
        r.q[s] = q;
        const int corrected = predicted + q * scale;
        const int recon = clamp16i((corrected + 1024) >> 11);
        const int d = x[s + 2] - recon;
        total += (uint64_t)(uint32_t)(d * d);
        o0 = o1;
        o1 = recon;
    }
    r.total = total; r.max_overflow = max_overflow; r.o12 = o0; r.o13 = o1;
    r.hist_pair = (unsigned)(o0 & 0xFFFF) | ((unsigned)o1 << 16);
    r.exact = true;
    return r;
}

// r = (int)(float)d : the reference's int -> float rounding (round-to-nearest-even to 24 bits),
// back as an integer.  |d| >= 2^31 - 64 rounds to 2^31, which does not fit: the hardware
// conversion saturates (host: same by hand) and the caller's overflow limit rejects the frame.
VGA_HD int round_through_f32(int d)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)(float)d;                       // v_cvt_f32_i32 + v_cvt_i32_f32 (saturating)
#else
    const float f = (float)d;
    if (f >= 2147483648.0f) return 2147483647;
    return (int)f;
#endif
}

// ---- packed pairs of 16-bit values (round 7) ------------------------------------------
// The fast pass keeps the two newest reconstructed samples as ONE register, (older & 0xFFFF) | (newer << 16) -- the form
// the kernel hands the history on in (PassOut::hist_pair) -- and the coefficients as (c1 & 0xFFFF) | (c0 << 16).  Two
// operations work on such pairs; the device has an instruction for each, the host build (the lane emulator of the CPU
// tests) spells out what the instruction does so that both run the same formulation.
VGA_HD uint32_t pack16(int lo, int hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }
VGA_HD int pair_lo(uint32_t v) { return (int)(int16_t)(v & 0xFFFFu); }
VGA_HD int pair_hi(uint32_t v) { return (int)v >> 16; }
// a.lo * b.lo + a.hi * b.hi + acc, halves read as int16, the sum saturated to int32: v_dot2_i32_i16 with its clamp bit.
// The bit is set for the ENCODING's sake, not for the saturation: without it hipcc takes the two-operand v_dot2c_i32_i16, whose
// accumulator is its destination -- a v_mov of the constant in front of every one (counted in the listing: the instruction
// the packed pair saves was spent again).  The three-operand form reads the constant from a scalar register.  The sum can
// reach the rails only when |b.lo| + |b.hi| > 32767 (else |sum| < 2^30 + |acc|); the fast pass calls itself inexact for such
// coefficients (S3) and the frame is encoded by pass_literal, so no product path sees a saturated sum.  The host build
// saturates the exact 64-bit sum; whether the hardware clamps per term or once is therefore nobody's business.
VGA_HD int dot2_i16(uint32_t a, uint32_t b, int acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short s16x2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b), acc, true);
#else
    const int64_t v = (int64_t)pair_lo(a) * pair_lo(b) + (int64_t)pair_hi(a) * pair_hi(b) + (int64_t)acc;
    return v > 2147483647ll ? 2147483647 : (v < -2147483648ll ? (int)-2147483648ll : (int)v);
#endif
}
// (clamp16(lo) & 0xFFFF) | (clamp16(hi) << 16)  (v_cvt_pk_i16_i32)
VGA_HD uint32_t sat_pack16(int lo, int hi)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pk_i16(lo, hi));
#else
    return pack16(clamp16i(lo), clamp16i(hi));
#endif
}
// ---- a frame's samples as packed pairs (round 8) ---------------------------------------
// The fast pass takes the frame as the seven dwords it has in memory, xw[i] = (in[2i], in[2i + 1]) = (x[2 + 2i], x[3 + 2i]),
// and forms its errors two at a time: one packed saturating subtract, one dot product of the pair with itself.
// (clamp16(a.lo - b.lo) & 0xFFFF) | (clamp16(a.hi - b.hi) << 16): v_pk_sub_i16 with its clamp bit.  The bit is part of the
// arithmetic here: a difference of two int16 needs 17 bits, unclamped 65535 would wrap to -1 (E2).
VGA_HD uint32_t pk_sub_sat_i16(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short s16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
#else
    return pack16(clamp16i(pair_lo(a) - pair_lo(b)), clamp16i(pair_hi(a) - pair_hi(b)));
#endif
}
// a.lo * b.lo + a.hi * b.hi in the reference's unchecked int arithmetic (mod 2^32): the dot product WITHOUT the clamp bit, as the
// helper wave's pre-scan uses it.  For the pre-scan, whose predictor must wrap as the reference's does (only
// (-32768, -32768) . (-32768, -32768) = 2^31 can).  hipcc makes the two-operand v_dot2c and a v_mov of the zero from it (see
// dot2_i16) -- twice a frame, not fourteen times a pass.  (Round 8 first wrote the three-operand instruction with the inline
// constant 0 as an asm statement and saved the copy; but hipcc does not look inside asm statements when it places the wait
// states a dot product's result needs -- it left `s_nop 0` where its own get `s_nop 2` -- so the builtin it is.)
VGA_HD int dot2_i16_wrap(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short s16x2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b), 0, false);
#else
    return (int)((uint32_t)(pair_lo(a) * pair_lo(b)) + (uint32_t)(pair_hi(a) * pair_hi(b)));
#endif
}
// ---- pre-scan distances in the numerator domain (round 9) --------------------------------
// The pre-scan distance of a sample is in - D / 2048 with D = a * c1 + b * c0 and C#'s division (toward zero).  With
// N = in * 2048 - D it is
//       d = floor((N + (D > 0 ? 2047 : 0)) / 2048)                                                          (N1)
//  * D > 0: D / 2048 = floor(D / 2048), so d = in + ceil(-D / 2048) = ceil(N / 2048) = floor((N + 2047) / 2048).
//  * D < 0: D / 2048 = ceil(D / 2048), so d = in + floor(-D / 2048) = floor(N / 2048).
//  * D = 0: N = in * 2048 is a multiple of 2048 and both forms give in (so "D >= 0" would do as well).
// This is the same number as in - div2048(D), without forming the quotient and without unpacking `in`.
//  (N2) for coefficients that cannot wrap (|c0| + |c1| <= 32767) |D| <= 32768 * 32767 < 2^30 and |in * 2048| <= 2^26, so
//       |N| < 2^30 + 2^27 and |N + 2047| likewise: nothing overflows, and the clamped dot product that delivers D + 1024
//       cannot saturate (P1).  Coefficients that can wrap keep the reference's unchecked sum (dot2_i16_wrap) and the quotient.
VGA_HD int numer_adjust(int N, int D_is_pos)
{
    VGA_OPAQUE(D_is_pos);                                                   // a 0/1 factor, as in div2048: v_mad_u32_u24
    return (int)((uint32_t)N + (uint32_t)VGA_MUL24(D_is_pos, 2047));
}
// A history-dependent distance of the pre-scan from P = predicted + 1024 as the pass forms it (dot2_i16 with 1024 as the
// accumulator) and the row's in * 2048 + 1024: N = in2048p - P (the 1024 cancels -- this IS the pass's d of the same
// sample, P2), D = P - 1024.  Valid where P is: |c0| + |c1| <= 32767 (P1).
VGA_HD int head_distance_numer(int in2048p, int P)
{
    const int N = (int)((uint32_t)in2048p - (uint32_t)P);
    return numer_adjust(N, (int)((uint32_t)(1024 - P) >> 31)) >> 11;                        // 1024 - P < 0  <=>  D > 0
}
// The range of samples 2..13 of ONE predictor in the numerator domain (round 14): the tile head's pre-scan word without a
// quotient per term.  pair[k] = (in[k], in[k + 1]) are the operands of sample k + 2's prediction, a2048[k] = in[k + 2] * 2048,
// ncpk = (-c1, -c0) as a packed pair (low half -c1).  Per term
//       N = dot2(pair, ncpk, a2048) = in * 2048 - D,        X = clamp(a2048, N, N + 2047),        d = X >> 11        (N1, N7)
// Returns clamp16(max d) & 0xFFFF | clamp16(min d) << 16 with max and min started at 0 -- the word
// prescan_range(x, c0, c1, 2, 14, ...) and clamp16i give.
//  (N3) the accumulator: |D| <= 32768 * (|c0| + |c1|) <= 32768 * 30720 = 2^30 - 2^26 under pass_b_coef_ok, |a2048| <= 2^26, so
//       |N| <= 2^30 and N + 2047 < 2^31 - 2048: the clamped dot product cannot saturate (its clamp bit only selects the
//       three-operand encoding, as in dot2_i16) and the add does not wrap.  The pass's row (a2048 + 1024 + 2^30) must NOT be the
//       accumulator: N + 2^30 leaves int32.
//  (N7) the sign test and the bias of N1 as one median.  a2048 = N + D, so clamp(a2048, N, N + 2047) = N + clamp(D, 0, 2047):
//         D <= 0:         X = N, N1's numerator;
//         D >= 2047:      X = N + 2047, N1's numerator;
//         0 < D < 2047:   X = a2048, where N1 has N + 2047 = a2048 + (2047 - D): both lie in [a2048, a2048 + 2047) and a2048 is
//                         a multiple of 2048, so both shift to the same d = in (the quotient D / 2048 is 0).
//       The lower bound is not above the upper one, so the median of the three IS the clamp (v_med3_i32).  Its operand N + 2047
//       is formed by the compiler from the dot product's result, so the median stands behind the wait states that result
//       needs although it is an asm statement (see dot2_i16_wrap, med3_i32).
//  (N4) x -> x >> 11 is monotone, so max_k (X_k >> 11) = (max_k X_k) >> 11 and likewise for the minimum; the start value 0 is
//       0 >> 11.  One shift per predictor and side, the running max / min over the X (v_max3 / v_min3 over pairs of terms).
//  (N5) the two clamps and the packing are sat_pack16 (one v_cvt_pk_i16_i32): |X >> 11| <= 2^19 + 1 needs them.
//  (N6) -c must fit int16: c = -32768 cannot be negated.  pass_b_coef_ok bounds |c0| + |c1| by 30720, so wherever this form is
//       valid no coefficient is below -30720.  Callers that cannot vouch for the bound keep prescan_range's form.
VGA_HD int med3_i32(int v, int lo, int hi);
VGA_HD uint32_t prescan_numer_word(const uint32_t (&pair)[12], const int (&a2048)[12], uint32_t ncpk)
{
    int xmax = 0, xmin = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 12; k += 2) {
        const int N0 = dot2_i16(pair[k], ncpk, a2048[k]);
        const int N1 = dot2_i16(pair[k + 1], ncpk, a2048[k + 1]);
        const int X0 = med3_i32(a2048[k], N0, N0 + 2047);
        const int X1 = med3_i32(a2048[k + 1], N1, N1 + 2047);
        xmax = imax(imax(xmax, X0), X1);
        xmin = imin(imin(xmin, X0), X1);
    }
    return sat_pack16(xmax >> 11, xmin >> 11);
}
VGA_HD void pack_row(const int (&x)[16], uint32_t (&xw)[7])
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 7; i++) xw[i] = pack16(x[2 + 2 * i], x[3 + 2 * i]);
}
// x[0], x[1] = the history, x[2..15] = the frame: the form the literal pass, the sequential pre-scan and the reference's loop
// as written (resume_passes) take -- the rare paths unpack where they run
VGA_HD void unpack_row(const uint32_t (&xw)[7], uint32_t hist, int (&x)[16])
{
    x[0] = pair_lo(hist);
    x[1] = pair_hi(hist);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 7; i++) { x[2 + 2 * i] = pair_lo(xw[i]); x[3 + 2 * i] = pair_hi(xw[i]); }
}

// Fast quantise pass: integer-only, 12 VALU ops per sample (14 with the f32 rounding) instead of the f32/f64 detour.
// With H = (o0, o1) the packed history and C = (c1, c0) the packed coefficients:
//   P      = dot2(H, C, 1024)                                predicted + 1024, one instruction
//   d      = in2048p - P                                     == in*2048 - predicted
//   r      = (int)(float)d                                   the reference's float rounding
//   u      = (r + 2^(k-1) - 1 + (d<0)) >> k                  unclamped nibble  (S2)
//   q      = clamp(u, -8, 7)
//   w      = (P >> 11) + (q << (k-11))                       the reconstruction before its clamp
//   H'     = sat_pack(w_prev, w)                             clamp AND history shift: (o1, recon) in one instruction
//   every second step, H' = (o[s-1], o[s]) being the two newest outputs:
//   E      = pk_sub_sat(xw[(s-1)/2], H')                     both errors, each saturated to int16
//   total  = dot2(E, E, total)                               + e0*e0 + e1*e1, the sum saturated to int32
// Why this is the same arithmetic as the reference's (and as the pass in two 32-bit history registers it replaces):
//  (P1) with |c0| + |c1| <= 32767 the dot product IS o0*c1 + o1*c0 + 1024: its operands are int16, every product is exact
//       in 32 bits and |sum| <= 32768 * 32767 + 1024 < 2^30 -- nothing wraps in the reference's int arithmetic and nothing
//       saturates here.  With larger coefficients the reference may wrap where dot2 saturates: the pass reports
//       exact == false for them (as it always did: S3 needs the same bound) and pass_literal encodes the frame.  No
//       coefficient is negated, so c = -32768 needs no 17th bit.
//  (P2) d: in2048p = in*2048 + 1024, the 1024 in P cancels (mod 2^32).
//  (P3) the reference reconstructs ((predicted + q * 2^k) + 1024) >> 11; q * 2^k is a multiple of 2^11 (k >= 11), so it passes
//       through the floor: (P + q * 2^k) >> 11 = (P >> 11) + (q << (k - 11)).  |P >> 11| <= 2^20 and |q << (k-11)| <= 2^15: no
//       overflow in w.
//  (P4) sat_pack saturates each input to [-32768, 32767]: that is clamp16i, so hi(H') is the reference's clamped sample.
//  (P5) the low half is w_prev saturated AGAIN, from the unclamped value of the step before: clamp16i of the same number, i.e.
//       the previous step's hi(H) -- the history shift o0 = o1 at no cost.  (Step 0: w_prev = x[1], a 16-bit value.)
//  (P6) S2, S3 and the `exact` test below are untouched: they speak about d, u and e, which are the same numbers.
// The error sum in pairs (round 8) -- what `total` means:
//  (E1) step s reconstructs o[s] for the input x[s + 2]; after steps s - 1 and s (s odd) H' holds (o[s-1], o[s]) and the row
//       dword xw[(s-1)/2] holds (x[s+1], x[s+2]): the inputs of exactly these two steps, halves in the same order.
//  (E2) x and o are int16, so e = x - o lies in [-65535, 65535] and need not fit 16 bits; pk_sub_sat saturates each half to
//       [-32768, 32767].  A half that did NOT saturate is e itself.
//  (E3) dot2 with its clamp adds e0*e0 + e1*e1 to the running sum and saturates the result to [.., 2^31 - 1].  Every term is
//       >= 0, so the running sum never decreases and, once saturated, stays at 2^31 - 1.  If no half saturated and the exact
//       sum is below 2^31, `total` IS the exact sum.  If a half saturated, its term is >= 32767^2 > 2^29, and if the sum
//       reached 2^31 it stays there: either way total >= 2^28 AND the exact sum >= 2^28.  Conversely an exact sum below
//       2^28 has no term of 2^28 or more, so no |e| > 16384, nothing saturated: total == exact sum.  Hence
//           exact sum <  2^28  =>  total == exact sum
//           exact sum >= 2^28  =>  total >= 2^28, its value otherwise unspecified.
//       This holds for ANY row and history (it is a statement about fourteen int16 pairs), whatever the overflow.
//  (E4) the kernel's argmin folds every sum from 2^28 on into one 32-bit key and lets 64-bit keys decide only when a channel's
//       best is that large; there, and only there, a lane at or above 2^28 needs its exact sum: the pass again with
//       WIDE_TOTAL (scalar 17-bit errors, 64-bit sum).  A final lane at the cap may have |e| up to 14338 (overflow 3) and,
//       if its sum came from a WIDE pass, up to 65535: all of them are above 2^28 when they matter and go that way.
//  (E5) r.exact == true promises more: `total` is the exact sum whatever its size.  That needs 14 e^2 < 2^31, |e| <= 12385;
//       the bound below ((2 ov + 1) << (k - 11) <= 24766, i.e. |e| <= 12385) is what pass_fast / resume_passes rely on when
//       they hand `total` to a 64-bit comparison without looking at it again.
// The nibbles leave the pass unpacked (r.q): the kernel's helper wave packs the winner's frame (pack_frame).
// The overflow is recovered from the running max/min of u (one max3/min3 per two samples).
// r.exact == false (frame must be redone with pass_literal) when the saturating 32-bit sum of squared
// errors could stop short (S3, E5): with |c0|+|c1| <= 32767 the predictor cannot wrap, and then
// |in - recon| <= (ov + 1/2) * 2^(k-11) + 2 where ov is the pass's max overflow; we require that
// bound to stay <= 12 385 (14 * 12385^2 < 2^31), which also rules out int32 overflow in u.
// in2048p[s] = x[s + 2] * 2048 + 1024 is supplied by the caller (the kernel's helper wave precomputes it per tile), hist
// is the packed history (x[0], x[1]), xw the frame as packed pairs (E1).
// WIDE_TOTAL: the error sum in 64 bits (a multiply and an add with carry per sample instead of one mad) -- exact whatever
// the overflow as long as the predictor cannot wrap (|c0| + |c1| <= 32767: then |d| < 2^30 + 2^26, u cannot leave int32, and
// |in - recon| <= 65535 squares into 32 bits).  For the one case the 32-bit sum cannot serve: a pass at the cap (scale 12 ends
// the reference's loop whatever it overflowed, :170) whose overflow exceeds 3 -- loud noise, clipped waves.
// NO_ROUND (round 5): the pass without the detour through f32 -- r = d instead of r = (int)(float)d, two conversions a
// sample less.  (int)(float)d IS d while |d| < 2^24, and a sample with |d| >= 2^24 shows: its unclamped nibble has
// |u| >= 2^(24-k), so the pass's overflow is at least 2^(13 - scale_power) - 8.  A pass whose overflow stays BELOW that bound
// (pass_no_round_is_exact) therefore never met such a sample -- by induction over the samples it is the exact pass, nibble
// for nibble -- and one that does not must be run again with the conversions.  The kernel takes this form for a frame when
// every lane of the wave quantises at scale 9 or below (70 % of the synthetic set's wave-frames).
// HAVE_P0 (round 9): step 0's P = dot2(hist, C, 1024) handed in by a caller that has formed it already (the kernel's pre-scan
// head takes its first distance from it, head_distance_numer) -- the same value, one dot product a pass less.
// predicted_p1024 is that dot product as the pass writes it.
VGA_HD int predicted_p1024(uint32_t h, uint32_t cpair)
{
    int k1024 = 1024;
    VGA_OPAQUE_S(k1024);
    return dot2_i16(h, cpair, k1024);
}
template <bool WIDE_TOTAL, bool NO_ROUND = false, bool HAVE_P0 = false>
VGA_HD PassOut pass_fast_core_t(const uint32_t (&xw)[7], uint32_t hist, const int (&in2048p)[14], int c0, int c1, int scale_power,
                                int P0 = 0)
{
    PassOut r;
    uint64_t total64 = 0;
    const int k = scale_power + 11;
    const int km11 = scale_power;
    int bias = (1 << (k - 1)) - 1;
    VGA_OPAQUE(bias);
    const uint32_t cpair = pack16(c1, c0);
    int k1024 = 1024;
    VGA_OPAQUE_S(k1024);
    int total = 0;
    int umax = 0, umin = 0;
    int u_prev = 0;
    uint32_t h = hist;                                              // (o0, o1)
    int w_prev = pair_hi(hist);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int s = 0; s < 14; s++) {
        const int P = (HAVE_P0 && s == 0) ? P0 : dot2_i16(h, cpair, k1024);   // predicted + 1024
        const int d = (int)((uint32_t)in2048p[s] - (uint32_t)P);    // == in2048 - predicted
        const int rd = NO_ROUND ? d : round_through_f32(d);
        const int u = (int)((uint32_t)rd + (uint32_t)bias + ((uint32_t)d >> 31)) >> k;
        const int q = imin(imax(u, -8), 7);
        if (s & 1) {
            umax = imax(imax(umax, u_prev), u);
            umin = imin(imin(umin, u_prev), u);
        }
        u_prev = u;
        r.q[s] = q;
        const int w = (P >> 11) + (int)((uint32_t)q << km11);       // off the chain: P >> 11 waits for q
        h = sat_pack16(w_prev, w);                                  // (o1, recon)
        w_prev = w;
        if (WIDE_TOTAL) {
            const int e = ((s & 1) ? pair_hi(xw[s >> 1]) : pair_lo(xw[s >> 1])) - pair_hi(h);      // x[s + 2] - o[s], 17 bits
#if defined(__HIP_DEVICE_COMPILE__)
            total64 += (uint64_t)vga_square24(e);                   // |e| <= 65535: the product's low 32 bits are the square
#else
            total64 += (uint64_t)((int64_t)e * (int64_t)e);
#endif
        } else if (s & 1) {
            const uint32_t epk = pk_sub_sat_i16(xw[s >> 1], h);     // (x[s+1] - o[s-1], x[s+2] - o[s]), saturated (E1, E2)
            total = dot2_i16(epk, epk, total);                      // total += e0*e0 + e1*e1, saturating (E3)
        }
    }
    r.hist_pair = h;                                                // falls out of the last step
    const int ov = imax(imax(umax - 7, -8 - umin), 0);
    const int ac0 = c0 < 0 ? -c0 : c0, ac1 = c1 < 0 ? -c1 : c1;
    r.exact = ac0 + ac1 <= 32767 && (WIDE_TOTAL || (ov <= 12383 && (((2 * ov + 1) << (k - 11)) <= 24766)));
    r.total = WIDE_TOTAL ? total64 : (uint64_t)(uint32_t)total;     // (total >= 0: see E3)
    r.max_overflow = ov;
    r.o12 = pair_lo(h); r.o13 = pair_hi(h);
    return r;
}
VGA_HD PassOut pass_fast_core(const uint32_t (&xw)[7], uint32_t hist, const int (&in2048p)[14], int c0, int c1, int scale_power)
{
    return pass_fast_core_t<false>(xw, hist, in2048p, c0, c1, scale_power);
}
VGA_HD PassOut pass_fast_core_no_round(const uint32_t (&xw)[7], uint32_t hist, const int (&in2048p)[14], int c0, int c1,
                                       int scale_power)
{
    return pass_fast_core_t<false, true>(xw, hist, in2048p, c0, c1, scale_power);
}
// the bound under which a NO_ROUND pass is the exact pass (scale_power <= 12: the bound is positive up to scale 9)
VGA_HD bool pass_no_round_is_exact(int scale_power, int max_overflow)
{
    return scale_power <= 9 && max_overflow < (1 << (13 - scale_power)) - 8;
}
VGA_HD PassOut pass_fast_core_wide(const uint32_t (&xw)[7], uint32_t hist, const int (&in2048p)[14], int c0, int c1,
                                   int scale_power)
{
    return pass_fast_core_t<true>(xw, hist, in2048p, c0, c1, scale_power);
}
// ---- the rounding sign from the subtract's borrow (round 10) --------------------------------
// pass_fast_core_t spends three instructions of the sample step's dependent chain on d = in2048p - P, sign = d >>> 31 and
// t = rd + bias + sign.  pass_fast_core_b runs the same step on numbers moved up by OFF = 2^30: both operands of the subtract are
// then non-negative, its unsigned borrow IS the sign, and an add with carry consumes it (v_sub_co_u32 + v_addc_co_u32: one
// instruction and one link of the chain less per sample step).  With Z = 2^(19 - scale_power) = OFF / 2^k:
//   P'     = dot2(H, C, 1024 + OFF)                          P + OFF; the accumulator constant in a scalar register as before
//   d, b   = usub_overflow(in', P')                          in' = in*2048 + 1024 + OFF (the caller's row); b = borrow
//   t      = rd + (bias - OFF) + b                           rd = d or (int)(float)d as in pass_fast_core_t; one add with carry
//   u2     = t >> k                                          = u - Z
//   q2     = med3(u2, -8 - Z, 7 - Z)                         = q - Z
//   w      = (P' >> 11) + (q2 << scale_power)                the true w
//   H', E, total                                             as in pass_fast_core_t
// The overflow comes from the running max / min of u2 against the shifted bounds; they start at -Z, the old 0.
//  (B1) |c0| + |c1| <= 30720: |predicted| <= 32768 * 30720 = 2^30 - 2^26, so P' = predicted + 1024 + 2^30 lies in
//       [2^26 + 1024, 2^31 - 2^26 + 1024], inside [0, 2^31): the dot product's clamp cannot fire (P1 carries over) and P' is
//       non-negative as an unsigned AND as a signed number.  in' = in * 2048 + 1024 + 2^30 lies in
//       [2^30 - 2^26 + 1024, 2^30 + 2^26 - 1024], inside [0, 2^31) as well.
//  (B2) both operands of in' - P' are non-negative and below 2^31: the difference is the true d = in * 2048 - predicted (the
//       1024 + OFF cancels, P2) without wrapping, and the unsigned subtract borrows exactly when in' < P', i.e. when d < 0.
//  (B3) t does not leave int32.  d >= -2^26 - (2^30 - 2^26) = -2^30, which f32 represents, so rd >= -2^30 (rounding is monotone)
//       and t >= -2^30 + bias - 2^30 >= -2^31 + 1023; upwards t < 2^30 + 2^26 + 2^22 - 2^30.  THIS is what sets the bound at 30720
//       = 32768 - 2048 and not at 32767: there d could reach -2^30 - 2^26 + 32768 and t would wrap below -2^31 at small scales.
//  (B4) OFF = Z * 2^k exactly (k <= 23 < 30), and an arithmetic shift commutes with subtracting a multiple of 2^k:
//       u2 = (rd + bias + b - Z * 2^k) >> k = u - Z.  Clamping u - Z to [-8 - Z, 7 - Z] gives q - Z; max / min likewise, so
//       max(umax2 - (7 - Z), (-8 - Z) - umin2, 0) is the old overflow.  Z is a multiple of 128 (scale_power <= 12): q2 & 15 == q & 15.
//  (B5) w: P' >> 11 = (P >> 11) + 2^19 (OFF is a multiple of 2^11) and q2 << scale_power = (q << scale_power) - 2^19: the two
//       cancel, w is pass_fast_core_t's w bit for bit.  Hence H, the errors and everything S2 / S3 / E1-E5 / NO_ROUND say speak
//       about the same numbers.
// The nibbles leave the pass as q2 (PassOutB::q2); whoever packs them takes them & 15 (pack_frame_mod16) or adds Z.
// Coefficients with |c0| + |c1| > 30720 get exact == false: the callers send them the way coefficients that can wrap go (the
// reference's loop as written, exact for any coefficients).  Real coefficient sets have |c0| + |c1| of a few thousand.
// pass_fast_core_t stays for the seam, tail and chain code and for the WIDE pass (bound 32767).
constexpr int PASS_B_OFF = 1 << 30;
constexpr int PASS_B_COEF_SUM_MAX = 30720;                             // B3
struct PassOutB {
    int q2[14];          // q - Z, Z = pass_b_z(scale_power); congruent to the nibble mod 16
    uint64_t total;
    int max_overflow;
    unsigned hist_pair;
    bool exact;          // as PassOut::exact, with the bound of B3 on the coefficients
    uint32_t pairs[7];   // WITH_SUM == false only: the seven history pairs (o[2i], o[2i + 1]) the error sum is formed from (E1)
};
VGA_HD bool pass_b_coef_ok(int c0, int c1)
{
    return (c0 < 0 ? -c0 : c0) + (c1 < 0 ? -c1 : c1) <= PASS_B_COEF_SUM_MAX;
}
VGA_HD int pass_b_z(int scale_power) { return 1 << (19 - scale_power); }
VGA_HD int pass_b_row(int in) { return in * 2048 + 1024 + PASS_B_OFF; }      // in' (the kernel's helper wave writes it per tile)
// P' of a history pair: the dot product as the pass writes it
VGA_HD int predicted_b(uint32_t h, uint32_t cpair)
{
    int kacc = 1024 + PASS_B_OFF;
    VGA_OPAQUE_S(kacc);
    return dot2_i16(h, cpair, kacc);
}
// head_distance_numer on the moved numbers: N = in' - P' is the same N, and 1024 + OFF - P' = 1024 - P without wrapping (B1)
VGA_HD int head_distance_numer_b(int in_b, int P_b)
{
    const int N = (int)((uint32_t)in_b - (uint32_t)P_b);
    return numer_adjust(N, (int)((uint32_t)(1024 + PASS_B_OFF - P_b) >> 31)) >> 11;
}
// median of three signed values (v_med3_i32): with lo <= hi, clamp(v, lo, hi).  hipcc makes v_max + v_min of a clamp whose
// bounds are registers; the asm statement's operands here come from a shift and registers that are set once per pass, never
// straight from a dot product, so no wait states are missing behind it (see dot2_i16_wrap).
VGA_HD int med3_i32(int v, int lo, int hi)
{
#if defined(__HIP_DEVICE_COMPILE__)
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(v), "v"(lo), "v"(hi));
    return r;
#else
    return imin(imax(v, lo), hi);
#endif
}
// d = a - b (mod 2^32) and the unsigned borrow; t = x + y + carry (mod 2^32).  The device build leaves both to hipcc
// (v_sub_co_u32 / v_addc_co_u32 from these very expressions); the host build computes the same.
VGA_HD uint32_t sub_borrow_u32(uint32_t a, uint32_t b, uint32_t &borrow)
{
    uint32_t d;
    borrow = __builtin_usub_overflow(a, b, &d) ? 1u : 0u;
    return d;
}
// WITH_SUM == false (round 10, step 2): the pass returns its seven history pairs and total = 0; a caller that runs two passes
// in one lane picks the pairs of the pass the reference ends on and forms ONE sum from them (error_sum_pairs) -- E1-E5 are
// statements about the pairs and hold for the sum formed there.
VGA_HD uint32_t error_sum_pairs(const uint32_t (&xw)[7], const uint32_t (&pairs)[7])
{
    int total = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 7; i++) {
        const uint32_t epk = pk_sub_sat_i16(xw[i], pairs[i]);       // (E1, E2)
        total = dot2_i16(epk, epk, total);                          // (E3)
    }
    return (uint32_t)total;
}
// OV_ONLY (round 11): the pass for its overflow alone -- neither the nibbles nor the history pairs become outputs (q2, pairs,
// total are left unset); see final_pass_pair.
template <bool NO_ROUND, bool HAVE_P0 = false, bool WITH_SUM = true, bool OV_ONLY = false>
VGA_HD PassOutB pass_fast_core_b(const uint32_t (&xw)[7], uint32_t hist, const int (&in_b)[14], int c0, int c1, int scale_power,
                                 int P0_b = 0)
{
    PassOutB r;
    const int k = scale_power + 11;
    const int km11 = scale_power;
    int bias2 = (1 << (k - 1)) - 1 - PASS_B_OFF;
    VGA_OPAQUE(bias2);
    const int nz = -(1 << 19) >> scale_power;                       // -Z in one shift
    const int q_lo = nz - 8, q_hi = nz + 7;
    const uint32_t cpair = pack16(c1, c0);
    int kacc = 1024 + PASS_B_OFF;
    VGA_OPAQUE_S(kacc);
    int total = 0;
    int umax = nz, umin = nz;
    int u_prev = nz;
    uint32_t h = hist;                                              // (o0, o1)
    int w_prev = pair_hi(hist);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int s = 0; s < 14; s++) {
        const int P = (HAVE_P0 && s == 0) ? P0_b : dot2_i16(h, cpair, kacc);  // predicted + 1024 + OFF
        uint32_t b;
        const int d = (int)sub_borrow_u32((uint32_t)in_b[s], (uint32_t)P, b);  // the true distance; b = (d < 0)  (B2)
        const int rd = NO_ROUND ? d : round_through_f32(d);
        const int u2 = (int)((uint32_t)rd + (uint32_t)bias2 + b) >> k;       // u - Z  (B3, B4)
        const int q2 = med3_i32(u2, q_lo, q_hi);
        if (s & 1) {
            umax = imax(imax(umax, u_prev), u2);
            umin = imin(imin(umin, u_prev), u2);
        }
        u_prev = u2;
        if (!OV_ONLY) r.q2[s] = q2;
        const int w = (P >> 11) + (int)((uint32_t)q2 << km11);      // (B5)
        h = sat_pack16(w_prev, w);
        w_prev = w;
        if ((s & 1) && !OV_ONLY) {
            if (WITH_SUM) {
                const uint32_t epk = pk_sub_sat_i16(xw[s >> 1], h);
                total = dot2_i16(epk, epk, total);
            } else
                r.pairs[s >> 1] = h;
        }
    }
    r.hist_pair = h;
    const int ov = imax(imax(umax - q_hi, q_lo - umin), 0);
    r.exact = pass_b_coef_ok(c0, c1) && ov <= 12383 && (((2 * ov + 1) << (k - 11)) <= 24766);
    r.total = (uint64_t)(uint32_t)total;
    r.max_overflow = ov;
    return r;
}
// ---- one lane, both trips: the pass at s1 for its overflow, then ONE final pass (round 11) -------------------------------
// A lane of the (channel, predictor) layout ran the pass at sp_b = s1 + 1 and the pass at sp_a = s1, kept the nibbles and the
// history pairs of both and picked one set with 21 selects.  Nothing needs both sets: the overflow of the pass at s1 alone
// says whether the reference's loop stops there (pass_a_is_final).  So the first pass runs for its overflow only (OV_ONLY) and
// the second at the lane's own scale sp2 = fin_a ? sp_a : sp_b:
//  (T1) fin_a: the second pass IS the pass at sp_a again -- same row, history, coefficients and scale, hence the same nibbles,
//       pairs and overflow (ov_2 == ov_a).
//  (T2) otherwise it is the pass at sp_b, ov_2 == ov_b.
// Either way its q2, pairs and hist_pair are what the selects delivered.  Every flag below reads ov_b only for a lane that is
// not fin_a (frame_flags: bump_b and resume carry !fin_a, inexact reads the side fin_a names), so ov_2 stands in for ov_b.
// A NO_ROUND pair vouches for itself when the pass at sp_a and the pass at sp2 both do (pass_no_round_is_exact): an exact
// first pass has the true ov_a, hence the true fin_a and sp2.
VGA_HD bool pass_a_is_final(int sp_a, int ov_a) { return sp_a >= 12 || ov_a <= 1; }
template <bool NO_ROUND>
VGA_HD PassOutB final_pass_pair(const uint32_t (&xw)[7], uint32_t hist, const int (&in_b)[14], int c0, int c1, int sp_a, int sp_b,
                                int P0_b, int &ov_a, int &sp2)
{
    ov_a = pass_fast_core_b<NO_ROUND, true, false, true>(xw, hist, in_b, c0, c1, sp_a, P0_b).max_overflow;
    sp2 = pass_a_is_final(sp_a, ov_a) ? sp_a : sp_b;
    return pass_fast_core_b<NO_ROUND, true, false>(xw, hist, in_b, c0, c1, sp2, P0_b);
}
// What can stand between the two passes and the frame's result, per lane (round 5; sp_a = min(s1, 12), sp_b = min(s1 + 1, 12)):
//   * bump_a / bump_b: the pass the loop has reached overflowed by more than 248, the bump loop (:166-168) moves the scale by
//     more than one step -- the reference's loop as written, from the scale it moves to;
//   * hostile coefficients (!coef_ok): the whole loop as written;      (generic = any of these)
//   * inexact: the final pass ran at the cap and overflowed by more than 3: its lane's sum goes by the exact-sum rule (E4);
//   * resume: both passes overflowed, on to s1 + 2.
// A pass at the cap ends the loop whatever it overflowed.  ov_b may be ov_2 of final_pass_pair (T1, T2).
struct FrameFlags { bool fin_a, bump_a, bump_b, generic, inexact, resume; };
VGA_HD FrameFlags frame_flags(int sp_a, int sp_b, int ov_a, int ov_b, bool coef_ok)
{
    FrameFlags f;
    const bool cap_a = sp_a >= 12, cap_b = sp_b >= 12;
    const int eff_a = cap_a ? 0 : ov_a, eff_b = cap_b ? 0 : ov_b;
    f.fin_a = eff_a < 2;
    f.bump_a = !cap_a && (unsigned)ov_a > 248u;
    f.bump_b = !f.fin_a && !cap_b && (unsigned)ov_b > 248u;
    f.generic = !coef_ok || f.bump_a || f.bump_b;
    f.inexact = !f.generic && (f.fin_a ? (cap_a && (unsigned)ov_a > 3u) : (cap_b && (unsigned)ov_b > 3u));
    f.resume = !f.generic && !f.fin_a && eff_b >= 2;
    return f;
}
// "Does the lane go to the cold block", and fin_a, as four compares and lane-mask logic -- no select, no branch (round 12;
// measured in round 11, LABNOTES 16.3).  thr = 1 below the cap, 3 at it: what a pass may overflow by and still end the loop
// with a sum the 32-bit key can trust.  With a_bad = ov_a > thr(sp_a), b_bad = ov_2 > thr(sp_b):
//   * cap_a: the pass at sp_a ends the loop; the lane is cold exactly when a_bad (inexact).
//   * !cap_a, !a_bad: fin_a, hot.
//   * !cap_a, a_bad: not fin_a, ov_2 is pass B's; cold when ov_a > 248 (bump_a) or b_bad -- below the cap that is resume or
//     bump_b, at it inexact.
// Hence cold = !coef_ok | (a_bad & (cap_a | ov_a > 248 | b_bad)), and cold == generic || resume || inexact of frame_flags
// (tests/test_host_gc_flag_masks.py, by enumeration).  The frame code branches on the ballot of `cold` and asks frame_flags
// for the single flags inside the cold branch only.
VGA_HD int frame_flag_limit(int sp) { return sp >= 12 ? 3 : 1; }
struct FrameCold { bool cold, fin_a; };
VGA_HD FrameCold frame_goes_cold(int sp_a, int sp_b, int ov_a, int ov_2, bool coef_ok)
{
    const bool cap_a = sp_a >= 12;
    const bool a_bad = ov_a > frame_flag_limit(sp_a), b_bad = ov_2 > frame_flag_limit(sp_b);
    FrameCold f;
    f.fin_a = cap_a | !a_bad;
    f.cold = !coef_ok | (a_bad & (cap_a | (ov_a > 248) | b_bad));
    return f;
}
// The 8 frame bytes (pack_frame) from nibbles known mod 16 only: q, q2 = q - Z, or the biased nibble all pack alike.
VGA_HD void pack_frame_mod16(const int (&q)[14], int predictor, int scale_power, uint32_t &d0, uint32_t &d1)
{
    uint32_t wa = 0, wb = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int s = 0; s < 14; s++) {
        if (s < 6) wa = (wa << 4) | ((uint32_t)q[s] & 15u);
        else       wb = (wb << 4) | ((uint32_t)q[s] & 15u);
    }
    const uint32_t header = (uint32_t)((predictor << 4) | (scale_power & 0xF));
    d0 = bswap32((header << 24) | wa);
    d1 = bswap32(wb);
}
// a PassOut (nibbles as they are) in the form the kernel's frame tail takes
VGA_HD PassOutB as_pass_b(const PassOut &r)
{
    PassOutB o;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int s = 0; s < 14; s++) o.q2[s] = r.q[s];
    o.total = r.total; o.max_overflow = r.max_overflow; o.hist_pair = r.hist_pair; o.exact = r.exact;
    return o;
}
// The exact-sum rule (E4) for one lane: a sum at or above 2^28 that is not known to be exact (r.exact) is taken again from
// the pass with the 64-bit sum, at the scale the pass ran at.  The kernel's cold block applies it when a channel's best key
// saturated; for coefficients that can wrap the wide pass is no authority and the caller has the literal pass's sum.
constexpr uint64_t PACKED_SUM_CAP = 1ull << 28;
VGA_HD bool needs_exact_sum(uint64_t total, bool known_exact) { return !known_exact && total >= PACKED_SUM_CAP; }
// The same three for callers that hold the frame as sixteen ints, x[0], x[1] the history (the lane emulators of the CPU
// tests): the row is packed here, the pass is the one above.
VGA_HD PassOut pass_fast_core(const int (&x)[16], uint32_t hist, const int (&in2048p)[14], int c0, int c1, int scale_power)
{
    uint32_t xw[7];
    pack_row(x, xw);
    return pass_fast_core_t<false>(xw, hist, in2048p, c0, c1, scale_power);
}
VGA_HD PassOut pass_fast_core_no_round(const int (&x)[16], uint32_t hist, const int (&in2048p)[14], int c0, int c1,
                                       int scale_power)
{
    uint32_t xw[7];
    pack_row(x, xw);
    return pass_fast_core_t<false, true>(xw, hist, in2048p, c0, c1, scale_power);
}
VGA_HD PassOut pass_fast_core_wide(const int (&x)[16], uint32_t hist, const int (&in2048p)[14], int c0, int c1,
                                   int scale_power)
{
    uint32_t xw[7];
    pack_row(x, xw);
    return pass_fast_core_t<true>(xw, hist, in2048p, c0, c1, scale_power);
}
// ... and with the row of x * 2048 the pass read until round 7 (the pass does not look at it).  These hand `total` straight
// to 64-bit comparisons, as the kernel did until round 8: they apply the exact-sum rule themselves.
template <bool NO_ROUND>
VGA_HD PassOut pass_fast_core_exact_sum(const int (&x)[16], const int (&in2048p)[14], int c0, int c1, int scale_power)
{
    uint32_t xw[7];
    pack_row(x, xw);
    const uint32_t hist = pack16(x[0], x[1]);
    PassOut r = pass_fast_core_t<false, NO_ROUND>(xw, hist, in2048p, c0, c1, scale_power);
    const int ac0 = c0 < 0 ? -c0 : c0, ac1 = c1 < 0 ? -c1 : c1;
    if (ac0 + ac1 <= 32767 && needs_exact_sum(r.total, r.exact))
        r.total = pass_fast_core_t<true>(xw, hist, in2048p, c0, c1, scale_power).total;
    return r;
}
VGA_HD PassOut pass_fast_core(const int (&x)[16], const int (&)[14], const int (&in2048p)[14], int c0, int c1, int scale_power)
{
    return pass_fast_core_exact_sum<false>(x, in2048p, c0, c1, scale_power);
}
VGA_HD PassOut pass_fast_core_no_round(const int (&x)[16], const int (&)[14], const int (&in2048p)[14], int c0, int c1,
                                       int scale_power)
{
    return pass_fast_core_exact_sum<true>(x, in2048p, c0, c1, scale_power);
}
VGA_HD PassOut pass_fast_core_wide(const int (&x)[16], const int (&)[14], const int (&in2048p)[14], int c0, int c1,
                                   int scale_power)
{
    return pass_fast_core_wide(x, pack16(x[0], x[1]), in2048p, c0, c1, scale_power);
}

VGA_HD PassOut pass_fast(const int (&x)[16], int c0, int c1, int scale_power)
{
    int in2048p[14];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int s = 0; s < 14; s++) in2048p[s] = x[s + 2] * 2048 + 1024;
    return pass_fast_core(x, pack16(x[0], x[1]), in2048p, c0, c1, scale_power);
}

// ---- speculative two-candidate resolution --------------------------------------------
// Lane A ran the pass at s1, lane B at s1+1 (the scale the reference tries next when A
// overflows without a bump).  From the two overflows alone every lane can tell which of
// the two passes (if any) is the one the reference's do-loop ends on.
struct Resolve {
    bool final_a;        // the reference stops after the pass at s1
    bool final_b;        // ... after the pass at s1+1
    int resume_sp;       // otherwise: value of scalePower when the do-loop is re-entered
};

VGA_HD Resolve resolve_candidates(int s1, int ov_a, int ov_b)
{
    Resolve z;
    z.final_a = z.final_b = false;
    z.resume_sp = 0;
    const int sp_a = apply_bumps(s1, ov_a);
    if (!(sp_a < 12 && ov_a > 1)) { z.final_a = true; return z; }
    if (sp_a != s1) { z.resume_sp = sp_a; return z; }        // bumped: next pass is not s1+1
    const int s2 = s1 + 1;
    const int sp_b = apply_bumps(s2, ov_b);
    if (!(sp_b < 12 && ov_b > 1)) { z.final_b = true; return z; }
    z.resume_sp = sp_b;
    return z;
}

// Same decision when neither overflow can trigger the bump loop (max_overflow + 8 <= 256):
// straight-line, no loops -- the kernel's common path.
VGA_HD Resolve resolve_candidates_nobump(int s1, int ov_a, int ov_b)
{
    Resolve z;
    z.final_a = !(s1 < 12 && ov_a > 1);
    z.final_b = !z.final_a && !(s1 + 1 < 12 && ov_b > 1);
    z.resume_sp = s1 + 1;
    return z;
}

// Continue the reference's do-loop from `scale_power` (value before the ++), precomputed in*2048 + 1024 array.
VGA_HD PassOut resume_passes_core(const int (&x)[16], const int (&in2048p)[14], int c0, int c1, int scale_power,
                                  int &final_sp)
{
    PassOut r;
    bool at_max;
    do {
        scale_power++;
        at_max = scale_power >= 12;
        r = pass_fast_core(x, pack16(x[0], x[1]), in2048p, c0, c1, scale_power);
        if (!r.exact) r = pass_literal(x, c0, c1, scale_power);
        scale_power = apply_bumps(scale_power, r.max_overflow);
    } while (scale_power < 12 && r.max_overflow > 1 && !at_max);
    final_sp = scale_power;     // the reference's `out scalePower` (== the pass scale on a regular exit)
    return r;
}

// Continue the reference's do-loop from `scale_power` (value before the ++).
// Includes the termination guard documented in gcadpcm_kernels.hip / oracle.
VGA_HD PassOut resume_passes(const int (&x)[16], int c0, int c1, int scale_power, int &final_sp)
{
    PassOut r;
    bool at_max;
    do {
        scale_power++;
        at_max = scale_power >= 12;
        r = pass_fast(x, c0, c1, scale_power);
        if (!r.exact) r = pass_literal(x, c0, c1, scale_power);
        scale_power = apply_bumps(scale_power, r.max_overflow);
    } while (scale_power < 12 && r.max_overflow > 1 && !at_max);
    final_sp = scale_power;     // the reference's `out scalePower` (== the pass scale on a regular exit)
    return r;
}

}  // namespace gc
}  // namespace vga
