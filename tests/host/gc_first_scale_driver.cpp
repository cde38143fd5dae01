// gc_first_scale_driver.cpp -- host driver for the GC-ADPCM encoder's first-scale work (round 9, gc_encode_core.hpp F1-F4 and
// N1-N2): the first scale from the frame's range against the round-1 form it replaces, and the encoder wave's two head
// distances in the numerator domain (no quotient) next to the helper wave's range against the literal pre-scan.
// TEST ONLY, compiled by tests/test_host_gc_first_scale.py from the SAME header the kernel uses.
#include "../../vgaudio_amd/csrc/gc_encode_core.hpp"

using namespace vga::gc;

namespace {

// first_scale_power_from_range as it stood from round 1 to round 8: the reference copy
int first_scale_power_from_range_r1(int dmax, int dmin)
{
    const int pos = imax(clamp16i(dmax), 0);
    const int neg = imax(-clamp16i(dmin), 0);
    const int hp = imax(bit_length((unsigned)pos | 1u) - 3, 0);
    const int nn = imax(bit_length((unsigned)neg | 1u) - 4, 0);
    const int hn = nn + ((((unsigned)neg >> nn) > 8u) ? 1 : 0);
    if (pos == neg && hp != hn) return -100;
    const int n = pos > neg ? hp : hn;
    return imax(n - 1, 0);
}

// the helper wave's pairs of a frame (gc_encode_kernel.hip, prepare): even k the dword as loaded, odd k one v_alignbit
void frame_pairs(const int (&x)[16], uint32_t (&pair)[12])
{
    uint32_t w[7];
    pack_row(x, w);
    for (int k = 0; k < 12; k++)
        pair[k] = (k & 1) ? ((w[(k - 1) / 2] >> 16) | (w[(k + 1) / 2] << 16)) : w[k / 2];
}

bool coef_ok(int c0, int c1) { return (c0 < 0 ? -c0 : c0) + (c1 < 0 ? -c1 : c1) <= 32767; }

// dmax / dmin of the frame as the kernel forms them: the helper's packed range of s = 2..13 (pairs, the unchecked sum, the
// quotient) and the encoder wave's two head distances -- in the numerator domain from P = predicted + 1024 (`numer`, what a wave
// without hostile lanes takes), or with the unchecked sum and the quotient
void kernel_range(const int (&x)[16], int c0, int c1, bool numer, uint32_t &pre, int &d0, int &d1)
{
    uint32_t pair[12];
    frame_pairs(x, pair);
    const uint32_t cpk = pack16(c1, c0), hpk = pack16(x[0], x[1]);
    const uint32_t h1 = pack16(x[1], x[2]);                           // alignbit(xw[0], hpk, 16)
    int dmax = 0, dmin = 0;
    for (int k = 0; k < 12; k++) {
        const int d = x[k + 4] - div2048(dot2_i16_wrap(pair[k], cpk));
        dmax = imax(dmax, d);
        dmin = imin(dmin, d);
    }
    pre = (uint32_t)(clamp16i(dmax) & 0xFFFF) | ((uint32_t)clamp16i(dmin) << 16);
    if (numer) {
        d0 = head_distance_numer(x[2] * 2048 + 1024, predicted_p1024(hpk, cpk));
        d1 = head_distance_numer(x[3] * 2048 + 1024, predicted_p1024(h1, cpk));
    } else {
        d0 = x[2] - div2048(dot2_i16_wrap(hpk, cpk));
        d1 = x[3] - div2048(dot2_i16_wrap(h1, cpk));
    }
}

}  // namespace

extern "C" {

// (i) every pair dmax in [dmax_begin, dmax_end) x dmin in [-32768, 0]: the new form against the reference copy.
// counts: [0] pairs  [1] pairs answered -100.  Returns 0, or 1 and the first differing pair in bad[0..1].
int fs_check_first_scale(int dmax_begin, int dmax_end, long long *counts, int *bad)
{
    long long n = 0, ties = 0;
    for (int dmax = dmax_begin; dmax < dmax_end; dmax++)
        for (int dmin = -32768; dmin <= 0; dmin++) {
            const int want = first_scale_power_from_range_r1(dmax, dmin);
            const int got = first_scale_power_from_range(dmax, dmin);
            if (want != got) { bad[0] = dmax; bad[1] = dmin; return 1; }
            n++;
            ties += want == -100;
        }
    counts[0] += n;
    counts[1] += ties;
    return 0;
}
// the same for given pairs (values beyond 16 bits, as the kernel's unclamped head distances can be)
int fs_check_first_scale_pairs(const int *dmax, const int *dmin, int n)
{
    for (int i = 0; i < n; i++)
        if (first_scale_power_from_range_r1(dmax[i], dmin[i]) != first_scale_power_from_range(dmax[i], dmin[i])) return i;
    return -1;
}

// (ii) n frames of 16 samples (x[0], x[1] the history), coefficients with |c0| + |c1| <= 32767: the two head distances of the
// numerator domain (head_distance_numer, predicted_p1024: the code under test) against prescan_range over s = 0 and s = 1.
// The range of s = 2..13 beside them is kernel_range's own copy of the helper wave's loop, which this round does not change;
// holding it to prescan_range(x, c0, c1, 2, 14) and clamp16 only keeps that copy honest for (iii).
// counts: [0] frames whose D is 0 somewhere  [1] frames with a numerator on a multiple of 2048  [2] frames with a clamped half
// Returns the index of the first differing frame, -1 if none; -2 if a coefficient pair can wrap.
int fs_check_numer(const int16_t *x16, const int *c0, const int *c1, int n, long long *counts)
{
    for (int i = 0; i < n; i++) {
        if (!coef_ok(c0[i], c1[i])) return -2;
        int x[16];
        for (int k = 0; k < 16; k++) x[k] = x16[(long long)i * 16 + k];
        uint32_t pre;
        int d0, d1;
        kernel_range(x, c0[i], c1[i], true, pre, d0, d1);
        int dmax = 0, dmin = 0;
        prescan_range(x, c0[i], c1[i], 2, 14, dmax, dmin);
        const uint32_t want = (uint32_t)(clamp16i(dmax) & 0xFFFF) | ((uint32_t)clamp16i(dmin) << 16);
        int a = 0, b = 0, w0, w1;
        prescan_range(x, c0[i], c1[i], 0, 1, a, b);
        w0 = a + b;                                                   // (one of the two stayed 0)
        a = b = 0;
        prescan_range(x, c0[i], c1[i], 1, 2, a, b);
        w1 = a + b;
        if (pre != want || d0 != w0 || d1 != w1) return i;
        bool zero = false, mult = false;
        for (int s = 0; s < 14; s++) {
            const int D = x[s] * c1[i] + x[s + 1] * c0[i];
            zero = zero || D == 0;
            mult = mult || ((x[s + 2] * 2048 - D) & 2047) == 0;
        }
        counts[0] += zero;
        counts[1] += mult;
        counts[2] += clamp16i(dmax) != dmax || clamp16i(dmin) != dmin;
    }
    return -1;
}

// (iii) the whole pre-scan as the kernel runs it -- range, first scale, the sequential pre-scan on a tie -- against the literal
// sequential pre-scan, for any coefficients: numer = 0 the head that keeps the unchecked sum and the quotient (what a wave
// with a wrapping lane takes), numer = 1 the numerator domain (coefficients that cannot wrap only).
// counts: [0] frames whose predictor sum wrapped int32  [1] ties.  Returns the first differing frame, -1 if none.
int fs_check_prescan(const int16_t *x16, const int *c0, const int *c1, int n, int numer, long long *counts)
{
    for (int i = 0; i < n; i++) {
        if (numer && !coef_ok(c0[i], c1[i])) return -2;
        int x[16];
        for (int k = 0; k < 16; k++) x[k] = x16[(long long)i * 16 + k];
        uint32_t pre;
        int d0, d1;
        kernel_range(x, c0[i], c1[i], numer != 0, pre, d0, d1);
        const int dmax = imax(imax((int)(int16_t)(pre & 0xFFFF), d0), d1);
        const int dmin = imin(imin((int)pre >> 16, d0), d1);
        int sum, pos;
        int s1 = first_scale_power_nt(dmax, dmin, sum, pos);          // as the kernel's first_scale lambda
        if (sum == 0 && first_scale_tie(pos)) { s1 = first_scale_power_from_md(prescan_sequential(x, c0[i], c1[i])); counts[1]++; }
        if (s1 != first_scale_power_from_md(prescan_sequential(x, c0[i], c1[i]))) return i;
        for (int s = 0; s < 14; s++) {
            const long long D = (long long)x[s] * c1[i] + (long long)x[s + 1] * c0[i];
            if (D != (long long)(int)D) { counts[0]++; break; }
        }
    }
    return -1;
}

// The fast pass with step 0's dot product handed in (HAVE_P0, what the kernel's frame does since round 9) against the pass that
// forms it itself, with and without the f32 detour: every field.  Returns the first differing frame, -1 if none.
int fs_check_pass_p0(const int16_t *x16, const int *c0, const int *c1, const int *sp, int n)
{
    for (int i = 0; i < n; i++) {
        int x[16], mp[14];
        for (int k = 0; k < 16; k++) x[k] = x16[(long long)i * 16 + k];
        for (int s = 0; s < 14; s++) mp[s] = x[s + 2] * 2048 + 1024;
        uint32_t xw[7];
        pack_row(x, xw);
        const uint32_t hist = pack16(x[0], x[1]);
        const int P0 = predicted_p1024(hist, pack16(c1[i], c0[i]));
        for (int nr = 0; nr < 2; nr++) {
            const PassOut a = nr ? pass_fast_core_t<false, true, false>(xw, hist, mp, c0[i], c1[i], sp[i])
                                 : pass_fast_core_t<false, false, false>(xw, hist, mp, c0[i], c1[i], sp[i]);
            const PassOut b = nr ? pass_fast_core_t<false, true, true>(xw, hist, mp, c0[i], c1[i], sp[i], P0)
                                 : pass_fast_core_t<false, false, true>(xw, hist, mp, c0[i], c1[i], sp[i], P0);
            bool same = a.total == b.total && a.max_overflow == b.max_overflow && a.hist_pair == b.hist_pair && a.exact == b.exact &&
                        a.o12 == b.o12 && a.o13 == b.o13;
            for (int s = 0; s < 14; s++) same = same && a.q[s] == b.q[s];
            if (!same) return i;
        }
    }
    return -1;
}

}  // extern "C"
