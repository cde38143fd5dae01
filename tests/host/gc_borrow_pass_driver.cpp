// gc_borrow_pass_driver.cpp -- host driver for the quantise pass that takes its rounding sign from the subtract's borrow
// (gc_encode_core.hpp: pass_fast_core_b, B1-B5) against the pass it stands beside (pass_fast_core_t).  TEST ONLY, compiled by
// tests/test_host_gc_borrow_pass.py from the SAME header the kernel uses; the host build of the header spells out the borrow,
// the add with carry and the median, so this runs the kernel's formulation.
#include "../../vgaudio_amd/csrc/gc_encode_core.hpp"

using namespace vga::gc;

namespace {

// returns 0 = |c0| + |c1| <= 30720 and the new pass equals the old one field for field (whether or not either vouches),
//         1 = within the bound and they DIFFER, 2 = beyond the bound and the new pass says exact == false,
//         3 = beyond the bound and it vouches all the same
int compare_one(const int16_t *x16, int c0, int c1, int sp, int no_round)
{
    int x[16], mp[14], mb[14];
    uint32_t xw[7];
    for (int i = 0; i < 16; i++) x[i] = x16[i];
    for (int s = 0; s < 14; s++) { mp[s] = x[s + 2] * 2048 + 1024; mb[s] = pass_b_row(x[s + 2]); }
    pack_row(x, xw);
    const uint32_t hist = pack16(x[0], x[1]);
    const PassOutB n = no_round ? pass_fast_core_b<true>(xw, hist, mb, c0, c1, sp) : pass_fast_core_b<false>(xw, hist, mb, c0, c1, sp);
    if (!pass_b_coef_ok(c0, c1)) return n.exact ? 3 : 2;
    const PassOut o = no_round ? pass_fast_core_t<false, true>(xw, hist, mp, c0, c1, sp) : pass_fast_core_t<false, false>(xw, hist, mp, c0, c1, sp);
    const int z = pass_b_z(sp);
    bool same = n.total == o.total && n.max_overflow == o.max_overflow && n.hist_pair == o.hist_pair && n.exact == o.exact;
    for (int s = 0; s < 14; s++) same = same && (n.q2[s] & 15) == (o.q[s] & 15) && n.q2[s] + z == o.q[s];
    // the record's two conventions pack alike, and as pack_frame packs the old pass's nibbles
    uint32_t a0, a1, b0, b1;
    pack_frame(o.q, 5, sp, a0, a1);
    pack_frame_mod16(n.q2, 5, sp, b0, b1);
    same = same && a0 == b0 && a1 == b1;
    pack_frame_mod16(o.q, 5, sp, b0, b1);
    same = same && a0 == b0 && a1 == b1;
    // the step-0 dot product handed in (HAVE_P0) is the one the pass forms
    const PassOutB h = no_round ? pass_fast_core_b<true, true>(xw, hist, mb, c0, c1, sp, predicted_b(hist, pack16(c1, c0)))
                                : pass_fast_core_b<false, true>(xw, hist, mb, c0, c1, sp, predicted_b(hist, pack16(c1, c0)));
    same = same && h.total == n.total && h.hist_pair == n.hist_pair && h.max_overflow == n.max_overflow;
    for (int s = 0; s < 14; s++) same = same && h.q2[s] == n.q2[s];
    // the pass that hands over its seven history pairs instead of the sum: one error block over them gives the same sum
    const PassOutB p = no_round ? pass_fast_core_b<true, false, false>(xw, hist, mb, c0, c1, sp)
                                : pass_fast_core_b<false, false, false>(xw, hist, mb, c0, c1, sp);
    same = same && error_sum_pairs(xw, p.pairs) == n.total && p.pairs[6] == n.hist_pair && p.hist_pair == n.hist_pair &&
           p.max_overflow == n.max_overflow && p.exact == n.exact;
    for (int s = 0; s < 14; s++) same = same && p.q2[s] == n.q2[s];
    return same ? 0 : 1;
}

}  // namespace

extern "C" {

int bp_compare(const int16_t *x16, int c0, int c1, int sp, int no_round) { return compare_one(x16, c0, c1, sp, no_round); }

// n frames of 16 samples each; counts[rc]++ per frame; returns the index of the first frame with rc 1 or 3, -1 if none
int bp_compare_many(const int16_t *x16, const int *c0, const int *c1, const int *sp, int n, int no_round, long long *counts)
{
    int first = -1;
    for (int i = 0; i < n; i++) {
        const int rc = compare_one(x16 + (long long)i * 16, c0[i], c1[i], sp[i], no_round);
        counts[rc]++;
        if ((rc == 1 || rc == 3) && first < 0) first = i;
    }
    return first;
}

// B1-B3 in 64-bit arithmetic along the OLD pass's trajectory: out[0] = min t, out[1] = max t, out[2] = min(P', in'),
// out[3] = max(P', in'), out[4] = number of steps whose borrow differs from (d < 0), out[5] = number of exact ties met
// (d congruent to 2^(k-1) mod 2^k) with d > 0, out[6] = with d < 0
void bp_ranges(const int16_t *x16, int c0, int c1, int sp, long long *out)
{
    int x[16];
    for (int i = 0; i < 16; i++) x[i] = x16[i];
    const PassOut l = pass_fast(x, c0, c1, sp);
    const int k = sp + 11;
    long long o0 = x[0], o1 = x[1];
    out[0] = out[2] = (1ll << 62);
    out[1] = out[3] = -(1ll << 62);
    out[4] = out[5] = out[6] = 0;
    for (int s = 0; s < 14; s++) {
        const long long predicted = o0 * c1 + o1 * c0;
        const long long Pb = predicted + 1024 + PASS_B_OFF, inb = (long long)x[s + 2] * 2048 + 1024 + PASS_B_OFF;
        const long long d = inb - Pb;
        const long long b = (uint32_t)inb < (uint32_t)Pb ? 1 : 0;
        const long long t = (long long)round_through_f32((int)d) + ((1ll << (k - 1)) - 1) - PASS_B_OFF + b;
        out[0] = t < out[0] ? t : out[0];
        out[1] = t > out[1] ? t : out[1];
        out[2] = Pb < out[2] ? Pb : out[2]; out[2] = inb < out[2] ? inb : out[2];
        out[3] = Pb > out[3] ? Pb : out[3]; out[3] = inb > out[3] ? inb : out[3];
        if (b != (d < 0 ? 1 : 0)) out[4]++;
        if ((d & ((1ll << k) - 1)) == (1ll << (k - 1))) out[d > 0 ? 5 : 6]++;
        const long long w = (predicted + (long long)l.q[s] * (1ll << k) + 1024) >> 11;
        o0 = o1;
        o1 = w > 32767 ? 32767 : (w < -32768 ? -32768 : w);
    }
}

}  // extern "C"
