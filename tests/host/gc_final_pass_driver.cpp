// gc_final_pass_driver.cpp -- host driver for the frame resolution of the (channel, predictor) layout since round 11
// (gc_encode_core.hpp: final_pass_pair, T1 / T2, frame_flags on ov_2) against the form it replaces, restated here from the
// header's functions: pass B at s1 + 1 and pass A at s1, both result sets kept, 21 selects on fin_a, the flags as the frame
// code wrote them.  TEST ONLY, compiled by tests/test_host_gc_final_pass.py from the SAME header the kernel uses.
#include "../../vgaudio_amd/csrc/gc_encode_core.hpp"

using namespace vga::gc;

namespace {

// what a lane hands to the frame's tail, and whether it asks for the cold block
struct Lane {
    int q[14];            // nibbles mod 16
    uint32_t hist_pair, total;
    int final_sp, cold, max_overflow;
    int fin_a, ov_a, ov_b;
    int generic, inexact, resume, bump_a;
    int trusted;          // the NO_ROUND pair vouches for itself
};

// the flags as encode_frame8 wrote them until round 11 (kept literally: this is the reference of the enumeration)
struct OldFlags { bool fin_a, bump_a, bump_b, generic, inexact, resume; };
OldFlags old_flags(int sp_a, int sp_b, int ov_a, int ov_b, bool coef_ok)
{
    OldFlags f;
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

// Round 11, step 2 -- "does the lane go to the cold block" as compares and mask logic, no branch -- was measured and not
// kept (LABNOTES 16): the expression stays here with its enumeration for whoever takes it up again.  thr = 1 below the cap,
// 3 at it; a_bad = ov_a > thr(sp_a), b_bad = ov_2 > thr(sp_b).
int step2_limit(int sp) { return sp >= 12 ? 3 : 1; }
bool step2_goes_cold(bool coef_ok, bool cap_a, int ov_a, bool a_bad, bool b_bad)
{
    return !coef_ok | (a_bad & (cap_a | (ov_a > 248) | b_bad));
}

struct Frame {
    uint32_t xw[7];
    int mb[14];
    uint32_t hist;
    int P0;
};
Frame make_frame(const int16_t *x16, int c0, int c1)
{
    Frame f;
    int x[16];
    for (int i = 0; i < 16; i++) x[i] = x16[i];
    for (int s = 0; s < 14; s++) f.mb[s] = pass_b_row(x[s + 2]);
    pack_row(x, f.xw);
    f.hist = pack16(x[0], x[1]);
    f.P0 = predicted_b(f.hist, pack16(c1, c0));
    return f;
}

// passes B and A, both sets, selects
template <bool NO_ROUND>
Lane lane_old(const Frame &f, int c0, int c1, int s1)
{
    const int sp_a = imin(s1, 12), sp_b = imin(s1 + 1, 12);
    const bool coef_ok = pass_b_coef_ok(c0, c1);
    const PassOutB rb = pass_fast_core_b<NO_ROUND, true, false>(f.xw, f.hist, f.mb, c0, c1, sp_b, f.P0);
    const PassOutB ra = pass_fast_core_b<NO_ROUND, true, false>(f.xw, f.hist, f.mb, c0, c1, sp_a, f.P0);
    const OldFlags g = old_flags(sp_a, sp_b, ra.max_overflow, rb.max_overflow, coef_ok);
    Lane o;
    for (int i = 0; i < 14; i++) o.q[i] = (g.fin_a ? ra.q2[i] : rb.q2[i]) & 15;
    uint32_t sel[7];
    for (int i = 0; i < 7; i++) sel[i] = g.fin_a ? ra.pairs[i] : rb.pairs[i];
    o.total = error_sum_pairs(f.xw, sel);
    o.hist_pair = sel[6];
    o.max_overflow = g.fin_a ? ra.max_overflow : rb.max_overflow;
    o.final_sp = g.fin_a ? sp_a : sp_b;
    o.cold = g.generic || g.resume || g.inexact;
    o.fin_a = g.fin_a; o.ov_a = ra.max_overflow; o.ov_b = rb.max_overflow;
    o.generic = g.generic; o.inexact = g.inexact; o.resume = g.resume; o.bump_a = g.bump_a;
    o.trusted = !coef_ok || (pass_no_round_is_exact(sp_a, ra.max_overflow) && pass_no_round_is_exact(sp_b, rb.max_overflow));
    return o;
}

// the frame code as it is now: final_pass_pair, the flags from (ov_a, ov_2)
template <bool NO_ROUND>
Lane lane_new(const Frame &f, int c0, int c1, int s1)
{
    const int sp_a = imin(s1, 12), sp_b = imin(s1 + 1, 12);
    const bool coef_ok = pass_b_coef_ok(c0, c1);
    int ov_a, sp2;
    const PassOutB r = final_pass_pair<NO_ROUND>(f.xw, f.hist, f.mb, c0, c1, sp_a, sp_b, f.P0, ov_a, sp2);
    const int ov_2 = r.max_overflow;
    Lane o;
    for (int i = 0; i < 14; i++) o.q[i] = r.q2[i] & 15;
    o.total = error_sum_pairs(f.xw, r.pairs);
    o.hist_pair = r.hist_pair;
    o.max_overflow = ov_2;
    o.final_sp = sp2;
    const FrameFlags g = frame_flags(sp_a, sp_b, ov_a, ov_2, coef_ok);
    o.cold = g.generic || g.resume || g.inexact;
    o.fin_a = g.fin_a; o.ov_a = ov_a; o.ov_b = ov_2;
    o.generic = g.generic; o.inexact = g.inexact; o.resume = g.resume; o.bump_a = g.bump_a;
    o.trusted = !coef_ok || (pass_no_round_is_exact(sp_a, ov_a) && pass_no_round_is_exact(sp2, ov_2));
    return o;
}

bool same_result(const Lane &a, const Lane &b)
{
    bool same = a.hist_pair == b.hist_pair && a.total == b.total && a.final_sp == b.final_sp && a.cold == b.cold &&
                a.max_overflow == b.max_overflow && a.fin_a == b.fin_a && a.ov_a == b.ov_a && a.generic == b.generic &&
                a.inexact == b.inexact && a.resume == b.resume && a.bump_a == b.bump_a;
    for (int i = 0; i < 14; i++) same = same && a.q[i] == b.q[i];
    // pass B's overflow: the new form has it wherever anything reads it -- in a lane that is not fin_a
    if (!a.fin_a) same = same && a.ov_b == b.ov_b;
    return same;
}

// returns 0 = the new resolution equals the old one, 1 = they DIFFER, 2 = not compared (a no-round pair that does not
// vouch for itself: the kernel runs the wave's frame again with the conversions).
// no_round: the new no-round pair, where it vouches for itself, against the old ROUNDED pair -- that is what it promises --
// and, where the old no-round pair vouched as well, against that one too; the new test is never the stricter one.
// info: fin_a, cold, ov_a, ov_b (pass B's own), final_sp, generic, inexact, resume, bump_a -- of the old form
int compare_one(const int16_t *x16, int c0, int c1, int s1, int no_round, int *info)
{
    const Frame f = make_frame(x16, c0, c1);
    const Lane o = lane_old<false>(f, c0, c1, s1);
    if (info) {
        info[0] = o.fin_a; info[1] = o.cold; info[2] = o.ov_a; info[3] = o.ov_b; info[4] = o.final_sp;
        info[5] = o.generic; info[6] = o.inexact; info[7] = o.resume; info[8] = o.bump_a;
    }
    if (!no_round) return same_result(o, lane_new<false>(f, c0, c1, s1)) ? 0 : 1;
    const Lane n = lane_new<true>(f, c0, c1, s1);
    const Lane on = lane_old<true>(f, c0, c1, s1);
    if (on.trusted && !n.trusted) return 1;
    if (!n.trusted) return 2;
    if (!pass_b_coef_ok(c0, c1)) return n.cold && o.cold ? 0 : 1;     // (such a lane walks the reference's loop whatever the passes say)
    if (on.trusted && !same_result(on, n)) return 1;
    return same_result(o, n) ? 0 : 1;
}

}  // namespace

extern "C" {

int fp_compare(const int16_t *x16, int c0, int c1, int s1, int no_round, int *info)
{
    return compare_one(x16, c0, c1, s1, no_round, info);
}

// n frames of 16 samples each; counts[rc]++ per frame; info: 9 ints per frame (may be null); returns the index of the first
// frame with rc 1, -1 if none
int fp_compare_many(const int16_t *x16, const int *c0, const int *c1, const int *s1, int n, int no_round, long long *counts, int *info)
{
    int first = -1;
    for (int i = 0; i < n; i++) {
        const int rc = compare_one(x16 + (long long)i * 16, c0[i], c1[i], s1[i], no_round, info ? info + 9ll * i : nullptr);
        counts[rc]++;
        if (rc == 1 && first < 0) first = i;
    }
    return first;
}

// the first scale the kernel's pre-scan arrives at for the frame (the reference's :107-124)
int fp_first_scale(const int16_t *x16, int c0, int c1)
{
    int x[16];
    for (int i = 0; i < 16; i++) x[i] = x16[i];
    return first_scale_power_from_md(prescan_sequential(x, c0, c1));
}

// The flags from (ov_a, ov_2), ov_2 = fin_a ? ov_a : ov_b (T1, T2), and step 2's one-bit form against the expressions of
// the old frame code, over (sp_a, ov_a, ov_b, coef_ok); ovs: n_ov overflow values.  Returns the number of tuples that differ
// in fin_a, in "goes to the cold block" (either form), or in any single flag; *visited = tuples looked at.
int fp_enumerate_flags(const int *ovs, int n_ov, long long *visited)
{
    int bad = 0;
    *visited = 0;
    for (int s1 = 0; s1 <= 12; s1++)
        for (int ia = 0; ia < n_ov; ia++)
            for (int ib = 0; ib < n_ov; ib++)
                for (int ok = 0; ok < 2; ok++) {
                    const int sp_a = imin(s1, 12), sp_b = imin(s1 + 1, 12);
                    const int ov_a = ovs[ia], ov_b = ovs[ib];
                    const OldFlags g = old_flags(sp_a, sp_b, ov_a, ov_b, ok != 0);
                    const bool old_cold = g.generic || g.resume || g.inexact;
                    const bool fin_a = pass_a_is_final(sp_a, ov_a);
                    const int ov_2 = fin_a ? ov_a : ov_b;
                    const bool a_bad = ov_a > step2_limit(sp_a), b_bad = ov_2 > step2_limit(sp_b);
                    const bool cold = step2_goes_cold(ok != 0, sp_a >= 12, ov_a, a_bad, b_bad);
                    const FrameFlags n = frame_flags(sp_a, sp_b, ov_a, ov_2, ok != 0);
                    const bool same = fin_a == g.fin_a && fin_a == (sp_a >= 12 || !a_bad) && cold == old_cold &&
                                      (n.generic || n.resume || n.inexact) == old_cold && n.fin_a == g.fin_a &&
                                      n.bump_a == g.bump_a && n.bump_b == g.bump_b && n.generic == g.generic &&
                                      n.inexact == g.inexact && n.resume == g.resume;
                    if (!same) bad++;
                    (*visited)++;
                }
    return bad;
}

}  // extern "C"
