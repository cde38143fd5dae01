// gc_flag_masks_driver.cpp -- host driver for the one-bit form of the frame's flags (gc_encode_core.hpp: frame_goes_cold)
// against frame_flags, which the kernel's cold branch, ColdState, the lane-per-candidate layout and the seam code keep
// reading.  TEST ONLY, compiled by tests/test_host_gc_flag_masks.py from the SAME header the kernel uses.
#include "../../vgaudio_amd/csrc/gc_encode_core.hpp"

using namespace vga::gc;

extern "C" {

// One tuple.  out: cold, fin_a of frame_goes_cold; fin_a, generic, resume, inexact, bump_a of frame_flags; and the same four
// flags as the kernel derives them inside its cold branch (a lane that is not cold is never asked).
// Returns a bit set of what differs: 1 = cold != (generic || resume || inexact), 2 = fin_a, 4 = a flag of a cold lane
// derived inside the branch is not the flag of frame_flags.
int fm_check(int sp_a, int sp_b, int ov_a, int ov_2, int coef_ok, int *out)
{
    const FrameCold c = frame_goes_cold(sp_a, sp_b, ov_a, ov_2, coef_ok != 0);
    const FrameFlags f = frame_flags(sp_a, sp_b, ov_a, ov_2, coef_ok != 0);
    // what encode_frame8 hands to the cold block: behind the branch on the ballot of `cold`
    bool generic = false, resume = false, inexact = false, bump_a = false;
    if (c.cold) {
        const FrameFlags in = frame_flags(sp_a, sp_b, ov_a, ov_2, coef_ok != 0);
        generic = in.generic; resume = in.resume; inexact = in.inexact; bump_a = in.bump_a;
    }
    if (out) {
        out[0] = c.cold; out[1] = c.fin_a; out[2] = f.fin_a; out[3] = f.generic; out[4] = f.resume; out[5] = f.inexact;
        out[6] = f.bump_a; out[7] = generic; out[8] = resume; out[9] = inexact; out[10] = bump_a;
    }
    int bad = 0;
    if (c.cold != (f.generic || f.resume || f.inexact)) bad |= 1;
    if (c.fin_a != f.fin_a || c.fin_a != pass_a_is_final(sp_a, ov_a)) bad |= 2;
    if (c.cold && (generic != f.generic || resume != f.resume || inexact != f.inexact || bump_a != f.bump_a)) bad |= 4;
    // a lane that stays hot must have nothing for the cold block to do
    if (!c.cold && (f.generic || f.resume || f.inexact || f.bump_a || f.bump_b)) bad |= 1;
    return bad;
}

// sp_a 0..12, sp_b = min(sp_a + 1, 12), ov_a and ov_2 over ovs, coef_ok 0 / 1.  counts[0] = tuples visited, [1] = cold ones,
// [2] = fin_a ones, [3..6] = generic, resume, inexact, bump_a ones.  Returns the number of tuples with a difference; *first
// receives (sp_a, ov_a, ov_2, coef_ok, bits) of the first such tuple.
int fm_enumerate(const int *ovs, int n_ov, long long *counts, int *first)
{
    int bad = 0;
    for (int i = 0; i < 7; i++) counts[i] = 0;
    for (int sp_a = 0; sp_a <= 12; sp_a++)
        for (int ia = 0; ia < n_ov; ia++)
            for (int ib = 0; ib < n_ov; ib++)
                for (int ok = 0; ok < 2; ok++) {
                    const int sp_b = imin(sp_a + 1, 12);
                    int out[11];
                    const int bits = fm_check(sp_a, sp_b, ovs[ia], ovs[ib], ok, out);
                    counts[0]++;
                    counts[1] += out[0]; counts[2] += out[1];
                    counts[3] += out[3]; counts[4] += out[4]; counts[5] += out[5]; counts[6] += out[6];
                    if (bits && !bad++ && first) {
                        first[0] = sp_a; first[1] = ovs[ia]; first[2] = ovs[ib]; first[3] = ok; first[4] = bits;
                    }
                }
    return bad;
}

}  // extern "C"
