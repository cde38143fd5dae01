// gc_packed_pass_driver.cpp -- host driver for the fast quantise pass on a packed history pair (gc_encode_core.hpp:
// pass_fast_core_t in its three instantiations) against the literal pass.  TEST ONLY, compiled by
// tests/test_host_gc_packed_pass.py from the SAME header the kernel uses; the host build of the header spells out what the
// device's two pair instructions do (dot2_i16, sat_pack16), so this runs the kernel's formulation.
#include "../../vgaudio_amd/csrc/gc_encode_core.hpp"

using namespace vga::gc;

namespace {

// variant 0: the pass with the f32 rounding, 1: NO_ROUND, 2: WIDE_TOTAL
// returns 0 = the pass vouches for itself and equals the literal pass field for field, 1 = it vouches and DIFFERS,
// 2 = it does not vouch (exact == false, or a NO_ROUND pass over its overflow bound): the kernel runs another pass then
int compare_one(const int16_t *x16, int c0, int c1, int sp, int variant)
{
    int x[16], mp[14];
    for (int i = 0; i < 16; i++) x[i] = x16[i];
    for (int s = 0; s < 14; s++) mp[s] = x[s + 2] * 2048 + 1024;
    const uint32_t hist = pack16(x[0], x[1]);
    const PassOut f = variant == 0 ? pass_fast_core(x, hist, mp, c0, c1, sp)
                    : variant == 1 ? pass_fast_core_no_round(x, hist, mp, c0, c1, sp)
                                   : pass_fast_core_wide(x, hist, mp, c0, c1, sp);
    if (!f.exact) return 2;
    if (variant == 1 && !pass_no_round_is_exact(sp, f.max_overflow)) return 2;
    const PassOut l = pass_literal(x, c0, c1, sp);
    bool same = f.total == l.total && f.max_overflow == l.max_overflow && f.hist_pair == l.hist_pair && f.o12 == l.o12 && f.o13 == l.o13;
    for (int s = 0; s < 14; s++) same = same && f.q[s] == l.q[s];
    return same ? 0 : 1;
}

}  // namespace

extern "C" {

int pp_compare(const int16_t *x16, int c0, int c1, int sp, int variant) { return compare_one(x16, c0, c1, sp, variant); }

// n frames of 16 samples each; counts[rc]++ per frame; returns the index of the first frame that differs, -1 if none
int pp_compare_many(const int16_t *x16, const int *c0, const int *c1, const int *sp, int n, int variant, long long *counts)
{
    int first = -1;
    for (int i = 0; i < n; i++) {
        const int rc = compare_one(x16 + (long long)i * 16, c0[i], c1[i], sp[i], variant);
        counts[rc]++;
        if (rc == 1 && first < 0) first = i;
    }
    return first;
}

// The reference's reconstruction before its clamp, sample by sample (the literal pass's nibbles): the longest runs of
// consecutive samples above 32767 (out2[0]) and below -32768 (out2[1]).  A run of two or more is what makes the packed pass
// saturate an out-of-range value a second time (gc_encode_core.hpp P5).
void pp_rail_runs(const int16_t *x16, int c0, int c1, int sp, int *out2)
{
    int x[16];
    for (int i = 0; i < 16; i++) x[i] = x16[i];
    const PassOut l = pass_literal(x, c0, c1, sp);
    int o0 = x[0], o1 = x[1], run_hi = 0, run_lo = 0;
    out2[0] = out2[1] = 0;
    for (int s = 0; s < 14; s++) {
        const int predicted = o0 * c1 + o1 * c0;
        const int w = (predicted + l.q[s] * (1 << (sp + 11)) + 1024) >> 11;
        run_hi = w > 32767 ? run_hi + 1 : 0;
        run_lo = w < -32768 ? run_lo + 1 : 0;
        out2[0] = imax(out2[0], run_hi);
        out2[1] = imax(out2[1], run_lo);
        o0 = o1;
        o1 = clamp16i(w);
    }
}

}  // extern "C"
