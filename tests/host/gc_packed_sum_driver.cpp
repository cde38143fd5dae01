// gc_packed_sum_driver.cpp -- host driver for the fast quantise pass's error sum in packed pairs (gc_encode_core.hpp E1-E5,
// round 8) and for the exact-sum rule of the encoder's cold block.  TEST ONLY, compiled by tests/test_host_gc_packed_sum.py
// from the SAME header the kernel uses; the host build of the header spells out what v_pk_sub_i16 and v_dot2_i32_i16 do
// with their clamp bits (pk_sub_sat_i16, dot2_i16), so this runs the kernel's formulation.
#include "../../vgaudio_amd/csrc/gc_encode_core.hpp"
#include <cstring>

using namespace vga::gc;

namespace {

// The scalar 64-bit error sum of a pass, from nothing but its nibbles: the reconstruction as the pass defines it (P1, P3,
// P4: predictor sum saturated to int32, floor shift, clamp to int16), written out in 64-bit arithmetic.
// max_abs_e: the largest |x - o| of the fourteen.
uint64_t scalar_sum(const int (&x)[16], const int (&q)[14], int c0, int c1, int sp, int &max_abs_e)
{
    int o0 = x[0], o1 = x[1];
    uint64_t total = 0;
    max_abs_e = 0;
    for (int s = 0; s < 14; s++) {
        long long P = (long long)o0 * c1 + (long long)o1 * c0 + 1024;
        if (P > 2147483647ll) P = 2147483647ll;
        if (P < -2147483648ll) P = -2147483648ll;
        long long w = (P >> 11) + (long long)q[s] * (1ll << sp);
        const int o = (int)(w > 32767 ? 32767 : (w < -32768 ? -32768 : w));
        const long long e = (long long)x[s + 2] - o;
        total += (uint64_t)(e * e);
        const int ae = (int)(e < 0 ? -e : e);
        if (ae > max_abs_e) max_abs_e = ae;
        o0 = o1;
        o1 = o;
    }
    return total;
}

}  // namespace

extern "C" {

// n frames of 16 samples (x[0], x[1] the history); variant 0: the pass with the f32 rounding, 1: NO_ROUND.
// counts: [0] exact sum < 2^28 and packed == exact   [1] exact sum >= 2^28 and packed >= 2^28   [2] VIOLATIONS
//         [3] frames with an error that does not fit int16 (a saturated half)   [4] frames whose exact sum is >= 2^31
//         [5] frames whose pass vouches (exact == true) -- for them packed == exact is required whatever the size
// returns the index of the first violating frame, -1 if none
int ps_check_many(const int16_t *x16, const int *c0, const int *c1, const int *sp, int n, int variant, long long *counts)
{
    int first = -1;
    for (int i = 0; i < n; i++) {
        int x[16], mp[14];
        for (int k = 0; k < 16; k++) x[k] = x16[(long long)i * 16 + k];
        for (int s = 0; s < 14; s++) mp[s] = x[s + 2] * 2048 + 1024;
        uint32_t xw[7];
        pack_row(x, xw);
        const uint32_t hist = pack16(x[0], x[1]);
        const PassOut f = variant == 0 ? pass_fast_core(xw, hist, mp, c0[i], c1[i], sp[i])
                                       : pass_fast_core_no_round(xw, hist, mp, c0[i], c1[i], sp[i]);
        int max_e;
        const uint64_t exact = scalar_sum(x, f.q, c0[i], c1[i], sp[i], max_e);
        bool ok = exact < (1ull << 28) ? f.total == exact : f.total >= (1ull << 28);
        if (f.exact) { counts[5]++; ok = ok && f.total == exact; }
        // (the wide pass is the scalar sum for coefficients that cannot wrap: the cold block's authority)
        const int ac0 = c0[i] < 0 ? -c0[i] : c0[i], ac1 = c1[i] < 0 ? -c1[i] : c1[i];
        if (ac0 + ac1 <= 32767 && variant == 0) ok = ok && pass_fast_core_wide(xw, hist, mp, c0[i], c1[i], sp[i]).total == exact;
        counts[ok ? (exact < (1ull << 28) ? 0 : 1) : 2]++;
        if (max_e > 32767) counts[3]++;
        if (exact >= (1ull << 31)) counts[4]++;
        if (!ok && first < 0) first = i;
    }
    return first;
}

// One channel through the (channel, predictor) layout's frame as the kernel resolves it since round 8 (encode_frame8,
// encode_frame_cold and the exact-sum rule in gc_encode_kernel.hip): both candidate passes on the packed row, per lane the
// reference's loop as written where the kernel takes it, third trips, 32-bit keys that saturate at 2^28, and -- only when the
// channel's best key saturated -- the wide pass for every final lane at or above 2^28 whose sum is not known to be exact, then
// 64-bit keys.  (The kernel shares its decisions between the eight channels of a wave; none of them changes a lane's result.)
// stats: [0] frames  [1] frames whose best key saturated (64-bit keys decided)  [2] lanes sent through the wide pass
//        [3] final lanes with an error that does not fit int16  [4] final lanes whose packed sum differed from the exact one
//        [5] frames where taking the packed sums as they are would have picked another predictor
int ps_encode8(const int16_t *pcm, int sample_count, const int16_t *coefs, int16_t hist1, int16_t hist2, uint8_t *out, uint64_t *stats)
{
    int x[16];
    x[0] = hist2;
    x[1] = hist1;
    const int full_frames = sample_count / 14;
    const int tail = sample_count - full_frames * 14;
    const int frames = full_frames + (tail ? 1 : 0);
    for (int f = 0; f < frames; f++) {
        for (int s = 0; s < 14; s++) {
            const int idx = f * 14 + s;
            x[2 + s] = idx < sample_count ? pcm[idx] : 0;
        }
        stats[0]++;
        int mp[14];
        for (int s = 0; s < 14; s++) mp[s] = x[s + 2] * 2048 + 1024;
        uint32_t xw[7];
        pack_row(x, xw);
        const uint32_t hist = pack16(x[0], x[1]);
        PassOut fin[8];
        int fin_sp[8];
        bool sum_exact[8];
        for (int p = 0; p < 8; p++) {
            const int c0 = coefs[2 * p], c1 = coefs[2 * p + 1];
            const bool coef_ok = (c0 < 0 ? -c0 : c0) + (c1 < 0 ? -c1 : c1) <= 32767;
            // the two history-dependent distances from pairs, the rest as the helper wave computes them
            const uint32_t cpk = pack16(c1, c0);
            const int d0 = pair_lo(xw[0]) - div2048(dot2_i16_wrap(hist, cpk));
            const int d1 = pair_hi(xw[0]) - div2048(dot2_i16_wrap(pack16(x[1], x[2]), cpk));
            int dmax = imax(imax(0, d0), d1), dmin = imin(imin(0, d0), d1);
            prescan_range(x, c0, c1, 2, 14, dmax, dmin);
            int s1 = first_scale_power_from_range(dmax, dmin);
            if (s1 == -100) s1 = first_scale_power_from_md(prescan_sequential(x, c0, c1));
            const int sp_a = imin(s1, 12), sp_b = imin(s1 + 1, 12);
            const PassOut rb = pass_fast_core(xw, hist, mp, c0, c1, sp_b), ra = pass_fast_core(xw, hist, mp, c0, c1, sp_a);
            const bool cap_a = sp_a >= 12, cap_b = sp_b >= 12;
            const int eff_a = cap_a ? 0 : ra.max_overflow, eff_b = cap_b ? 0 : rb.max_overflow;
            const bool fin_a = eff_a < 2;
            const bool bump_a = !cap_a && (unsigned)ra.max_overflow > 248u;
            const bool bump_b = !fin_a && !cap_b && (unsigned)rb.max_overflow > 248u;
            const bool generic = !coef_ok || bump_a || bump_b;
            const bool resume = !generic && !fin_a && eff_b >= 2;
            PassOut r = fin_a ? ra : rb;
            int fsp = fin_a ? sp_a : sp_b;
            bool known = false;
            if (generic) {
                const int start = !coef_ok ? s1 - 1 : (bump_a ? apply_bumps(s1, ra.max_overflow) : apply_bumps(s1 + 1, rb.max_overflow));
                r = resume_passes(x, c0, c1, start, fsp);
                known = true;
            }
            if (resume) {
                int sp = s1 + 1;
                for (;;) {
                    sp++;
                    bool short_pass = sp <= 9;
                    if (short_pass) {
                        r = pass_fast_core_no_round(xw, hist, mp, c0, c1, sp);
                        short_pass = pass_no_round_is_exact(sp, r.max_overflow);
                    }
                    if (!short_pass) r = pass_fast_core(xw, hist, mp, c0, c1, sp);
                    const bool cap = sp >= 12;
                    if ((unsigned)r.max_overflow > (cap ? 3u : 248u)) { r = resume_passes(x, c0, c1, sp - 1, fsp); known = true; break; }
                    fsp = sp;
                    if (cap || r.max_overflow <= 1) break;
                }
            }
            fin[p] = r;
            fin_sp[p] = fsp;
            sum_exact[p] = known;
            if (!known) {                                  // diagnostics only
                int max_e;
                const uint64_t exact = scalar_sum(x, r.q, c0, c1, fsp, max_e);
                if (max_e > 32767) stats[3]++;
                if (exact != r.total) stats[4]++;
            }
        }
        const unsigned SAT = (1u << 28) - 1;
        unsigned best32 = 0xFFFFFFFFu;
        for (int p = 0; p < 8; p++) {
            const unsigned tot = (fin[p].total >> 32) ? SAT : ((unsigned)fin[p].total < SAT ? (unsigned)fin[p].total : SAT);
            const unsigned key = (tot << 3) | (unsigned)p;
            if (key < best32) best32 = key;
        }
        int winner = (int)(best32 & 7u);
        if ((best32 >> 3) >= SAT) {
            stats[1]++;
            uint64_t best = ~0ull, naive = ~0ull;
            for (int p = 0; p < 8; p++) {
                uint64_t total = fin[p].total;
                const uint64_t nkey = (total << 3) | (uint64_t)p;
                if (nkey < naive) naive = nkey;
                if (needs_exact_sum(total, sum_exact[p])) {
                    total = pass_fast_core_wide(xw, hist, mp, coefs[2 * p], coefs[2 * p + 1], fin_sp[p]).total;
                    stats[2]++;
                }
                const uint64_t key = (total << 3) | (uint64_t)p;
                if (key < best) best = key;
            }
            winner = (int)(best & 7u);
            if ((int)(naive & 7u) != winner) stats[5]++;
        }
        uint8_t frame[8];
        uint32_t d0, d1;
        frame_words(fin[winner], winner, fin_sp[winner], d0, d1);
        memcpy(frame, &d0, 4);
        memcpy(frame + 4, &d1, 4);
        const int nbytes = f < full_frames ? 8 : (tail + 2 + 1) / 2;
        memcpy(out + (size_t)f * 8, frame, (size_t)nbytes);
        x[0] = fin[winner].o12;
        x[1] = fin[winner].o13;
    }
    return 0;
}

}  // extern "C"
