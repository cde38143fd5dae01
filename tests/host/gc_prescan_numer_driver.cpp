// gc_prescan_numer_driver.cpp -- stand-alone check of the tile head's pre-scan word in the numerator domain
// (vgaudio_amd/csrc/gc_encode_core.hpp: prescan_numer_word, N1 and N3-N7) against the reference's form, prescan_range(x, c0, c1,
// 2, 14, ...) with clamp16i, word for word.  Built with -fsanitize=address,undefined and run as a program by
// tests/test_host_gc_prescan_numer.py; exit status 0 = every check held.  Prints "ok <frames> <pinned>": the (frame,
// predictor) pairs compared and how many of the built frames had their chosen D at the maximising / minimising sample.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../vgaudio_amd/csrc/gc_encode_core.hpp"

using namespace vga::gc;

namespace {

long g_failures = 0, g_frames = 0, g_pinned = 0;

uint32_t reference_word(const int (&x)[16], int c0, int c1)
{
    int dmax = 0, dmin = 0;
    prescan_range(x, c0, c1, 2, 14, dmax, dmin);
    return ((uint32_t)clamp16i(dmax) & 0xFFFFu) | ((uint32_t)clamp16i(dmin) << 16);
}

// the operands as the kernel's tile head forms them from the frame in[0..13] = x[2..15]
uint32_t numer_word(const int (&x)[16], int c0, int c1)
{
    uint32_t pair[12];
    int a2048[12];
    for (int k = 0; k < 12; k++) {
        pair[k] = pack16(x[k + 2], x[k + 3]);
        a2048[k] = x[k + 4] * 2048;
    }
    return prescan_numer_word(pair, a2048, pack16(-c1, -c0));
}

void check(const int (&x)[16], int c0, int c1, const char *what)
{
    if (!pass_b_coef_ok(c0, c1)) { std::printf("FAILED %s: the driver built coefficients above the bound\n", what); g_failures++; return; }
    const uint32_t want = reference_word(x, c0, c1), got = numer_word(x, c0, c1);
    g_frames++;
    if (want != got && g_failures++ < 20) {
        std::printf("FAILED %s: c0 %d c1 %d want %08x got %08x  x =", what, c0, c1, want, got);
        for (int i = 0; i < 16; i++) std::printf(" %d", x[i]);
        std::printf("\n");
    }
}

// D of sample s (2..13) in the reference's arithmetic and its distance
int dividend(const int (&x)[16], int c0, int c1, int s) { return x[s] * c1 + x[s + 1] * c0; }
int distance(const int (&x)[16], int c0, int c1, int s) { return x[s + 2] - dividend(x, c0, c1, s) / 2048; }

// A frame whose sample s has the dividend D exactly and the largest (up) or smallest distance of the frame; noise: the other
// samples carry small values instead of zeros.  Returns false where (c0, c1) cannot make that D from int16 samples.
bool build_pinned(int (&x)[16], int c0, int c1, int s, int D, bool up, std::mt19937 &rng, bool noise)
{
    for (int i = 0; i < 16; i++) x[i] = noise ? (int)(rng() % 7) - 3 : 0;
    // D = x[s] * c1 + x[s + 1] * c0: one sample carries most of it, the other the rest
    bool made = false;
    for (int b = -2; b <= 2 && !made; b++) {
        if (c1 != 0 && (D - b * c0) % c1 == 0) {
            const int a = (D - b * c0) / c1;
            if (a >= -32768 && a <= 32767) { x[s] = a; x[s + 1] = b; made = true; }
        } else if (c1 == 0 && c0 != 0 && D % c0 == 0) {
            const int v = D / c0;
            if (v >= -32768 && v <= 32767) { x[s + 1] = v; made = true; }
        }
    }
    if (!made || dividend(x, c0, c1, s) != D) return false;
    x[s + 2] = up ? 30000 : -30000;
    return true;
}

}  // namespace

int main()
{
    std::mt19937 rng(20261020u);
    auto uniform = [&](int lo, int hi) { return lo + (int)(rng() % (uint32_t)(hi - lo + 1)); };
    int x[16];

    // 1. seeded random frames, |c0| + |c1| <= 30720, at every amplitude
    for (int n = 0; n < 1000000; n++) {
        const int amp = 1 << uniform(0, 15);
        for (int i = 0; i < 16; i++) x[i] = clamp16i(uniform(-amp, amp));
        const bool at_bound = (n & 3) == 0;
        const int sum = at_bound ? 30720 : uniform(0, 30720);
        const int a = uniform(0, sum), b = at_bound ? sum - a : uniform(0, sum - a);
        check(x, (rng() & 1) ? a : -a, (rng() & 1) ? b : -b, "random");
    }
    // 2. frames at the rails, alternating and constant, and 3. coefficient sums of exactly 30720 at every sign combination
    const int splits[] = {0, 1, 2047, 2048, 15360, 28672, 30719, 30720};
    for (int phase = 0; phase < 4; phase++) {
        for (int i = 0; i < 16; i++)
            x[i] = phase == 0 ? ((i & 1) ? 32767 : -32768) : phase == 1 ? ((i & 1) ? -32768 : 32767) : phase == 2 ? -32768 : 32767;
        for (int a : splits)
            for (int sg = 0; sg < 4; sg++) check(x, (sg & 1) ? -a : a, (sg & 2) ? -(30720 - a) : 30720 - a, "rails");
    }
    for (int n = 0; n < 20000; n++) {
        for (int i = 0; i < 16; i++) x[i] = (rng() & 1) ? 32767 : -32768;
        const int a = splits[rng() % 8], sg = (int)(rng() & 3);
        check(x, (sg & 1) ? -a : a, (sg & 2) ? -(30720 - a) : 30720 - a, "random rails");
    }
    // 4. D = 0, +-1, +-2047, +-2048, +-2049 at the maximising and at the minimising sample
    const int pairs[][2] = {{0, 1}, {1, 0}, {0, -1}, {-1, 0}, {2047, 1}, {1, 2047}, {-2047, 1}, {2047, -1}, {3, 5}, {30719, 1}};
    const int targets[] = {0, 1, -1, 2047, -2047, 2048, -2048, 2049, -2049, 4095, -4095, 4096, -4096};
    for (const auto &c : pairs)
        for (int D : targets)
            for (int s = 2; s < 14; s++)
                for (int up = 0; up < 2; up++)
                    for (int noise = 0; noise < 2; noise++) {
                        if (!build_pinned(x, c[0], c[1], s, D, up != 0, rng, noise != 0)) continue;
                        bool extreme = true;
                        for (int t = 2; t < 14; t++)
                            if (t != s && (up ? distance(x, c[0], c[1], t) >= distance(x, c[0], c[1], s)
                                              : distance(x, c[0], c[1], t) <= distance(x, c[0], c[1], s))) extreme = false;
                        g_pinned += extreme ? 1 : 0;
                        check(x, c[0], c[1], "pinned D");
                    }
    // 5. all-zero frames
    for (int i = 0; i < 16; i++) x[i] = 0;
    for (int a : splits) { check(x, a, 30720 - a, "zero"); check(x, -a, a - 30720, "zero"); check(x, 0, 0, "zero"); }
    // 6. distances beyond 16 bits either way: the clamp decides (one rail sample among large ones of the other sign)
    for (int n = 0; n < 20000; n++) {
        const int sign = (n & 1) ? 1 : -1;
        for (int i = 0; i < 16; i++) x[i] = sign * uniform(20000, 32767);
        x[uniform(4, 15)] = sign > 0 ? -32768 : 32767;
        const int a = uniform(8000, 15360), b = uniform(8000, 15360);
        check(x, (n & 2) ? a : -a, (n & 4) ? b : -b, "clamp");
    }
    if (g_pinned < 1000) { std::printf("FAILED: only %ld built frames had their D at the extreme sample\n", g_pinned); g_failures++; }
    if (g_failures) { std::printf("%ld of %ld comparisons failed\n", g_failures, g_frames); return 1; }
    std::printf("ok %ld %ld\n", g_frames, g_pinned);
    return 0;
}
