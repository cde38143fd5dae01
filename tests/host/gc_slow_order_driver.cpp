// gc_slow_order_driver.cpp -- stand-alone walk of the self-served encoder's queue with the slow groups first
// (vgaudio_amd/csrc/gc_plan8.hpp: plan8_slow_order, plan8_item with the order table, plan8_slow_channel).  Built with
// -fsanitize=address,undefined and run as a program by tests/test_host_gc_slow_order.py; exit status 0 = every check held.
//
// For 1 to 40 channels in 1, 4, 31 and 160 pieces on 1, 8 and 256 compute units, and for the flag patterns none, all, one,
// the first, the last and random ones over 3000 seeds: the item -> (group, piece) map with the table visits every existing
// (group, piece) exactly once, every item of a flagged group comes before every item of another group, and the map is
// the plain piece-major one when no group or every group is flagged.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../vgaudio_amd/csrc/gc_plan8.hpp"

using namespace vga::gc;

namespace {

int g_failures = 0, g_cases = 0;
#define CHECK(cond, ...)                                             \
    do {                                                             \
        if (!(cond)) {                                               \
            if (g_failures++ < 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                            \
    } while (0)

void walk(int cus, int nch, int segments, const std::vector<unsigned char> &flagged, const char *what)
{
    g_cases++;
    const Plan8 p = plan_groups_of_eight(cus, nch, segments, -1);
    CHECK(p.groups == (int)flagged.size() && p.items == p.groups * segments, "%s: nch %d", what, nch);
    std::vector<int> order((size_t)p.groups, -1);
    const int slow = plan8_slow_order(flagged.data(), p.groups, order.data());
    int want_slow = 0;
    for (unsigned char f : flagged) want_slow += f ? 1 : 0;
    CHECK(slow == want_slow, "%s: nch %d slow %d want %d", what, nch, slow, want_slow);
    // the table: a permutation, flagged groups first, ascending inside either part
    std::vector<int> seen((size_t)p.groups, 0);
    for (int i = 0; i < p.groups; i++) {
        const int g = order[(size_t)i];
        CHECK(g >= 0 && g < p.groups, "%s: order[%d] = %d", what, i, g);
        if (g < 0 || g >= p.groups) return;
        seen[(size_t)g]++;
        CHECK((flagged[(size_t)g] != 0) == (i < slow), "%s: order[%d] = %d on the wrong side of %d", what, i, g, slow);
        if (i > 0 && i != slow) CHECK(order[(size_t)i - 1] < g, "%s: order[%d] not ascending", what, i);
    }
    for (int g = 0; g < p.groups; g++) CHECK(seen[(size_t)g] == 1, "%s: group %d in the table %d times", what, g, seen[(size_t)g]);
    // the queue
    std::vector<int> visits((size_t)p.groups * segments, 0);
    bool past_flagged = false;
    for (int item = 0; item < p.items; item++) {
        int g = -1, y = -1;
        const bool any = plan8_item(item, p.groups, nch, nullptr, order.data(), slow, segments, g, y);
        CHECK(any, "%s: item %d of a uniform batch holds no channel", what, item);
        CHECK(g >= 0 && g < p.groups && y >= 0 && y < segments, "%s: item %d -> (%d, %d)", what, item, g, y);
        if (g < 0 || g >= p.groups || y < 0 || y >= segments) return;
        visits[(size_t)y * p.groups + g]++;
        if (!flagged[(size_t)g]) past_flagged = true;
        CHECK(!(flagged[(size_t)g] && past_flagged), "%s: item %d of flagged group %d behind an item of another group", what, item, g);
        int g0 = -1, y0 = -1;
        (void)plan8_item(item, p.groups, nch, nullptr, g0, y0);
        CHECK(g0 == item % p.groups && y0 == item / p.groups, "%s: the plain map moved at item %d", what, item);
        if (slow == 0 || slow == p.groups) CHECK(g == g0 && y == y0, "%s: item %d differs from the plain order", what, item);
    }
    for (size_t i = 0; i < visits.size(); i++) CHECK(visits[i] == 1, "%s: (group, piece) %zu visited %d times", what, i, visits[i]);
}

// the criterion on crafted predictors: complex poles at radius^2 = -c1 / 2048
void criterion()
{
    g_cases++;
    int16_t coefs[16] = {};
    CHECK(!plan8_slow_channel(coefs), "zero coefficients");
    coefs[6] = 3000; coefs[7] = (int16_t)-PLAN8_SLOW_C1;              // complex: 3000^2 < 8192 * 2040
    CHECK(plan8_slow_channel(coefs), "a predictor on the threshold");
    coefs[7] = (int16_t)(-PLAN8_SLOW_C1 + 1);
    CHECK(!plan8_slow_channel(coefs), "a predictor one below the threshold");
    coefs[6] = 4095; coefs[7] = -2047;                                // real poles: 4095^2 > 8192 * 2047
    CHECK(!plan8_slow_channel(coefs), "real poles");
    coefs[6] = 4094;
    CHECK(plan8_slow_channel(coefs), "complex poles next to the real axis");
    coefs[6] = -32768; coefs[7] = -32768;                             // (hostile values: no overflow)
    CHECK(!plan8_slow_channel(coefs), "real poles, extreme values");
    coefs[6] = 0;
    CHECK(plan8_slow_channel(coefs), "extreme c1");
}

}  // namespace

int main()
{
    criterion();
    const int pieces[] = {1, 4, 31, 160}, cus[] = {1, 8, 256};
    std::mt19937 rng(20261020);
    for (int cu : cus)
        for (int segments : pieces)
            for (int nch = 1; nch <= 40; nch++) {
                const int groups = (nch + PLAN8_SLOTS - 1) / PLAN8_SLOTS;
                std::vector<unsigned char> f((size_t)groups, 0);
                walk(cu, nch, segments, f, "none");
                f.assign((size_t)groups, 1);
                walk(cu, nch, segments, f, "all");
                f.assign((size_t)groups, 0); f[(size_t)groups / 2] = 1;
                walk(cu, nch, segments, f, "one");
                f.assign((size_t)groups, 0); f[0] = 1;
                walk(cu, nch, segments, f, "first");
                f.assign((size_t)groups, 0); f[(size_t)groups - 1] = 1;
                walk(cu, nch, segments, f, "last");
            }
    for (int seed = 0; seed < 3000; seed++) {
        const int nch = 1 + (int)(rng() % 40), segments = pieces[rng() % 4], cu = cus[rng() % 3];
        const int groups = (nch + PLAN8_SLOTS - 1) / PLAN8_SLOTS;
        std::vector<unsigned char> f((size_t)groups);
        const unsigned density = rng() % 5;                           // 0: sparse ... 4: dense
        for (auto &v : f) v = (rng() % 5) <= density && (rng() & 1) ? 1 : 0;
        walk(cu, nch, segments, f, "random");
    }
    if (g_failures) {
        std::printf("%d checks failed in %d cases\n", g_failures, g_cases);
        return 1;
    }
    std::printf("ok %d\n", g_cases);
    return 0;
}
