// gc_plan8_driver.cpp -- stand-alone walk of the self-served encoder's queue (vgaudio_amd/csrc/gc_plan8.hpp): group
// counts, item counts, the item decode the kernel uses, for uniform and ragged batches.  Built with
// -fsanitize=address,undefined and run as a program by tests/test_host_gc_plan8.py; exit status 0 = every check held.
//
// For every batch: each (channel, frame) must belong to exactly one queue item, with a piece existing for a group of eight
// as the kernel decides it (its slot 0 reaches the piece), and the queue must be as long as the launch says.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../vgaudio_amd/csrc/gc_host.hpp"
#include "../../vgaudio_amd/csrc/gc_plan8.hpp"

// (gc_host.hpp reports its argument errors through the library's set_error; nothing walked here raises one)
void vga::set_error(const char *, ...) {}

using namespace vga;
using namespace vga::gc;

namespace {

// (gcadpcm_kernels.hpp's Pieces, which needs HIP: `nb` pieces of `big` frames, then pieces of `small`)
struct Sched {
    int big, nb, small, segments;
    int64_t first(int k) const { return (int64_t)std::min(k, nb) * big + (int64_t)std::max(k - nb, 0) * small; }
    int frames(int k) const { return k < nb ? big : small; }
};

int g_failures = 0, g_cases = 0;
#define CHECK(cond, ...)                                             \
    do {                                                             \
        if (!(cond)) {                                               \
            if (g_failures++ < 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                            \
    } while (0)

// equal pieces as the segments test hook asks for them, or a two-size schedule
Sched equal_pieces(int frames, int want)
{
    const int segments = std::max(1, std::min(std::max(frames / 64, 1), want));
    const int big = (frames + segments - 1) / segments;
    Sched s{big, segments, big, segments};
    while (s.segments > 1 && s.first(s.segments - 1) >= frames) s.segments--;
    return s;
}
Sched two_sizes(int frames, int big, int small)
{
    int nb = std::max(1, (frames / 2 + big - 1) / big);
    Sched s{big, nb, small, nb};
    while (s.first(s.segments) < frames) s.segments++;
    return s;
}

// ragged == false: every channel has lengths[0] samples and the queue is piece-major; true: the host's item list, made as
// RaggedShape::build (gc_capi.hpp) makes it -- (group of sixteen, piece) items, biggest first
void walk(int cus, const std::vector<int> &lengths, const Sched &s, bool ragged, const char *what)
{
    g_cases++;
    const int nch = (int)lengths.size();
    RaggedLayout L;
    L.lay_out(lengths.data(), nch, 0, 0);
    std::vector<uint32_t> host_items;
    if (ragged) {
        struct Item { int size, y, g; };
        std::vector<Item> list;
        for (int y = 0; y < s.segments; y++)
            for (int g = 0; g < (int)L.group_frames.size(); g++)
                if (s.first(y) < L.group_frames[g])
                    list.push_back({(int)std::min<int64_t>(s.frames(y), L.group_frames[g] - s.first(y)), y, g});
        std::stable_sort(list.begin(), list.end(), [](const Item &a, const Item &b) { return a.size > b.size; });
        for (const Item &it : list) host_items.push_back(((uint32_t)it.y << 20) | (uint32_t)it.g);
    }
    const Plan8 p = plan_groups_of_eight(cus, nch, s.segments, ragged ? (int)host_items.size() : -1);
    CHECK(p.groups == (nch + 7) / 8, "%s: nch %d groups %d", what, nch, p.groups);
    CHECK(p.items == (ragged ? 2 * (int)host_items.size() : p.groups * s.segments), "%s: nch %d items %d", what, nch, p.items);
    CHECK(p.wgs == std::min(p.items, cus * PLAN8_WGS_PER_CU) && p.wgs >= (p.items > 0 ? 1 : 0), "%s: nch %d wgs %d", what, nch, p.wgs);
    CHECK((int64_t)p.rounds_x16 * p.wgs >= (int64_t)p.items * 16 && (int64_t)(p.rounds_x16 - 1) * p.wgs < (int64_t)p.items * 16 + p.wgs,
          "%s: nch %d rounds %d", what, nch, p.rounds_x16);
    std::vector<std::vector<uint8_t>> seen(nch);
    for (int c = 0; c < nch; c++) seen[c].assign((size_t)(((int64_t)lengths[c] + 13) / 14), 0);
    std::vector<uint8_t> taken((size_t)p.groups * s.segments, 0);
    int pieces = 0;
    for (int item = 0; item < p.items; item++) {
        int g = -1, y = -1;
        const bool any = plan8_item(item, p.groups, nch, ragged ? host_items.data() : nullptr, g, y);
        if (!any) {
            CHECK(ragged && (item & 1) && g * PLAN8_SLOTS >= nch, "%s: item %d empty, group %d of %d channels", what, item, g, nch);
            continue;
        }
        CHECK(g >= 0 && g < p.groups && y >= 0 && y < s.segments, "%s: item %d -> group %d piece %d", what, item, g, y);
        if (g < 0 || g >= p.groups || y < 0 || y >= s.segments) continue;
        CHECK(!taken[(size_t)y * p.groups + g], "%s: (group %d, piece %d) twice", what, g, y);
        taken[(size_t)y * p.groups + g] = 1;
        // the kernel's rule: the piece exists for the group when its slot 0 (its longest channel) reaches it
        const int longest = lengths[L.order[g * PLAN8_SLOTS]];
        if (s.first(y) * 14 >= longest) continue;
        pieces++;
        for (int slot = g * PLAN8_SLOTS; slot < std::min(nch, (g + 1) * PLAN8_SLOTS); slot++) {
            const int c = L.order[slot];
            CHECK(lengths[c] <= longest, "%s: slot %d longer than its group's slot 0", what, slot);
            const int64_t end = std::min<int64_t>(s.first(y) + s.frames(y), (int64_t)seen[c].size());
            for (int64_t f = s.first(y); f < end; f++) seen[c][(size_t)f]++;
        }
    }
    for (int c = 0; c < nch; c++)
        for (size_t f = 0; f < seen[c].size(); f++)
            if (seen[c][f] != 1) {
                CHECK(seen[c][f] == 1, "%s: nch %d channel %d frame %zu belongs to %d items", what, nch, c, f, (int)seen[c][f]);
                break;
            }
    // what the launch enqueues: with a piece-major queue every (group, piece) once, existing or not
    if (!ragged) {
        CHECK(std::count(taken.begin(), taken.end(), 1) == (long)p.items, "%s: nch %d: %d items, not every (group, piece)", what, nch, p.items);
        const int frames = (lengths[0] + 13) / 14;
        int existing = 0;
        for (int y = 0; y < s.segments; y++) existing += s.first(y) < frames ? 1 : 0;
        CHECK(pieces == existing * p.groups, "%s: nch %d: %d pieces encoded, %d planned", what, nch, pieces, existing * p.groups);
    }
}

}  // namespace

int main()
{
    const int edge[] = {1, 13, 14, 15, 111, 112, 113, 335, 336, 337, 4205};
    const int n_edge = (int)(sizeof edge / sizeof edge[0]);
    for (int cus : {1, 8, 256})
        for (int nch = 1; nch <= 40; nch++) {
            for (int e = 0; e < n_edge; e++)
                for (int want : {1, 4, 160}) {
                    const int frames = (edge[e] + 13) / 14;
                    walk(cus, std::vector<int>((size_t)nch, edge[e]), equal_pieces(frames, want), false, "uniform");
                }
            // ragged: every edge length in turn, rotated so that the groups of eight differ
            for (int rot = 0; rot < 3; rot++) {
                std::vector<int> lengths((size_t)nch);
                for (int c = 0; c < nch; c++) lengths[(size_t)c] = edge[(c + rot * 4 + c / 8) % n_edge];
                const int frames = (*std::max_element(lengths.begin(), lengths.end()) + 13) / 14;
                for (int want : {1, 4, 160}) walk(cus, lengths, equal_pieces(frames, want), true, "ragged");
                walk(cus, lengths, two_sizes(frames, 100, 64), true, "ragged, two sizes");
            }
        }
    // long channels: the two-size schedule, more items than workgroups
    walk(256, std::vector<int>(160, 143367), equal_pieces(10241, 160), false, "uniform, many items");
    walk(256, std::vector<int>(40, 2880000), two_sizes(205715, 50000, 4096), false, "uniform, two sizes");
    {
        std::vector<int> lengths(40);
        for (int c = 0; c < 40; c++) lengths[(size_t)c] = 2880000 / (1 + c % 7);
        walk(256, lengths, two_sizes(205715, 50000, 4096), true, "ragged, long");
    }
    // nothing to do
    const Plan8 none = plan_groups_of_eight(256, 0, 1, -1);
    CHECK(none.groups == 0 && none.items == 0 && none.wgs == 0, "empty batch");
    std::printf("%s: %d batches walked, %d failures\n", g_failures ? "FAILED" : "ok", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
