// gc_plan8.hpp -- the queue of the GC-ADPCM encoder's self-served shape (gc_encode_self_served_kernel, gc_encode_kernel.hip):
// one-wave workgroups of eight channel slots, twelve per compute unit.  Host arithmetic and the item decode the kernel
// shares with it; free of HIP types, so that tests/host/gc_plan8_driver.cpp walks it without a device.
//
// The piece schedule is NOT planned here: it stays gc::plan_encode_pieces' (for groups of sixteen), so that a channel has
// the seams it has with the 2 + 1 shape.  A group of sixteen work slots is two groups of eight: slots 16 g .. 16 g + 7 and
// 16 g + 8 .. 16 g + 15 (ragged batches: `order` is longest first, so slot 0 of either half is its longest channel).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VGA_PLAN8_HD __host__ __device__
#else
#define VGA_PLAN8_HD
#endif

namespace vga {
namespace gc {

constexpr int PLAN8_SLOTS = 8;                 // channel slots per workgroup
constexpr int PLAN8_WGS_PER_CU = 12;           // three one-wave workgroups on every SIMD: at 168 VGPRs a SIMD holds no more

struct Plan8 {
    int groups = 0;                            // groups of eight work slots
    int items = 0;                             // queue length (ragged batches: empty second halves included)
    int wgs = 0;                               // workgroups launched
    int rounds_x16 = 0;                        // items per workgroup, in sixteenths: the queue's rounds
};

// nch channels in `segments` pieces; host_items >= 0: the host's list of (group of sixteen, piece) items has that many
// entries (ragged batches, gc_capi.hpp) and every one of them becomes two queue items, one per half
inline Plan8 plan_groups_of_eight(int cus, int nch, int segments, int host_items)
{
    Plan8 p;
    if (nch <= 0 || segments <= 0 || cus <= 0) return p;
    p.groups = (nch + PLAN8_SLOTS - 1) / PLAN8_SLOTS;
    p.items = host_items >= 0 ? 2 * host_items : p.groups * segments;
    const int cap = cus * PLAN8_WGS_PER_CU;
    p.wgs = p.items < cap ? p.items : cap;
    p.rounds_x16 = p.wgs > 0 ? (int)(((int64_t)p.items * 16 + p.wgs - 1) / p.wgs) : 0;
    return p;
}

// Round 15: groups whose seams are likely to close slowly are taken from the queue first (uniform batches).  A seam that
// outlives its piece is continued into the next one by a single wave, frame after frame (self_served_seams,
// gc_encode_kernel.hip); started with the launch, that walk runs underneath the other groups' items, started with the last
// round of short items it is what the launch ends on.
//
// Which channels: the reconstruction error of a run obeys the predictor's recurrence, so two runs from different histories
// approach each other at the rate of its poles -- complex poles of z^2 = (c0 z + c1) / 2048 have radius^2 = -c1 / 2048 --
// and only a predictor next to the unit circle keeps them apart for thousands of frames.  tools/gc_slow_seam_table.py
// (LABNOTES round 15, gate 0) holds the closing times of a host model next to the radius: every channel whose seams need more
// than 1024 frames has a predictor with complex poles and -c1 >= PLAN8_SLOW_C1.  A false positive costs nothing (its
// group's items are as long as any, they only run early); a pure tone's seams close at once (it is coded without loss) and
// it is flagged all the same.
#ifndef VGA_PLAN8_SLOW_C1                      // (timing variants only, tools/build_variants.sh: 4096 = no group is ever flagged)
#define VGA_PLAN8_SLOW_C1 2040
#endif
constexpr int PLAN8_SLOW_C1 = VGA_PLAN8_SLOW_C1;   // radius^2 >= 0.996
VGA_PLAN8_HD inline bool plan8_slow_predictor(int c0, int c1)
{
    return -c1 >= PLAN8_SLOW_C1 && (int64_t)c0 * c0 < (int64_t)-8192 * c1;      // (c0 / 2048)^2 + 4 c1 / 2048 < 0: complex poles
}
// ... a channel: any of its eight predictors (coefs16: c0, c1 of predictor 0, of predictor 1, ...)
VGA_PLAN8_HD inline bool plan8_slow_channel(const int16_t *coefs16)
{
    bool slow = false;
    for (int p = 0; p < 8; p++) slow = slow || plan8_slow_predictor(coefs16[2 * p], coefs16[2 * p + 1]);
    return slow;
}
// The order of the groups: order[0 .. S) = the flagged groups, ascending, order[S .. groups8) = the others, ascending.
// Returns S.  (The device builds the same table from the coefficients where they are: gc_self_served_prologue_kernel.)
inline int plan8_slow_order(const unsigned char *flagged, int groups8, int *order)
{
    int s = 0;
    for (int g = 0; g < groups8; g++)
        if (flagged[g]) order[s++] = g;
    int r = s;
    for (int g = 0; g < groups8; g++)
        if (!flagged[g]) order[r++] = g;
    return s;
}

// queue item -> (group of eight, piece).  Piece-major without a host list, else the list's order (biggest first), a host
// item's two halves next to each other.  false: nothing to encode (the half lies behind the batch's last channel).
// order / slow (uniform batches, plan8_slow_order; order == nullptr: none): the first slow x segments items are all pieces
// of the flagged groups, piece-major among them, the rest is the piece-major order over the other groups; with no flagged
// group or with every group flagged the order is the plain one.  Round 16: `segments` is the piece count of the FLAGGED
// groups (they keep the coarse tail, a schedule of their own: gc::plan_encode_tail_pieces_on); the others' count only
// bounds the queue, slow x segments + (groups8 - slow) x theirs, which the caller knows.
VGA_PLAN8_HD inline bool plan8_item(int item, int groups8, int nch, const uint32_t *host_items, const int *order, int slow, int segments,
                                    int &g, int &y)
{
    if (host_items) {
        const uint32_t v = host_items[item >> 1];
        g = 2 * (int)(v & 0xFFFFFu) + (item & 1);
        y = (int)(v >> 20);
    } else if (order && slow > 0 && slow < groups8) {
        const int front = slow * segments;
        if (item < front) {
            g = order[item % slow];
            y = item / slow;
        } else {
            const int rest = groups8 - slow;
            g = order[slow + (item - front) % rest];
            y = (item - front) / rest;
        }
    } else {
        g = item % groups8;
        y = item / groups8;
    }
    return g * PLAN8_SLOTS < nch;
}
VGA_PLAN8_HD inline bool plan8_item(int item, int groups8, int nch, const uint32_t *host_items, int &g, int &y)
{
    return plan8_item(item, groups8, nch, host_items, nullptr, 0, 0, g, y);
}

}  // namespace gc
}  // namespace vga
