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

// queue item -> (group of eight, piece).  Piece-major without a host list, else the list's order (biggest first), a host
// item's two halves next to each other.  false: nothing to encode (the half lies behind the batch's last channel).
VGA_PLAN8_HD inline bool plan8_item(int item, int groups8, int nch, const uint32_t *host_items, int &g, int &y)
{
    if (host_items) {
        const uint32_t v = host_items[item >> 1];
        g = 2 * (int)(v & 0xFFFFFu) + (item & 1);
        y = (int)(v >> 20);
    } else {
        g = item % groups8;
        y = item / groups8;
    }
    return g * PLAN8_SLOTS < nch;
}

}  // namespace gc
}  // namespace vga
