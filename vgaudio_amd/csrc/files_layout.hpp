// files_layout.hpp -- what the *_files_host.hpp headers share below the object: where the images and the rows of
// a set of files lie, the running counts, the overlap check of caller-placed ranges and the cut of the general work items.
// Arithmetic and classification only: a step returns where the thing lies and a verdict, and the format's header picks its own
// message from the verdict.  Header-only and free of <hip/hip_runtime.h>; whoever includes it supplies vga::set_error and
// vga::last_error.  The parts of the GC-ADPCM family lie in gc_files_layout.hpp.
#pragma once
#include "../../include/vgaudio_hip.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace vga {

void set_error(const char *fmt, ...);            // (common.hpp)
const char *last_error();                        // the message of the last set_error on this thread

namespace fileset {

constexpr int64_t IMAGE_GUARD_BYTES = 256;       // behind the last image
constexpr int64_t MAX_TOTAL = (int64_t)1 << 62;  // of the bytes of a buffer, and of an offset into it
constexpr int64_t MAX_COUNT = 0x7FFFFFFF;        // of channels, rows, work items, and of the bytes of one image

inline int64_t pad_to(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// "file <f>: " in front of the message the per-file code left
inline int name_file(int f, int rc)
{
    const std::string msg = last_error();
    set_error("file %d: %s", f, msg.c_str());
    return rc;
}

// how a layout opens; `array` names the array of the files as the caller knows it
inline int check_files(int nfiles, bool have_array, const char *array)
{
    if (nfiles < 0) { set_error("negative file count"); return VGA_ERR_ARGUMENT; }
    if (nfiles > 0 && !have_array) { set_error("null %s", array); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

// a fresh layout of nfiles files with the per-file arrays most sets keep
template <class Layout> inline void start_layout(Layout &L, int nfiles, bool from_infos)
{
    L = Layout();
    L.from_infos = from_infos;
    L.totals.files = nfiles;
    L.first_channel.resize(nfiles);
    L.image_off.resize(nfiles);
    L.image_size.resize(nfiles);
    L.tab.resize(nfiles);
}

// the running count of channels or rows (`what`) of a set, file f adding n: a set holds fewer than 2^31
inline int count_rows(int f, int n, int64_t &count, const char *what)
{
    if (count + n > MAX_COUNT) { set_error("file %d: more than 2^31 %s", f, what); return VGA_ERR_ARGUMENT; }
    count += n;
    return VGA_OK;
}
inline int check_item_count(size_t items)
{
    if (items > (size_t)MAX_COUNT) { set_error("the set has more than 2^31 work items"); return VGA_ERR_OUT_OF_RANGE; }
    return VGA_OK;
}

// ---- what a placement step says of the thing it placed (bits: more than one may hold, the caller's order of checks decides)
enum : unsigned {
    OFFSET_NEGATIVE = 1,                         // the caller's offset
    OFFSET_PAST_MAX = 2,                         // where it lies is past the limit
    IMAGE_PAST_2GIB = 4,                         // its size
    TOTAL_PAST_MAX = 8,                          // where the next one would lie is past the limit
};
struct Placed {
    int64_t at;
    unsigned verdict;
};

// The images of a set, one after the other on multiples of 16, or where the caller's offsets say: the next image lies behind
// the one placed last either way.
struct Images {
    int64_t at = 0, end = 0;                     // of the next packed image; behind the farthest image so far
    Placed place(int64_t size, const int64_t *offset = nullptr)
    {
        const int64_t here = offset ? *offset : at;
        at = pad_to(here + size, 16);
        end = std::max(end, at);
        return {here, (here < 0 ? OFFSET_NEGATIVE : 0u) | (here > MAX_TOTAL ? OFFSET_PAST_MAX : 0u) | (size > MAX_COUNT ? IMAGE_PAST_2GIB : 0u) |
                          (at > MAX_TOTAL ? TOTAL_PAST_MAX : 0u)};
    }
    int64_t total() const { return end + IMAGE_GUARD_BYTES; }
};

// The rows of a set in the caller's unit (samples, bytes): packed with `room` for each, or at the caller's offsets, where only
// a row that holds something counts towards the end.
struct Rows {
    int64_t at = 0, end = 0;                     // of the next packed row; behind the farthest row so far
    Placed place(int64_t length, int64_t room, int64_t limit, const int64_t *offset = nullptr)
    {
        const int64_t here = offset ? *offset : at;
        if (!offset) end = at += room;
        else if (length > 0) end = std::max(end, here + length);
        return {here, (here < 0 ? OFFSET_NEGATIVE : 0u) | (here > limit ? OFFSET_PAST_MAX : 0u) | (at > limit ? TOTAL_PAST_MAX : 0u)};
    }
};

// Ranges [off(i), off(i) + len(i)) of i < n, those of len(i) > 0 only, must not overlap.  True, and the pair (a lies in front
// of b; equal offsets in the order of the indices), for the first two in that order that do.
template <class Off, class Len> inline bool find_overlap(int n, Off off, Len len, int &a, int &b)
{
    std::vector<int> order;
    for (int i = 0; i < n; i++)
        if (len(i) > 0) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](int x, int y) { return off(x) != off(y) ? off(x) < off(y) : x < y; });
    for (size_t i = 1; i < order.size(); i++) {
        a = order[i - 1];
        b = order[i];
        if (off(a) + len(a) > off(b)) return true;
    }
    return false;
}

// ---- work items of the sets whose files take a fast form or the general one (WAVE, ADX, NW-PCM): table [0] holds every file
// in its own form, table [1] every file in the general form.  The general items of one file: `count` owners from `first`, `per`
// bytes each in chunks of `unit`; a file in its fast form has none in table [0].
template <class Item> inline void cut_general_items(std::vector<Item> (&items)[2], bool fast, int first, int count, int64_t per, int64_t unit)
{
    for (int k = fast ? 1 : 0; k < 2; k++)
        for (int i = 0; i < count; i++)
            for (int64_t at = 0, y = 0; at < per; at += unit, y++) items[k].push_back({first + i, (uint32_t)y});
}
// the fast items go in front (they are one launch, the general items the next); returns their count
template <class Item> inline int put_in_front(std::vector<Item> &items, const std::vector<Item> &fast)
{
    items.insert(items.begin(), fast.begin(), fast.end());
    return (int)fast.size();
}

// ---- the regions a set's items write (the testing hooks): the count always, the regions when there is room for them
template <class Region> inline int copy_regions(const std::vector<Region> &r, Region *regions_out, int64_t capacity, int64_t *count_out)
{
    if (!count_out) { set_error("null count"); return VGA_ERR_ARGUMENT; }
    *count_out = (int64_t)r.size();
    if (!regions_out) return VGA_OK;
    if ((int64_t)r.size() > capacity) { set_error("%lld regions: capacity %lld", (long long)r.size(), (long long)capacity); return VGA_ERR_ARGUMENT; }
    std::copy(r.begin(), r.end(), regions_out);
    return VGA_OK;
}

}  // namespace fileset
}  // namespace vga
