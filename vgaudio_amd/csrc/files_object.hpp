// files_object.hpp -- what the "set of files on the device" objects of the capi_*_files.hip files share on the host
// (DESIGN.md 4.6n): the block of tables a set uploads at create, the null / device check of a call, the create protocol
// and the capped copy of the work-item hooks.  Layouts, consistency checks, launches and stats stay with each file.
#pragma once
#include "common.hpp"
#include "files_table_pack.hpp"

#include <algorithm>

namespace vga {
namespace fileset {

// The tables of a set in device memory: one allocation, one copy.  The caller has run require_device() and recorded the
// current device in `device` (before it builds a ragged batch of its own).
struct TableBlock {
    void *d_tables = nullptr;
    size_t table_bytes = 0;
    int device = 0;
    TableBlock() = default;
    TableBlock(const TableBlock &) = delete;
    TableBlock &operator=(const TableBlock &) = delete;
    ~TableBlock()
    {
        if (d_tables) (void)hipFree(d_tables);
    }
    // every byte of the allocation is written, pad and slack included (a poisoned allocation keeps none of its poison)
    int upload(const std::vector<unsigned char> &host)
    {
        VGA_HIP_TRY(device_malloc(&d_tables, host.size()));
        VGA_HIP_TRY(hipMemcpy(d_tables, host.data(), host.size(), hipMemcpyHostToDevice));
        table_bytes = host.size();
        return VGA_OK;
    }
    int upload(const TablePack &pack) { return upload(pack.image()); }
};

// null object, or made on another device than the current one: VGA_ERR_ARGUMENT, `what` in front of the message
inline int check_object(int files_in_set, int device_of_set, bool is_null, const char *what, const char *type_name)
{
    if (is_null) { set_error("%s: null %s", what, type_name); return VGA_ERR_ARGUMENT; }
    int device = -1;
    if (files_in_set > 0) (void)hipGetDevice(&device);
    if (files_in_set > 0 && device != device_of_set) {
        set_error("%s: the set was created on device %d, the current one is %d", what, device_of_set, device);
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}
// the same of a set object: S::type_name, S::files() and its TableBlock `block`
template <class S> int check_object(const S *s, const char *what)
{
    return check_object(s ? s->files() : 0, s ? s->block.device : 0, !s, what, S::type_name);
}

// a create call: make(s->L) lays the set out, finish(s) uploads it; on any failure nothing is left and *out is null
template <class S, class Make, class Finish> int create_with(S **out, Make &&make, Finish &&finish)
{
    if (!out) { set_error("null output"); return VGA_ERR_ARGUMENT; }
    *out = nullptr;
    S *s = new S;
    int rc = make(s->L);
    if (!rc) rc = finish(s);
    if (rc) {
        delete s;
        return rc;
    }
    *out = s;
    return VGA_OK;
}

// the tail of an _items_for hook: the count, then the items when there is room for them
template <class Item> int copy_capped(const std::vector<Item> &v, Item *out, int64_t capacity, int64_t *count_out)
{
    if (count_out) *count_out = (int64_t)v.size();
    if (!out) return VGA_OK;
    if ((int64_t)v.size() > capacity) { set_error("%lld work items, room for %lld", (long long)v.size(), (long long)capacity); return VGA_ERR_ARGUMENT; }
    std::copy(v.begin(), v.end(), out);
    return VGA_OK;
}

}  // namespace fileset
}  // namespace vga
