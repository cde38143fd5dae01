// adx_keyed_files_host.hpp -- the host side of include/vgaudio_hip_files/adx_keyed_files.h without HIP: the argument checks of
// the three keyed calls, the size and shape of the search's workspace, and the search's work items as the public hook
// describes them.  The items themselves are cut with the set's other tables (adx_files_host.hpp).  Header-only and free of
// <hip/hip_runtime.h> (tests/host/adx_keyed_files_host_driver.cpp includes it as capi_adx_keyed_files.hip does).
#pragma once
#include "adx_files_host.hpp"
#include "../../include/vgaudio_hip_files/adx_keyed_files.h"

namespace vga {
namespace adxk {

// The workspace: one "still possible" bit per (file, candidate), bit i of a file's words = d_keys[i]; a file's words follow
// each other, files in order.
inline int64_t find_words_per_file(int nkeys8, int nkeys9) { return ((int64_t)nkeys8 + nkeys9 + 31) / 32; }
inline int64_t find_workspace_bytes(const adxf::FilesLayout &L, int nkeys8, int nkeys9)
{
    if (!L.from_infos || nkeys8 < 0 || nkeys9 < 0) return 0;
    return (int64_t)L.totals.files * find_words_per_file(nkeys8, nkeys9) * 4;
}

inline void describe_find_items(const adxf::FilesLayout &L, std::vector<vga_adx_find_keys_item> &out)
{
    for (const adxf::Item &it : L.find_items) {
        const adxf::FileTab &t = L.tab[it.x];
        const int64_t slots = (int64_t)t.copy_frames * t.h.nch, first = (int64_t)it.y * adxf::FIND_SPAN_SLOTS;
        out.push_back({it.x, (int)first, (int)std::min<int64_t>(adxf::FIND_SPAN_SLOTS, slots - first)});
    }
}

inline int check_keys(const char *what, const void *d_keys, int nkeys)
{
    if (nkeys <= 0) { set_error("%s: %d keys: a keyed call needs at least one", what, nkeys); return VGA_ERR_ARGUMENT; }
    if (!d_keys) { set_error("%s: null d_keys", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

inline int check_keyed_write(const adxf::FilesLayout &L, const void *d_audio, const void *d_history, const void *d_keys, int nkeys,
                             const void *d_images)
{
    const char *what = "vga_adx_write_keyed_device_v";
    if (L.from_infos) { set_error("%s: the set was made from parsed headers (vga_adx_files_create_from_infos): it serves the read calls", what); return VGA_ERR_INVALID_OP; }
    if (int rc = check_keys(what, d_keys, nkeys)) return rc;
    if (!d_images || (!d_audio && L.moving_files > 0)) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (L.any_v4 && !d_history) { set_error("%s: version 4 headers carry the channel histories", what); return VGA_ERR_ARGUMENT; }
    if (!adxf::aligned16(d_audio) || !adxf::aligned16(d_images)) { set_error("%s: d_audio and d_images need 16-byte alignment", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

inline int check_read_set(const adxf::FilesLayout &L, const char *what)
{
    if (!L.from_infos) { set_error("%s: the set was not made from parsed headers (vga_adx_files_create_from_infos)", what); return VGA_ERR_INVALID_OP; }
    if (L.tiny_frame) { set_error("%s: a file of the set has 1-byte frames: no scale to cipher", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

inline int check_keyed_read(const adxf::FilesLayout &L, const void *d_images, const void *d_keys, int nkeys, const void *d_audio)
{
    const char *what = "vga_adx_read_keyed_device_v";
    if (int rc = check_read_set(L, what)) return rc;
    if (int rc = check_keys(what, d_keys, nkeys)) return rc;
    if ((!d_images || !d_audio) && L.moving_files > 0) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (!adxf::aligned16(d_audio) || !adxf::aligned16(d_images)) { set_error("%s: d_audio and d_images need 16-byte alignment", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

inline int check_find(const adxf::FilesLayout &L, const void *d_images, const void *d_keys, int nkeys8, int nkeys9,
                      const void *d_key_index_out, const void *d_workspace, uint64_t workspace_bytes)
{
    const char *what = "vga_adx_find_keys_device_v";
    if (int rc = check_read_set(L, what)) return rc;
    if (nkeys8 < 0 || nkeys9 < 0) { set_error("%s: negative candidate count (%d, %d)", what, nkeys8, nkeys9); return VGA_ERR_ARGUMENT; }
    if ((int64_t)nkeys8 + nkeys9 > 0x7FFFFFFF) { set_error("%s: more than 2^31 candidates", what); return VGA_ERR_ARGUMENT; }
    if (nkeys8 + nkeys9 > 0 && !d_keys) { set_error("%s: null d_keys", what); return VGA_ERR_ARGUMENT; }
    if (!d_key_index_out) { set_error("%s: null d_key_index_out", what); return VGA_ERR_ARGUMENT; }
    if (!d_images && L.moving_files > 0) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (!adxf::aligned16(d_images)) { set_error("%s: d_images needs 16-byte alignment", what); return VGA_ERR_ARGUMENT; }
    const int64_t need = find_workspace_bytes(L, nkeys8, nkeys9);
    if (need > 0 && (!d_workspace || workspace_bytes < (uint64_t)need || ((uintptr_t)d_workspace & 3))) {
        set_error("%s: the workspace needs %lld bytes at an int boundary (vga_adx_find_keys_workspace_bytes), %llu given", what, (long long)need,
                  d_workspace ? (unsigned long long)workspace_bytes : 0ull);
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}

}  // namespace adxk
}  // namespace vga
