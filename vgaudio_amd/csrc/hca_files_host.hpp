// hca_files_host.hpp -- the host side of include/vgaudio_hip/hca_files.h without HIP: every check, the layout of a set of HCA
// files (frame streams, images), the prebuilt headers, the per-file table and the work items the kernels of
// hca_files_kernels.hip read.  A file's size and header bytes are what vga_hca_file_size and vga_hca_file_header say (they
// are CALLED here, not restated, which is why a set refuses a file with the per-file call's own code and message).
// Header-only and free of <hip/hip_runtime.h>, so that a stand-alone host program can include it
// (tests/host/hca_files_host_driver.cpp) as capi_hca_files.hip does; whoever includes it supplies vga::set_error,
// vga::last_error and the two per-file functions.
#pragma once
#include "files_layout.hpp"
#include "../../include/vgaudio_hip/hca_files.h"

namespace vga {
namespace hcaf {

using fileset::name_file;
using fileset::pad_to;
using fileset::MAX_TOTAL;
constexpr int64_t SLACK_BYTES = 8;               // behind the last stream (hca_ragged.h's)
constexpr int SPAN_BYTES = 16384;                // the whole frames of one work item, at most (a frame beyond it goes alone)
constexpr int MAX_SPAN_FRAME = 4096;             // the largest frame of the span form: at least four frames per span

// What the kernels need of one file (a device table, one per file).  src / dst are byte offsets into the call's source and
// destination buffers: d_frames -> d_images + header for a write, d_images -> d_frames for a read.
struct FileTab {
    int64_t src_off, dst_off;
    int64_t image_off;                           // (write) where the header goes
    int frame_size, frame_count;
    int key;                                     // table index, -1: none
    int header_off, header_size;                 // (write) into the header blob
    int item_frames;                             // whole frames per work item
};
struct Item { int file; int first_frame; };

struct FilesLayout {
    vga_hca_files_totals totals = {};
    bool from_infos = false;
    std::vector<int64_t> frame_off, image_off, stream_bytes;   // per file
    std::vector<int> image_size;                 // per file
    std::vector<vga_hca_info> hca;               // (from parsed headers) per file, for the key search (hca_keyed_files_host.hpp)
    std::vector<int> encryption_type;            // (from parsed headers) per file
    std::vector<uint8_t> headers;                // (write) every header, each at a multiple of 16
    std::vector<uint8_t> tables;                 // ntables x 256
    std::vector<FileTab> tab;
    // [0]: every file in its own form, the span items in front; [1]: every file in the general form (the force hook)
    std::vector<Item> items[2];
    int span_items = 0;                          // of items[0]
    int span_files = 0, general_files = 0, moving_files = 0;   // of items[0]; files that move frame bytes at all
};

inline bool span_shape(int frame_size) { return frame_size <= MAX_SPAN_FRAME; }
inline int item_frames_of(int frame_size) { return frame_size > 0 ? std::max(1, SPAN_BYTES / frame_size) : 1; }

inline int check_tables(const uint8_t *tables, int ntables)
{
    if (ntables < 0 || (ntables > 0 && !tables)) { set_error("%d substitution tables at a null pointer", ntables); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}
// with_keys == false: the keys are not looked at (layout and work items do not depend on them)
inline int check_key(int f, int key, int frame_size, int frame_count, int ntables, bool with_keys)
{
    if (!with_keys) return VGA_OK;
    if (key < -1 || key >= ntables) { set_error("file %d: key %d outside -1 .. %d", f, key, ntables - 1); return VGA_ERR_ARGUMENT; }
    if (key >= 0 && frame_count > 0 && (frame_size < 2 || frame_size > 0xFFFF)) {
        set_error("file %d: keyed frames of %d bytes (2 .. 65535)", f, frame_size);
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}

// where file f's stream lies, and that the streams do not overlap; fills frame_off and totals.frame_bytes
inline int place_streams(FilesLayout &L, const int64_t *frame_offsets)
{
    const int nfiles = L.totals.files;
    fileset::Rows streams;
    L.frame_off.resize(nfiles);
    for (int f = 0; f < nfiles; f++) {
        const int64_t room = pad_to(L.stream_bytes[f], 4);
        const fileset::Placed s = streams.place(room, room, MAX_TOTAL, frame_offsets ? frame_offsets + f : nullptr);
        if (s.at < 0 || s.at % 4) { set_error("file %d: frame offset %lld is negative or no multiple of 4", f, (long long)s.at); return VGA_ERR_ARGUMENT; }
        if (s.verdict) { set_error("file %d: the frames of the set exceed 2^62 bytes", f); return VGA_ERR_OUT_OF_RANGE; }
        L.frame_off[f] = s.at;
    }
    int a, b;                                     // a stream takes its bytes rounded up to 4
    if (frame_offsets && fileset::find_overlap(nfiles, [&](int f) { return L.frame_off[f]; }, [&](int f) { return pad_to(L.stream_bytes[f], 4); }, a, b)) {
        set_error("file %d: stream %d (offset %lld, %lld bytes) overlaps stream %d (offset %lld)", std::max(a, b), a,
                  (long long)L.frame_off[a], (long long)L.stream_bytes[a], b, (long long)L.frame_off[b]);
        return VGA_ERR_ARGUMENT;
    }
    L.totals.frame_bytes = streams.end + SLACK_BYTES;
    return VGA_OK;
}

// the items of every file for both tables, the span items in front
inline int cut_items(FilesLayout &L)
{
    std::vector<Item> own_general;
    for (int f = 0; f < L.totals.files; f++) {
        FileTab &t = L.tab[f];
        t.item_frames = item_frames_of(t.frame_size);
        if (L.stream_bytes[f] <= 0) continue;
        const bool span = span_shape(t.frame_size);
        L.moving_files++;
        (span ? L.span_files : L.general_files)++;
        for (int64_t k = 0; k < t.frame_count; k += t.item_frames) {
            const Item it = {f, (int)k};
            (span ? L.items[0] : own_general).push_back(it);
            L.items[1].push_back(it);
        }
    }
    L.span_items = (int)L.items[0].size();
    L.items[0].insert(L.items[0].end(), own_general.begin(), own_general.end());
    return fileset::check_item_count(L.items[1].size());
}

inline void keep_tables(FilesLayout &L, const uint8_t *tables, int ntables)
{
    if (ntables > 0) L.tables.assign(tables, tables + (size_t)ntables * 256);
}

// a set for writing.  with_keys == false: layout and items only (keys unchecked, no tables kept)
inline int make_layout(const vga_hca_file *files, int nfiles, const int64_t *frame_offsets, const uint8_t *tables, int ntables, bool with_keys,
                       FilesLayout &L)
{
    if (int rc = fileset::check_files(nfiles, files != nullptr, "files")) return rc;
    if (with_keys)
        if (int rc = check_tables(tables, ntables)) return rc;
    L = FilesLayout();
    L.totals.files = nfiles;
    L.image_off.resize(nfiles);
    L.image_size.resize(nfiles);
    L.stream_bytes.resize(nfiles);
    L.tab.resize(nfiles);
    fileset::Images images;
    for (int f = 0; f < nfiles; f++) {
        const vga_hca_file &F = files[f];
        const vga_hca_info &H = F.hca;
        FileTab &t = L.tab[f];
        std::memset(&t, 0, sizeof t);
        const int size = vga_hca_file_size(&H);
        if (size < 0) return name_file(f, size);
        const size_t header_at = L.headers.size();
        // (the header call checks the header size before it writes: 8 .. 0x7FFF)
        L.headers.resize(header_at + (size_t)pad_to(std::min(std::max(H.header_size, 0), 0x7FFF), 16));
        if (int rc = vga_hca_file_header(&H, F.comment, F.volume, F.encryption_type, F.encrypted_ids, L.headers.data() + header_at)) return name_file(f, rc);
        if (int rc = check_key(f, F.key, H.frame_size, H.frame_count, ntables, with_keys)) return rc;
        const fileset::Placed image = images.place(size);
        const int64_t image_at = image.at;
        L.stream_bytes[f] = (int64_t)H.frame_size * H.frame_count;
        L.totals.total_frames += H.frame_count;
        L.image_off[f] = image_at;
        L.image_size[f] = size;
        t.image_off = image_at;
        t.dst_off = image_at + H.header_size;
        t.frame_size = H.frame_size;
        t.frame_count = H.frame_count;
        t.key = F.key;
        t.header_off = (int)header_at;
        t.header_size = H.header_size;
        if ((image.verdict & fileset::TOTAL_PAST_MAX) || header_at > 0x7FFFFFFF) { set_error("file %d: the images of the set exceed 2^62 bytes", f); return VGA_ERR_OUT_OF_RANGE; }
    }
    if (int rc = place_streams(L, frame_offsets)) return rc;
    for (int f = 0; f < nfiles; f++) L.tab[f].src_off = L.frame_off[f];
    L.totals.image_bytes = images.total();
    if (with_keys) keep_tables(L, tables, ntables);
    return cut_items(L);
}

// a set for reading, from what vga_hca_parse returned for every file
inline int make_layout_from_infos(const vga_hca_file_info *const *infos, int nfiles, const int64_t *image_offsets, const int *keys,
                                  const uint8_t *tables, int ntables, bool with_keys, const int64_t *frame_offsets, FilesLayout &L)
{
    if (int rc = fileset::check_files(nfiles, infos != nullptr, "infos")) return rc;
    if (with_keys)
        if (int rc = check_tables(tables, ntables)) return rc;
    L = FilesLayout();
    L.from_infos = true;
    L.totals.files = nfiles;
    L.hca.resize(nfiles);
    L.encryption_type.resize(nfiles);
    L.image_off.resize(nfiles);
    L.image_size.resize(nfiles);
    L.stream_bytes.resize(nfiles);
    L.tab.resize(nfiles);
    fileset::Images images;
    for (int f = 0; f < nfiles; f++) {
        const vga_hca_file_info *I = infos[f];
        if (!I) { set_error("file %d: null info", f); return VGA_ERR_ARGUMENT; }
        const vga_hca_info &H = I->hca;
        // (vga_hca_read_device's check)
        if (H.frame_count < 0 || H.frame_size < 8 || H.frame_size > 0xFFFF || I->frames_offset < 0) {
            set_error("file %d: info does not describe an HCA file", f);
            return VGA_ERR_ARGUMENT;
        }
        const int64_t bytes = (int64_t)H.frame_size * H.frame_count, size = I->frames_offset + bytes;
        const fileset::Placed image = images.place(size, image_offsets ? image_offsets + f : nullptr);
        const int64_t at = image.at;
        if (image.verdict & fileset::OFFSET_NEGATIVE) { set_error("file %d: negative image offset %lld", f, (long long)at); return VGA_ERR_ARGUMENT; }
        if (image.verdict & (fileset::IMAGE_PAST_2GIB | fileset::OFFSET_PAST_MAX)) { set_error("file %d: image past 2 GiB or offset past 2^62", f); return VGA_ERR_OUT_OF_RANGE; }
        const int key = keys ? keys[f] : -1;
        if (int rc = check_key(f, key, H.frame_size, H.frame_count, ntables, with_keys)) return rc;
        L.stream_bytes[f] = bytes;
        L.totals.total_frames += H.frame_count;
        L.image_off[f] = at;
        L.image_size[f] = (int)size;
        L.hca[f] = H;
        L.encryption_type[f] = I->encryption_type;
        FileTab &t = L.tab[f];
        std::memset(&t, 0, sizeof t);
        t.image_off = at;
        t.src_off = at + I->frames_offset;
        t.frame_size = H.frame_size;
        t.frame_count = H.frame_count;
        t.key = key;
    }
    if (int rc = place_streams(L, frame_offsets)) return rc;
    for (int f = 0; f < nfiles; f++) L.tab[f].dst_off = L.frame_off[f];
    L.totals.image_bytes = images.total();
    if (with_keys) keep_tables(L, tables, ntables);
    return cut_items(L);
}

// ---- the work items as the public accessor describes them: what the kernels compute from FileTab and Item
inline void describe_items(const FilesLayout &L, bool general, std::vector<vga_hca_files_item> &out)
{
    const std::vector<Item> &items = L.items[general ? 1 : 0];
    const int span_items = general ? 0 : L.span_items;
    if (!L.from_infos)
        for (int f = 0; f < L.totals.files; f++) out.push_back({VGA_HCA_FILES_HEADER, f, 0, 0, 0, L.tab[f].header_size});
    for (size_t i = 0; i < items.size(); i++) {
        const Item it = items[i];
        const FileTab &t = L.tab[it.file];
        const int n = std::min(t.item_frames, t.frame_count - it.first_frame);
        const int64_t base = L.from_infos ? 0 : t.header_size;
        vga_hca_files_item d = {(int)i < span_items ? VGA_HCA_FILES_SPAN : VGA_HCA_FILES_GENERAL, it.file, it.first_frame, n,
                                base + (int64_t)it.first_frame * t.frame_size, base + (int64_t)(it.first_frame + n) * t.frame_size};
        if (L.from_infos && it.first_frame + n == t.frame_count) d.end = pad_to(d.end, 4);     // the rounding zeros
        out.push_back(d);
    }
}

inline bool aligned_to(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// ---- the calls' argument checks
inline int check_write(const FilesLayout &L, const void *d_frames, const void *d_images)
{
    const char *what = "vga_hca_write_device_v";
    if (L.from_infos) { set_error("%s: the set was made from parsed headers (vga_hca_files_create_from_infos): it serves the read call", what); return VGA_ERR_INVALID_OP; }
    if (!d_images || (!d_frames && L.moving_files > 0)) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (!aligned_to(d_frames, 4) || !aligned_to(d_images, 16)) { set_error("%s: d_frames needs 4-byte and d_images 16-byte alignment", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}
inline int check_read(const FilesLayout &L, const void *d_images, const void *d_frames, const char *what = "vga_hca_read_device_v")
{
    if (!L.from_infos) { set_error("%s: the set was not made from parsed headers (vga_hca_files_create_from_infos)", what); return VGA_ERR_INVALID_OP; }
    if ((!d_images || !d_frames) && L.moving_files > 0) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (!aligned_to(d_frames, 4) || !aligned_to(d_images, 16)) { set_error("%s: d_frames needs 4-byte and d_images 16-byte alignment", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

}  // namespace hcaf
}  // namespace vga
