// adx_files_host.hpp -- the host side of include/vgaudio_hip/adx_files.h without HIP: every check, the packed layout of a set
// of ADX files (rows, images), the per-file table and the work items the kernels of adx_files_kernels.hip read.  File f of a
// set is what adx_file_host.hpp (vga_adx_file_layout_for's and vga_adx_write_device's code) says for the file's params.
// Header-only and free of <hip/hip_runtime.h>, so that a stand-alone host program can include it
// (tests/host/adx_files_host_driver.cpp) as capi_adx_files.hip does; whoever includes it supplies vga::set_error and
// vga::last_error.
#pragma once
#include "files_layout.hpp"
#include "adx_file_host.hpp"
#include "adx_span.hpp"
#include "../../include/vgaudio_hip/adx_files.h"

namespace vga {
namespace adxf {

using fileset::aligned16;
using fileset::name_file;
using fileset::pad_to;
using fileset::MAX_TOTAL;
constexpr int64_t GUARD_BYTES = fileset::IMAGE_GUARD_BYTES;   // behind the last row as behind the last image
constexpr int CHUNK_GRANULES = 2048;             // of one general work item: 256 threads, eight granules each
// keyed calls (include/vgaudio_hip_files/adx_keyed_files.h): a slot is frame * channels + channel, the cipher's own order
constexpr int CIPHER_CHUNK_SLOTS = 2048;         // of one item of the general form's cipher pass: 256 threads, eight slots each
constexpr int FIND_SPAN_SLOTS = 1024;            // of one item of the key search: 256 lanes = 64 candidates x 4 quarters

// What the kernels need of one file (a device table, one per file).  A set for reading fills h.nch and h.frame_size only.
struct FileTab {
    container::AdxHeaderArgs h;
    int64_t image_off;
    int first_channel, audio_offset;
    int copy_frames;                             // frames per channel the audio kernels move: min(rows hold, asked) / frame_count
    int span_frames;                             // > 0: the file qualifies for the span form, with spans of this many frames
    int granule;                                 // of the general form: 16, 8, 4, 2 or 1 bytes
    int header_end;                              // (write) the header kernel's bytes: max(audio offset, end of the fields)
};
struct Item { int x; uint32_t y; };              // SPAN: file, first frame; GENERAL: file (write) / row (read), chunk

struct FilesLayout {
    vga_adx_files_totals totals = {};
    bool from_infos = false, any_v4 = false;
    std::vector<vga_adx_file_layout> layout;     // per file (a set for writing)
    std::vector<int> first_channel, image_size;  // per file
    std::vector<int64_t> image_off;              // per file
    std::vector<int64_t> row_off;                // per row
    std::vector<int> row_bytes, row_file;        // per row
    std::vector<int16_t> history;                // per row (from_infos)
    std::vector<FileTab> tab;
    // [0]: every file in its own form, the span items in front; [1]: every file in the general form (the force hook)
    std::vector<Item> items[2];
    int span_items = 0;                          // of items[0]
    int span_files = 0, general_files = 0, moving_files = 0;   // of items[0]; files that move audio at all
    // keyed calls: (file, chunk of CIPHER_CHUNK_SLOTS slots) of the files items[k] serves in the general form;
    // (file, span of FIND_SPAN_SLOTS slots) of every file of a set for reading
    std::vector<Item> cipher_items[2], find_items;
    bool tiny_frame = false;                     // a file of 1-byte frames (a set for reading): no scale to cipher
};

// the widest power of two up to 16 that divides every bit set in `bits`
inline int granule_of(uint64_t bits)
{
    for (int g = 16; g > 1; g >>= 1)
        if (!(bits & (uint64_t)(g - 1))) return g;
    return 1;
}

inline bool span_shape(int frame_size, int nch) { return frame_size == adxspan::kFrame && nch <= adxspan::kMaxChannels; }

// items of file f (every row of it, when reading) for both tables
inline void cut_items(FilesLayout &L, int f, bool span_ok)
{
    FileTab &t = L.tab[f];
    const int nch = t.h.nch, fs = t.h.frame_size;
    if (t.copy_frames <= 0) return;
    L.moving_files++;
    // write: chunks of the file's interleaved bytes; read: chunks of every row
    fileset::cut_general_items(L.items, span_ok, L.from_infos ? t.first_channel : f, L.from_infos ? nch : 1,
                               (int64_t)t.copy_frames * fs * (L.from_infos ? 1 : nch), (int64_t)CHUNK_GRANULES * t.granule);
    const int64_t slots = (int64_t)t.copy_frames * nch;
    for (int k = 0; k < 2; k++)
        for (int64_t at = 0, y = 0; at < slots && !(k == 0 && span_ok); at += CIPHER_CHUNK_SLOTS, y++) L.cipher_items[k].push_back({f, (uint32_t)y});
    for (int64_t at = 0, y = 0; at < slots && L.from_infos; at += FIND_SPAN_SLOTS, y++) L.find_items.push_back({f, (uint32_t)y});
    if (span_ok) {
        t.span_frames = adxspan::span_frames(nch);
        L.span_files++;
    } else {
        L.general_files++;
    }
}
// the span items go in front (they are one launch, the general items the next)
inline void finish_items(FilesLayout &L)
{
    std::vector<Item> span;
    for (size_t f = 0; f < L.tab.size(); f++)
        for (int k0 = 0; L.tab[f].span_frames > 0 && k0 < L.tab[f].copy_frames; k0 += L.tab[f].span_frames) span.push_back({(int)f, (uint32_t)k0});
    L.span_items = fileset::put_in_front(L.items[0], span);
}

inline int check_item_counts(const FilesLayout &L)
{
    return fileset::check_item_count(std::max({L.items[0].size(), L.items[1].size(), L.cipher_items[1].size(), L.find_items.size()}));
}

inline int make_layout(const vga_adx_file *files, int nfiles, const int64_t *audio_offsets, FilesLayout &L)
{
    if (int rc = fileset::check_files(nfiles, files != nullptr, "files")) return rc;
    fileset::start_layout(L, nfiles, false);
    L.layout.resize(nfiles);
    int64_t channels = 0;
    fileset::Rows rows;
    fileset::Images images;
    for (int f = 0; f < nfiles; f++) {
        const vga_adx_file &F = files[f];
        const vga_adx_file_params &p = F.params;
        FileTab &t = L.tab[f];
        std::memset(&t, 0, sizeof t);
        // the rows hold CriAdxFormat.SampleCount samples: ceil(sample_count / spf) frames (a bad frame size is refused below)
        const int spf = (p.frame_size - 2) * 2;
        const int64_t in_frames = p.frame_size >= 3 && p.sample_count > 0 ? ((int64_t)p.sample_count + spf - 1) / spf : 0;
        const int64_t row = in_frames * p.frame_size;
        if (int rc = container::adx_args(&p, F.channels, (int)std::min<int64_t>(row, 0x7FFFFFFF), &L.layout[f], &t.h)) return name_file(f, rc);
        if (row > 0x7FFFFFFF) { set_error("file %d: a row of the file would exceed 2 GiB", f); return VGA_ERR_OUT_OF_RANGE; }
        // The one refusal a set adds to the per-file call's: the footer's four bytes must fit too (3-byte frames without a
        // loop leave it 3).  The reference throws there as it does for the header (the MemoryStream is not expandable);
        // vga_adx_write_device drops the fourth byte instead, and keeps doing so.
        if (t.h.footer_pos + 4 > t.h.file_size) {
            set_error("file %d: ADX footer (4 bytes at %d) does not fit the %d-byte file", f, t.h.footer_pos, t.h.file_size);
            return VGA_ERR_INVALID_OP;
        }
        const int first = (int)channels;
        if (int rc = fileset::count_rows(f, F.channels, channels, "rows")) return rc;
        const vga_adx_file_layout &A = L.layout[f];
        L.any_v4 = L.any_v4 || p.version == 4;
        L.first_channel[f] = first;
        uint64_t bits = 0;
        for (int i = 0; i < F.channels; i++) {
            const fileset::Placed r = rows.place(row, pad_to(row, 16), MAX_TOTAL, audio_offsets ? audio_offsets + first + i : nullptr);
            const int64_t at = r.at;
            if (at < 0 || at % 4) { set_error("file %d: audio offset %lld of row %lld is negative or no multiple of 4", f, (long long)at, (long long)(first + i)); return VGA_ERR_ARGUMENT; }
            if (r.verdict & fileset::OFFSET_PAST_MAX) { set_error("file %d: the rows of the set exceed 2^62 bytes", f); return VGA_ERR_OUT_OF_RANGE; }
            L.row_off.push_back(at);
            L.row_bytes.push_back((int)row);
            L.row_file.push_back(f);
            if (row > 0) bits |= (uint64_t)at;
        }
        const fileset::Placed image = images.place(A.file_size);
        const int64_t image_at = image.at;
        t.image_off = image_at;
        t.first_channel = first;
        t.audio_offset = A.audio_offset;
        t.copy_frames = (int)std::min<int64_t>(in_frames, A.frame_count);
        t.header_end = std::max(A.audio_offset, container::adx_header_fields_end(p.version, F.channels));
        // a mono file is a plain copy: the frame size does not enter its granule
        t.granule = granule_of(bits | (uint64_t)(image_at + A.audio_offset) | (F.channels > 1 ? (uint64_t)p.frame_size : 0));
        cut_items(L, f, span_shape(p.frame_size, F.channels) && !(bits & 15));
        L.image_off[f] = image_at;
        L.image_size[f] = A.file_size;
        if (image.verdict & fileset::TOTAL_PAST_MAX) { set_error("file %d: the images of the set exceed 2^62 bytes", f); return VGA_ERR_OUT_OF_RANGE; }
    }
    int a, b;                                     // rows of bytes must not overlap
    if (audio_offsets && fileset::find_overlap((int)channels, [&](int c) { return L.row_off[c]; }, [&](int c) { return L.row_bytes[c]; }, a, b)) {
        set_error("file %d: row %d (offset %lld, %d bytes) overlaps row %d (offset %lld)", L.row_file[std::max(a, b)], a,
                  (long long)L.row_off[a], L.row_bytes[a], b, (long long)L.row_off[b]);
        return VGA_ERR_ARGUMENT;
    }
    finish_items(L);
    L.totals.channels = (int)channels;
    L.totals.audio_bytes = rows.end + GUARD_BYTES;
    L.totals.image_bytes = images.total();
    return check_item_counts(L);
}

// a set for reading, from what vga_adx_parse returned for every file
inline int make_layout_from_infos(const vga_adx_file_info *const *infos, int nfiles, const int64_t *image_offsets, FilesLayout &L)
{
    if (int rc = fileset::check_files(nfiles, infos != nullptr, "infos")) return rc;
    fileset::start_layout(L, nfiles, true);
    int64_t channels = 0;
    fileset::Rows rows;
    fileset::Images images;
    for (int f = 0; f < nfiles; f++) {
        const vga_adx_file_info *I = infos[f];
        if (!I) { set_error("file %d: null info", f); return VGA_ERR_ARGUMENT; }
        const int nch = I->channel_count, fs = I->frame_size;
        // (vga_adx_read_device's check)
        if (nch < 1 || nch > 255 || fs < 1 || I->frame_count < 0 || I->audio_bytes != (int64_t)I->frame_count * fs || I->audio_offset < 0) {
            set_error("file %d: info does not describe an ADX file", f);
            return VGA_ERR_ARGUMENT;
        }
        const int64_t size = (int64_t)I->audio_offset + (int64_t)I->audio_bytes * nch;
        const fileset::Placed image = images.place(size, image_offsets ? image_offsets + f : nullptr);
        const int64_t at = image.at;
        if (image.verdict & fileset::OFFSET_NEGATIVE) { set_error("file %d: negative image offset %lld", f, (long long)at); return VGA_ERR_ARGUMENT; }
        if (image.verdict & (fileset::IMAGE_PAST_2GIB | fileset::OFFSET_PAST_MAX)) { set_error("file %d: image past 2 GiB or offset past 2^62", f); return VGA_ERR_OUT_OF_RANGE; }
        const int first = (int)channels;
        if (int rc = fileset::count_rows(f, nch, channels, "rows")) return rc;
        L.first_channel[f] = first;
        L.image_off[f] = at;
        L.image_size[f] = (int)size;
        for (int i = 0; i < nch; i++) {
            L.row_off.push_back(rows.place(I->audio_bytes, pad_to(I->audio_bytes, 16), MAX_TOTAL).at);
            L.row_bytes.push_back(I->audio_bytes);
            L.row_file.push_back(f);
            L.history.push_back(I->history[i][0]);
        }
        if (rows.at > MAX_TOTAL) { set_error("file %d: the rows of the set exceed 2^62 bytes", f); return VGA_ERR_OUT_OF_RANGE; }
        FileTab &t = L.tab[f];
        std::memset(&t, 0, sizeof t);
        t.h.nch = nch;
        t.h.frame_size = fs;
        t.h.encryption_type = I->revision;                      // the file's own type (the keyed calls)
        L.tiny_frame = L.tiny_frame || fs < 2;
        t.image_off = at;
        t.first_channel = first;
        t.audio_offset = I->audio_offset;
        t.copy_frames = I->frame_count;
        t.granule = granule_of((uint64_t)(at + I->audio_offset) | (nch > 1 ? (uint64_t)fs : 0));   // the rows are on 16
        cut_items(L, f, span_shape(fs, nch));
    }
    finish_items(L);
    L.totals.channels = (int)channels;
    L.totals.audio_bytes = rows.end + GUARD_BYTES;
    L.totals.image_bytes = images.total();
    return check_item_counts(L);
}

// ---- the work items as the public accessor describes them: what the kernels compute from FileTab and Item
inline void describe_items(const FilesLayout &L, bool general, std::vector<vga_adx_files_item> &out)
{
    const int nfiles = L.totals.files;
    const std::vector<Item> &items = L.items[general ? 1 : 0];
    const int span_items = general ? 0 : L.span_items;
    if (!L.from_infos)
        for (int f = 0; f < nfiles; f++) out.push_back({VGA_ADX_FILES_HEADER, f, f, 0, 0, 0, L.tab[f].header_end, 0});
    for (size_t i = 0; i < items.size(); i++) {
        const Item it = items[i];
        const bool span = (int)i < span_items;
        const int f = span || !L.from_infos ? it.x : L.row_file[it.x];
        const FileTab &t = L.tab[f];
        const int64_t group = (int64_t)t.h.frame_size * (L.from_infos ? 1 : t.h.nch);   // bytes of one frame in the item's space
        const int64_t base = L.from_infos ? 0 : t.audio_offset, total = group * t.copy_frames;
        vga_adx_files_item d = {span ? VGA_ADX_FILES_SPAN : VGA_ADX_FILES_GENERAL, f, it.x, it.y, span ? 0 : t.granule, 0, 0, 0};
        if (span) {
            d.begin = base + group * it.y;
            d.end = base + group * std::min<int64_t>((int64_t)it.y + t.span_frames, t.copy_frames);
        } else {
            const int64_t unit = (int64_t)CHUNK_GRANULES * t.granule;
            d.begin = base + unit * it.y;
            d.end = base + std::min(unit * ((int64_t)it.y + 1), total);
        }
        out.push_back(d);
    }
    if (!L.from_infos)
        for (int f = 0; f < nfiles; f++)
            out.push_back({VGA_ADX_FILES_FOOTER, f, f, 0, 0, L.tab[f].h.footer_pos, L.tab[f].h.file_size, L.tab[f].header_end});
}

// ---- the calls' argument checks
inline int check_write(const FilesLayout &L, const void *d_audio, const void *d_history, const void *d_images)
{
    const char *what = "vga_adx_write_device_v";
    if (L.from_infos) { set_error("%s: the set was made from parsed headers (vga_adx_files_create_from_infos): it serves the read call", what); return VGA_ERR_INVALID_OP; }
    if (!d_images || (!d_audio && L.moving_files > 0)) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (L.any_v4 && !d_history) { set_error("%s: version 4 headers carry the channel histories", what); return VGA_ERR_ARGUMENT; }
    if (!aligned16(d_audio) || !aligned16(d_images)) { set_error("%s: d_audio and d_images need 16-byte alignment", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}
inline int check_read(const FilesLayout &L, const void *d_images, const void *d_audio)
{
    const char *what = "vga_adx_read_device_v";
    if (!L.from_infos) { set_error("%s: the set was not made from parsed headers (vga_adx_files_create_from_infos)", what); return VGA_ERR_INVALID_OP; }
    if ((!d_images || !d_audio) && L.moving_files > 0) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (!aligned16(d_audio) || !aligned16(d_images)) { set_error("%s: d_audio and d_images need 16-byte alignment", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

}  // namespace adxf
}  // namespace vga
