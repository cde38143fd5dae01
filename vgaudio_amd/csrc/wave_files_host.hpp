// wave_files_host.hpp -- the host side of include/vgaudio_hip_files/wave_files.h without HIP: every check, the packed layout
// of a set of WAVE files (rows, images), the per-file table, the headers and the work items the kernels of
// wave_files_kernels.hip read.  File f of a set is what wave_file_host.hpp (the per-file calls' code) says for it.
// Header-only and free of <hip/hip_runtime.h>, so that a stand-alone host program can include it
// (tests/host/wave_files_host_driver.cpp) as capi_wave_files.hip does; whoever includes it supplies vga::set_error and
// vga::last_error.
#pragma once
#include "files_layout.hpp"
#include "wave_file_host.hpp"
#include "../../include/vgaudio_hip_files/wave_files.h"

namespace vga {
namespace wavf {

using fileset::name_file;
using fileset::pad_to;
constexpr int64_t GUARD_SAMPLES = 128;           // behind the last row
constexpr int ROW_ROUND = 8;                     // samples a packed row is rounded up to
constexpr int SPAN_BYTES = 16384;                // interleaved bytes of one tile item, at most
constexpr int MAX_TILE_FRAME = VGA_WAVE_FILES_MAX_TILE_FRAME;   // 8 frames fit a span
constexpr int CHUNK_GRANULES = 2048;             // of one general work item: 256 threads, eight granules each
constexpr int GRANULE_BYTES = 16;                // read: 8 samples of a row; write: 16 bytes of the data chunk
constexpr int HEADER_PITCH = container::kWaveMaxHeader;

// What the kernels need of one file (a device table, one per file)
struct FileTab {
    int64_t data_at;                             // of the data chunk's bytes in d_images: image offset + data offset
    int64_t image_off;
    int first_channel, nch, bps;                 // bps: bytes per sample, 2 or 1
    int frames;                                  // samples per channel the kernels move
    int span_frames;                             // > 0: the file takes the tile form, with spans of this many frames
    int header_size;                             // (write)
};
struct Item { int x; uint32_t y; };              // TILE: file, first frame; GENERAL: file (write) / row (read), chunk

struct FilesLayout {
    vga_wave_files_totals totals = {};
    bool from_infos = false;
    std::vector<int> first_channel, image_size;  // per file
    std::vector<int64_t> image_off;              // per file
    std::vector<int64_t> row_off;                // per row, samples
    std::vector<int> row_samples, row_file;      // per row
    std::vector<FileTab> tab;
    std::vector<uint8_t> headers;                // (write) HEADER_PITCH bytes per file
    // [0]: every file in its own form, the tile items in front; [1]: every file in the general form (the force hook)
    std::vector<Item> items[2];
    int tile_items = 0;                          // of items[0]
    int tile_files = 0, general_files = 0, moving_files = 0;   // of items[0]; files that move samples at all
};

// frames of one span of a file whose frame is `frame` bytes; 0: the file does not take the tile form
inline int span_frames(int frame) { return frame <= MAX_TILE_FRAME ? SPAN_BYTES / frame / 8 * 8 : 0; }

// the items of file f for both tables; the tile items are gathered by finish_items
inline void cut_items(FilesLayout &L, int f)
{
    FileTab &t = L.tab[f];
    if (t.frames <= 0) return;
    L.moving_files++;
    // write: chunks of the file's interleaved bytes; read: chunks of every row
    const int64_t per = L.from_infos ? (int64_t)t.frames * 2 : (int64_t)t.frames * t.nch * t.bps;
    t.span_frames = span_frames(t.nch * t.bps);
    fileset::cut_general_items(L.items, t.span_frames > 0, L.from_infos ? t.first_channel : f, L.from_infos ? t.nch : 1, per,
                               (int64_t)CHUNK_GRANULES * GRANULE_BYTES);
    if (t.span_frames > 0) L.tile_files++;
    else L.general_files++;
}
// the tile items go in front (they are one launch, the general items the next)
inline int finish_items(FilesLayout &L)
{
    std::vector<Item> tile;
    for (size_t f = 0; f < L.tab.size(); f++)
        for (int k0 = 0; L.tab[f].span_frames > 0 && k0 < L.tab[f].frames; k0 += L.tab[f].span_frames) tile.push_back({(int)f, (uint32_t)k0});
    L.tile_items = fileset::put_in_front(L.items[0], tile);
    return fileset::check_item_count(std::max(L.items[0].size(), L.items[1].size()));
}

// ranges [off, off + len) (len > 0 only) must not overlap; `what` names them, file_of(i) the file of range i
template <class FileOf>
inline int check_overlap(const std::vector<int64_t> &off, const std::vector<int> &len, const char *what, FileOf file_of)
{
    int a, b;
    if (!fileset::find_overlap((int)off.size(), [&](int i) { return off[i]; }, [&](int i) { return len[i]; }, a, b)) return VGA_OK;
    set_error("file %d: %s %d (offset %lld, length %d) overlaps %s %d (offset %lld)", file_of(std::max(a, b)), what, a, (long long)off[a],
              len[a], what, b, (long long)off[b]);
    return VGA_ERR_ARGUMENT;
}

// Called for every file, in order, BEFORE a row is placed (a row costs 16 bytes of host tables): the set's rows so far
inline int count_rows(int f, int nch, int64_t &rows) { return fileset::count_rows(f, nch, rows, "rows"); }

// the running placement of a set: the rows placed so far, where the next row (in samples) and the next image go
struct Placement {
    int64_t channels = 0;
    fileset::Rows rows;
    fileset::Images images;
};

// The rows and the image of file f, shared by both kinds of set.  `samples` per row, `size` bytes of image.
inline int place_file(FilesLayout &L, int f, int nch, int samples, int64_t size, const int64_t *pcm_offsets, const int64_t *image_offsets, Placement &P)
{
    L.first_channel[f] = (int)P.channels;
    for (int i = 0; i < nch; i++) {
        const int64_t row = P.channels + i;
        const fileset::Placed r = P.rows.place(samples, pad_to(samples, ROW_ROUND), fileset::MAX_TOTAL / 2, pcm_offsets ? pcm_offsets + row : nullptr);
        if (r.verdict & fileset::OFFSET_NEGATIVE) { set_error("file %d: pcm offset %lld of row %lld is negative", f, (long long)r.at, (long long)row); return VGA_ERR_ARGUMENT; }
        if (r.verdict) { set_error("file %d: the rows of the set exceed 2^62 bytes", f); return VGA_ERR_OUT_OF_RANGE; }
        L.row_off.push_back(r.at);
        L.row_samples.push_back(samples);
        L.row_file.push_back(f);
    }
    const fileset::Placed image = P.images.place(size, image_offsets ? image_offsets + f : nullptr);
    if (image.verdict & fileset::OFFSET_NEGATIVE) { set_error("file %d: negative image offset %lld", f, (long long)image.at); return VGA_ERR_ARGUMENT; }
    if (image.verdict & fileset::OFFSET_PAST_MAX) { set_error("file %d: the images of the set exceed 2^62 bytes", f); return VGA_ERR_OUT_OF_RANGE; }
    L.image_off[f] = image.at;
    L.image_size[f] = (int)size;
    P.channels += nch;
    return VGA_OK;
}

inline int finish_layout(FilesLayout &L, const int64_t *pcm_offsets, const Placement &P)
{
    if (pcm_offsets)
        if (int rc = check_overlap(L.row_off, L.row_samples, "row", [&](int c) { return L.row_file[c]; })) return rc;
    L.totals.channels = (int)P.channels;
    L.totals.pcm_samples = P.rows.end + GUARD_SAMPLES;
    L.totals.image_bytes = P.images.total();
    return finish_items(L);
}

// a set for writing
inline int make_layout(const vga_wave_file *files, int nfiles, const int64_t *pcm_offsets, const int64_t *image_offsets, FilesLayout &L)
{
    if (int rc = fileset::check_files(nfiles, files != nullptr, "files")) return rc;
    fileset::start_layout(L, nfiles, false);
    L.headers.assign((size_t)nfiles * HEADER_PITCH, 0);
    Placement P;
    int64_t rows = 0;
    std::vector<int> sizes((size_t)nfiles);
    for (int f = 0; f < nfiles; f++) {                       // every file's own checks first: nothing is placed for a set that is refused here
        const vga_wave_file &F = files[f];
        if (F.bits != 16 && F.bits != 8) { set_error("file %d: %d bits per sample: a set writes 16 or 8", f, F.bits); return VGA_ERR_ARGUMENT; }
        const int64_t size = container::wave_file_size(&F.params, F.channels, F.bits / 8);
        if (size < 0) return name_file(f, (int)size);
        sizes[f] = (int)size;
        if (int rc = count_rows(f, F.channels, rows)) return rc;
    }
    L.row_off.reserve((size_t)rows);
    L.row_samples.reserve((size_t)rows);
    L.row_file.reserve((size_t)rows);
    for (int f = 0; f < nfiles; f++) {
        const vga_wave_file &F = files[f];
        const int bps = F.bits / 8;
        const int64_t size = sizes[f];
        if (int rc = place_file(L, f, F.channels, F.params.sample_count, size, pcm_offsets, image_offsets, P)) return rc;
        FileTab &t = L.tab[f];
        std::memset(&t, 0, sizeof t);
        t.header_size = container::wave_header_size(&F.params, F.channels);
        container::wave_header(&F.params, F.channels, size, L.headers.data() + (size_t)f * HEADER_PITCH, bps);
        t.image_off = L.image_off[f];
        t.data_at = t.image_off + t.header_size;
        t.first_channel = L.first_channel[f];
        t.nch = F.channels;
        t.bps = bps;
        t.frames = F.params.sample_count;
        cut_items(L, f);
    }
    if (image_offsets)
        if (int rc = check_overlap(L.image_off, L.image_size, "image", [](int f) { return f; })) return rc;
    return finish_layout(L, pcm_offsets, P);
}

// a set for reading, from what vga_wave_parse returned for every file
inline int make_layout_from_infos(const vga_wave_info *const *infos, int nfiles, const int64_t *pcm_offsets, const int64_t *image_offsets,
                                  FilesLayout &L)
{
    if (int rc = fileset::check_files(nfiles, infos != nullptr, "infos")) return rc;
    fileset::start_layout(L, nfiles, true);
    Placement P;
    int64_t rows = 0;
    std::vector<int> sizes((size_t)nfiles);
    for (int f = 0; f < nfiles; f++) {                       // every file's own checks first: nothing is placed for a set that is refused here
        const vga_wave_info *I = infos[f];
        if (!I) { set_error("file %d: null info", f); return VGA_ERR_ARGUMENT; }
        // (a WAVE header's channel count is 16 bits wide)
        if (I->channel_count < 0 || I->channel_count > 0xFFFF || I->sample_count < 0 || I->data_size < 0) { set_error("file %d: info does not describe this file", f); return VGA_ERR_ARGUMENT; }
        // a caller-made data_offset is bounded before anything is added to it (a negative one is the per-file check's to refuse)
        if (I->data_offset > 0x7FFFFFFF) { set_error("file %d: image past 2 GiB", f); return VGA_ERR_OUT_OF_RANGE; }
        // the image a set sees runs to the end of the data bytes present: that is the file length the per-file checks get
        const int64_t size = I->data_offset + (int64_t)I->data_size;
        if (int rc = I->bits_per_sample == 8 ? container::wave_read8_check(I, size) : container::wave_read16_check(I, size)) return name_file(f, rc);
        if (size > 0x7FFFFFFF) { set_error("file %d: image past 2 GiB", f); return VGA_ERR_OUT_OF_RANGE; }
        sizes[f] = (int)size;
        if (int rc = count_rows(f, I->channel_count, rows)) return rc;
    }
    L.row_off.reserve((size_t)rows);
    L.row_samples.reserve((size_t)rows);
    L.row_file.reserve((size_t)rows);
    for (int f = 0; f < nfiles; f++) {
        const vga_wave_info *I = infos[f];
        const int64_t size = sizes[f];
        if (int rc = place_file(L, f, I->channel_count, I->sample_count, size, pcm_offsets, image_offsets, P)) return rc;
        FileTab &t = L.tab[f];
        std::memset(&t, 0, sizeof t);
        t.image_off = L.image_off[f];
        t.data_at = t.image_off + I->data_offset;
        t.first_channel = L.first_channel[f];
        t.nch = I->channel_count;
        t.bps = I->bits_per_sample / 8;
        t.frames = I->channel_count > 0 ? I->sample_count : 0;
        cut_items(L, f);
    }
    return finish_layout(L, pcm_offsets, P);
}

// ---- the work items as the public accessor describes them: what the kernels compute from FileTab and Item
inline void describe_items(const FilesLayout &L, bool general, std::vector<vga_wave_files_item> &out)
{
    const int nfiles = L.totals.files;
    const std::vector<Item> &items = L.items[general ? 1 : 0];
    const int tile_items = general ? 0 : L.tile_items;
    if (!L.from_infos)
        for (int f = 0; f < nfiles; f++) out.push_back({VGA_WAVE_FILES_HEADER, f, f, 0, 0, 0, L.tab[f].header_size});
    for (size_t i = 0; i < items.size(); i++) {
        const Item it = items[i];
        const bool tile = (int)i < tile_items;
        const int f = tile || !L.from_infos ? it.x : L.row_file[it.x];
        const FileTab &t = L.tab[f];
        // bytes of one frame in the item's space: the image's data chunk (write) or one int16 row (read)
        const int64_t group = L.from_infos ? 2 : (int64_t)t.nch * t.bps;
        const int64_t base = L.from_infos ? 0 : t.header_size, total = group * t.frames;
        vga_wave_files_item d = {tile ? VGA_WAVE_FILES_TILE : VGA_WAVE_FILES_GENERAL, f, it.x, it.y, tile ? t.span_frames : 0, 0, 0};
        if (tile) {
            d.begin = base + group * it.y;
            d.end = base + group * std::min<int64_t>((int64_t)it.y + t.span_frames, t.frames);
        } else {
            const int64_t unit = (int64_t)CHUNK_GRANULES * GRANULE_BYTES;
            d.begin = base + unit * it.y;
            d.end = base + std::min(unit * ((int64_t)it.y + 1), total);
        }
        out.push_back(d);
    }
}

// ---- the calls' argument checks
inline int check_write(const FilesLayout &L, const void *d_pcm, const void *d_images)
{
    const char *what = "vga_wave_write_device_v";
    if (L.from_infos) { set_error("%s: the set was made from parsed headers (vga_wave_files_create_from_infos): it serves the read call", what); return VGA_ERR_INVALID_OP; }
    if (!d_images || (!d_pcm && L.moving_files > 0)) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if ((uintptr_t)d_pcm & 1) { set_error("%s: d_pcm needs 2-byte alignment", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}
inline int check_read(const FilesLayout &L, const void *d_images, const void *d_pcm)
{
    const char *what = "vga_wave_read_device_v";
    if (!L.from_infos) { set_error("%s: the set was not made from parsed headers (vga_wave_files_create_from_infos)", what); return VGA_ERR_INVALID_OP; }
    if ((!d_images || !d_pcm) && L.moving_files > 0) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if ((uintptr_t)d_pcm & 1) { set_error("%s: d_pcm needs 2-byte alignment", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

}  // namespace wavf
}  // namespace vga
