// nw_pcm_files_host.hpp -- the host side of include/vgaudio_hip_files/nw_pcm_files.h without HIP: every check, the layout of a
// set of PCM16 / PCM8 BRSTM / BCSTM / BFSTM files (rows, images), the per-file table, the work items the kernels of
// nw_pcm_files_kernels.hip read and the form every file takes.  File f of a set for writing is what nw::nw_layout
// (vga_nwstm_pcm_layout_for's code) says for the set's configuration and the file's numbers; file f of a set for reading has
// passed nw::pcm_read_info_check (vga_nwstm_pcm_read_device's code).  Rows and images are placed by wave_files_host.hpp's
// code, which is why the rows lie as vga_wave_files_layout_for lays them.  Header-only and free of <hip/hip_runtime.h>, so
// that a stand-alone host program can include it (tests/host/nw_pcm_files_host_driver.cpp) as capi_nw_pcm_files.hip does;
// whoever includes it supplies vga::set_error and vga::last_error.
#pragma once
#include "nw_files_host.hpp"
#include "wave_files_host.hpp"
#include "../../include/vgaudio_hip_files/nw_pcm_files.h"

namespace vga {
namespace nwpf {

constexpr int GRANULE_BYTES = 16;                // of the file side: what one thread of the vector form moves
constexpr int CHUNK_GRANULES = 1024;             // of one work item: 256 threads, four granules each (gc_files_chunks.hpp's)
constexpr int CHUNK_BYTES = CHUNK_GRANULES * GRANULE_BYTES;
enum : int { kCopy = VGA_NW_PCM_FILES_COPY, kSwap16 = VGA_NW_PCM_FILES_SWAP16, kPcm8 = VGA_NW_PCM_FILES_PCM8 };

// What the kernels need of one file (a device table, one per file).  Sizes are bytes of one channel AS STORED:
// write: Interleave(rows of input_size, interleave, output_size = audio_data_size);
// read:  DeInterleave(input_size = audio_data_length / nch, interleave, nch, output_size = the row's bytes as stored).
struct FileTab {
    nw::HeaderGeom h;                            // (write)
    int64_t image_off, audio_at;                 // of the image and of its audio region in d_images
    int first_channel, nch;
    uint32_t input_size, interleave, output_size;
    int conv, bps;                               // kCopy / kSwap16 / kPcm8; stored bytes per sample
    int vector;                                  // the file takes the vector form
};
using Item = wavf::Item;                         // x: file (write) / row (read); y: chunk of CHUNK_BYTES stored bytes

struct FilesLayout {
    wavf::FilesLayout P;                         // the placement: totals, first_channel, image_off / size, row_off / samples / file
    std::vector<vga_nwstm_layout> layout;        // per file (a set for writing)
    std::vector<FileTab> tab;
    // [0]: every file in its own form, the vector items in front; [1]: every file in the general form (the force hook)
    std::vector<Item> items[2];
    int vector_items = 0;                        // of items[0]
    int vector_files = 0, general_files = 0, moving_files = 0;
    bool from_infos() const { return P.from_infos; }
};

inline int conv_of(int codec, int endianness)
{
    return codec == nw::kCodecPcm8 ? kPcm8 : endianness == VGA_NW_BIG_ENDIAN ? kSwap16 : kCopy;
}

// the bytes the items of file f tile, per item owner: the audio region (write) or one row as stored (read)
inline int64_t item_space(const FilesLayout &L, const FileTab &t) { return L.from_infos() ? (int64_t)t.output_size : (int64_t)t.output_size * t.nch; }

// The form of file f and its items for both tables.  The vector form needs every 16-byte granule of the file side inside one
// (block, channel) segment and at an aligned address, and the row side of a granule aligned too.
inline void cut_items(FilesLayout &L, int f)
{
    FileTab &t = L.tab[f];
    const int64_t per = item_space(L, t);
    if (per <= 0) return;
    L.moving_files++;
    const uint32_t il = t.interleave, size = L.from_infos() ? t.input_size : t.output_size;   // the file side's bytes per channel
    const uint32_t blocks = (size + il - 1) / il, last = size ? size - (blocks - 1) * il : 0;
    bool vec = il % 16 == 0 && last % 16 == 0 && t.audio_at % 16 == 0;
    for (int c = 0; c < t.nch; c++) vec = vec && L.P.row_off[t.first_channel + c] % 8 == 0;
    t.vector = vec ? 1 : 0;
    (vec ? L.vector_files : L.general_files)++;
    // (the vector items are gathered by finish_items)
    fileset::cut_general_items(L.items, vec, L.from_infos() ? t.first_channel : f, L.from_infos() ? t.nch : 1, per, CHUNK_BYTES);
}
// the vector items go in front (they are one launch, the general items the next)
inline int finish_items(FilesLayout &L)
{
    std::vector<Item> vec;
    for (size_t f = 0; f < L.tab.size(); f++) {
        const FileTab &t = L.tab[f];
        if (!t.vector) continue;
        const int64_t per = item_space(L, t);
        const int first = L.from_infos() ? t.first_channel : (int)f, count = L.from_infos() ? t.nch : 1;
        for (int i = 0; i < count; i++)
            for (int64_t at = 0, y = 0; at < per; at += CHUNK_BYTES, y++) vec.push_back({first + i, (uint32_t)y});
    }
    L.vector_items = fileset::put_in_front(L.items[0], vec);
    return fileset::check_item_count(std::max(L.items[0].size(), L.items[1].size()));
}

// a set for writing
inline int make_layout(const vga_nw_file *files, int nfiles, const vga_nw_file_config *config, int codec, const int64_t *pcm_offsets,
                       const int64_t *image_offsets, FilesLayout &L)
{
    if (int rc = fileset::check_files(nfiles, files != nullptr, "files")) return rc;
    if (!config) { set_error("null configuration"); return VGA_ERR_ARGUMENT; }
    if (codec != nw::kCodecPcm8 && codec != nw::kCodecPcm16) { set_error("codec %d: a set holds PCM8 (0) or PCM16 (1) streams (nw_files.h for GC-ADPCM)", codec); return VGA_ERR_ARGUMENT; }
    L = FilesLayout();
    fileset::start_layout(L.P, nfiles, false);
    L.layout.resize(nfiles);
    L.tab.resize(nfiles);
    wavf::Placement P;
    int64_t rows = 0;
    for (int f = 0; f < nfiles; f++) {                       // every file's own checks first: nothing is placed for a set that is refused here
        const vga_nwstm_params p = nwf::params_of(files[f], *config);
        std::memset(&L.layout[f], 0, sizeof L.layout[f]);
        if (int rc = nw::nw_layout(&p, codec, files[f].channels, &L.layout[f])) return fileset::name_file(f, rc);
        if (int rc = wavf::count_rows(f, files[f].channels, rows)) return rc;
    }
    L.P.row_off.reserve((size_t)rows);
    L.P.row_samples.reserve((size_t)rows);
    L.P.row_file.reserve((size_t)rows);
    for (int f = 0; f < nfiles; f++) {
        const vga_nw_file &F = files[f];
        const vga_nwstm_layout &N = L.layout[f];
        if (image_offsets && image_offsets[f] >= 0 && image_offsets[f] % 16) { set_error("file %d: image offset %lld is not a multiple of 16", f, (long long)image_offsets[f]); return VGA_ERR_ARGUMENT; }
        if (int rc = wavf::place_file(L.P, f, F.channels, F.sample_count, N.file_size, pcm_offsets, image_offsets, P)) return rc;
        const vga_nwstm_params p = nwf::params_of(F, *config);
        FileTab &t = L.tab[f];
        std::memset(&t, 0, sizeof t);
        nw::header_geom(N, &p, F.channels, codec, &t.h);
        t.image_off = L.P.image_off[f];
        t.audio_at = t.image_off + N.audio_data_offset;
        t.first_channel = L.P.first_channel[f];
        t.nch = F.channels;
        t.input_size = (uint32_t)N.channel_adpcm_bytes;
        t.output_size = (uint32_t)N.audio_data_size;
        // an interleave past the audio of one channel is one block of it, whatever its size: holding it to that keeps
        // interleave * channels, which the kernels form, below the region's 2^31
        t.interleave = std::min((uint32_t)N.interleave_size, std::max(t.output_size, 1u));
        t.conv = conv_of(codec, N.endianness);
        t.bps = codec == nw::kCodecPcm16 ? 2 : 1;
        cut_items(L, f);
    }
    if (image_offsets)
        if (int rc = wavf::check_overlap(L.P.image_off, L.P.image_size, "image", [](int f) { return f; })) return rc;
    if (int rc = wavf::finish_layout(L.P, pcm_offsets, P)) return rc;
    return finish_items(L);
}

// a set for reading, from what vga_nwstm_pcm_parse returned for every file
inline int make_layout_from_infos(const vga_nwstm_info *const *infos, int nfiles, const int64_t *pcm_offsets, const int64_t *image_offsets,
                                  FilesLayout &L)
{
    if (int rc = fileset::check_files(nfiles, infos != nullptr, "infos")) return rc;
    L = FilesLayout();
    fileset::start_layout(L.P, nfiles, true);
    L.tab.resize(nfiles);
    wavf::Placement P;
    int64_t rows = 0;
    std::vector<int> sizes((size_t)nfiles);
    for (int f = 0; f < nfiles; f++) {                       // every file's own checks first
        const vga_nwstm_info *I = infos[f];
        if (!I) { set_error("file %d: null info", f); return VGA_ERR_ARGUMENT; }
        if (int rc = nw::pcm_read_info_check(I, VGA_SAMPLES_S16, true)) return fileset::name_file(f, rc);
        // what the per-file call leaves to its pointers and pitches: the set places rows and images from these numbers
        if (I->channel_count < 0 || I->channel_count > VGA_NW_MAX_CHANNELS || I->sample_count < 0 || I->audio_data_offset < 0 || I->audio_data_length < 0 ||
            I->adpcm_bytes != (int64_t)I->sample_count * (I->codec == nw::kCodecPcm16 ? 2 : 1)) {
            set_error("file %d: info does not describe this file", f);
            return VGA_ERR_ARGUMENT;
        }
        const int64_t size = (int64_t)I->audio_data_offset + I->audio_data_length;
        if (size > 0x7FFFFFFF) { set_error("file %d: image past 2 GiB", f); return VGA_ERR_OUT_OF_RANGE; }
        // the general form moves a PCM16 stream sample by sample: a sample must not straddle two segments
        if (I->codec == nw::kCodecPcm16 && I->adpcm_bytes > 0 && (I->interleave_size % 2 || (I->audio_data_length / I->channel_count) % 2)) {
            set_error("file %d: a PCM16 stream whose interleave (%d) or bytes per channel (%d) are odd: read it with vga_nwstm_pcm_read_device", f,
                      I->interleave_size, I->audio_data_length / I->channel_count);
            return VGA_ERR_INVALID_OP;
        }
        sizes[f] = (int)size;
        if (int rc = wavf::count_rows(f, I->channel_count, rows)) return rc;
    }
    L.P.row_off.reserve((size_t)rows);
    L.P.row_samples.reserve((size_t)rows);
    L.P.row_file.reserve((size_t)rows);
    for (int f = 0; f < nfiles; f++) {
        const vga_nwstm_info *I = infos[f];
        if (int rc = wavf::place_file(L.P, f, I->channel_count, I->sample_count, sizes[f], pcm_offsets, image_offsets, P)) return rc;
        FileTab &t = L.tab[f];
        std::memset(&t, 0, sizeof t);
        t.image_off = L.P.image_off[f];
        t.audio_at = t.image_off + I->audio_data_offset;
        t.first_channel = L.P.first_channel[f];
        t.nch = I->channel_count;
        t.output_size = t.nch > 0 ? (uint32_t)I->adpcm_bytes : 0u;
        t.input_size = t.output_size ? (uint32_t)(I->audio_data_length / t.nch) : 0u;
        t.interleave = (uint32_t)I->interleave_size;
        t.conv = conv_of(I->codec, I->endianness);
        t.bps = I->codec == nw::kCodecPcm16 ? 2 : 1;
        cut_items(L, f);
    }
    if (int rc = wavf::finish_layout(L.P, pcm_offsets, P)) return rc;
    return finish_items(L);
}

// ---- the work items as the public accessor describes them: what the kernels compute from FileTab and Item
inline void describe_items(const FilesLayout &L, bool general, std::vector<vga_nw_pcm_files_item> &out)
{
    const int nfiles = L.P.totals.files;
    const std::vector<Item> &items = L.items[general ? 1 : 0];
    const int vector_items = general ? 0 : L.vector_items;
    if (!L.from_infos())
        for (int f = 0; f < nfiles; f++) out.push_back({VGA_NW_PCM_FILES_HEADER, f, f, 0, L.tab[f].conv, 0, L.tab[f].h.audio_offset});
    for (size_t i = 0; i < items.size(); i++) {
        const Item it = items[i];
        const int f = L.from_infos() ? L.P.row_file[it.x] : it.x;
        const FileTab &t = L.tab[f];
        // stored bytes -> the bytes written: the image's own (write), or the int16 row's (read: two per PCM8 byte)
        const int64_t scale = L.from_infos() && t.bps == 1 ? 2 : 1, base = L.from_infos() ? 0 : t.h.audio_offset;
        const int64_t total = item_space(L, t);
        vga_nw_pcm_files_item d = {(int)i < vector_items ? VGA_NW_PCM_FILES_VECTOR : VGA_NW_PCM_FILES_GENERAL, f, it.x, it.y, t.conv, 0, 0};
        d.begin = base + scale * CHUNK_BYTES * (int64_t)it.y;
        d.end = base + scale * std::min(CHUNK_BYTES * ((int64_t)it.y + 1), total);
        out.push_back(d);
    }
}

// ---- the calls' argument checks
inline int check_write(const FilesLayout &L, const void *d_pcm, const void *d_images)
{
    const char *what = "vga_nwstm_pcm_write_device_v";
    if (L.from_infos()) { set_error("%s: the set was made from parsed headers (vga_nw_pcm_files_create_from_infos): it serves the read call", what); return VGA_ERR_INVALID_OP; }
    if (!d_images || (!d_pcm && L.moving_files > 0)) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if ((uintptr_t)d_pcm & 1) { set_error("%s: d_pcm needs 2-byte alignment", what); return VGA_ERR_ARGUMENT; }
    if ((uintptr_t)d_images & 15) { set_error("%s: d_images needs 16-byte alignment", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}
inline int check_read(const FilesLayout &L, const void *d_images, const void *d_pcm)
{
    const char *what = "vga_nwstm_pcm_read_device_v";
    if (!L.from_infos()) { set_error("%s: the set was not made from parsed headers (vga_nw_pcm_files_create_from_infos)", what); return VGA_ERR_INVALID_OP; }
    if ((!d_images || !d_pcm) && L.moving_files > 0) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if ((uintptr_t)d_pcm & 1) { set_error("%s: d_pcm needs 2-byte alignment", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}
// the vector form's accesses are aligned only from aligned bases
inline bool bases_aligned(const void *d_pcm, const void *d_images) { return (((uintptr_t)d_pcm | (uintptr_t)d_images) & 15) == 0; }

}  // namespace nwpf
}  // namespace vga
