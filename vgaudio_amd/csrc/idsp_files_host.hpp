// idsp_files_host.hpp -- the host side of include/vgaudio_hip_files/idsp_files.h without HIP: every check, the packed layout of
// a set of IDSP files (rows, images), the per-file table and the work items the kernels of idsp_files_kernels.hip read, and the
// regions those items write (the testing hook).  File f of a set is what gcs::idsp_layout (vga_idsp_layout_for's code) says
// for the set's configuration and the file's numbers.  Header-only and free of <hip/hip_runtime.h>, so that a stand-alone
// host program can include it (tests/host/idsp_files_host_driver.cpp) as capi_idsp_files.hip does; whoever includes it
// supplies vga::set_error and vga::last_error.
#pragma once
#include "gc_files_host.hpp"
#include "gc_stream_host.hpp"
#include "../../include/vgaudio_hip_files/idsp_files.h"

namespace vga {
namespace idf {

using fileset::name_file;
constexpr uint32_t GRANULE1 = 4;                 // FileGeom::granule16 of a file read byte by byte (bits 0, 1: gc_files_host.hpp's)
constexpr int CHUNK_BYTES1 = gcf::CHUNK_GRANULES;   // bytes of one work item of that form

// the numbers IdspWriter.WriteHeader (:63-96) writes
struct HeaderGeom {
    int nch, sample_rate, sample_count, loop_start, loop_end, block_size, header_size, audio_data_size;
    int channel_sample_count, channel_nibble_count, looping, start_addr, end_addr, cur_addr;
};
// What the kernels need of one file (a device table, one per file): the header's numbers and the audio as
// Interleave(rows of channel_adpcm_bytes, interleave_size, audio_data_size) when written and DeInterleave(audio_data_length
// of every channel, interleave, nch, adpcm_bytes) when read (gcf::FileGeom: image_off, first_channel, channels, input_size,
// interleave, output_size, granule16).  The audio starts at h.header_size (written) / audio_offset (read) of the image.
struct FileTab {
    HeaderGeom h;
    gcf::FileGeom audio;
    int audio_offset, pad;
};
using ChannelRow = gcf::ChannelRow;              // adpcm_off, file (pcm_off of the same batch)
using Item = gcf::Item;                          // as gc_files_host.hpp: x = file (writer) or row (reader), y = first byte / 8, bit 31: 16 bytes
struct ChannelMeta { int16_t v[23]; };           // the reader's per-channel arrays as the object holds them (fileset::fill_meta)

struct FilesLayout {
    vga_idsp_files_totals totals = {};
    bool from_infos = false;
    std::vector<vga_idsp_layout> layout;         // per file (a set for writing)
    std::vector<int> sample_rate;                // per file
    std::vector<int> first_channel, counts;      // per file; per channel (the ragged batch's sample counts)
    std::vector<int64_t> image_off;              // per file
    std::vector<int> image_size;                 // per file
    gc::RaggedLayout rows;
    std::vector<ChannelRow> channel;
    std::vector<ChannelMeta> meta;               // (from_infos)
    std::vector<FileTab> tab;
    std::vector<Item> audio_items;
};

inline vga_idsp_params params_of(const vga_idsp_file &F, const vga_idsp_file_config &c)
{
    return {F.sample_rate, F.sample_count, F.looping, F.loop_start, F.loop_end, c.block_size, c.trim_file};
}

inline int make_layout(const vga_idsp_file *files, int nfiles, const vga_idsp_file_config *config, FilesLayout &L)
{
    if (int rc = fileset::check_files(nfiles, files != nullptr, "files")) return rc;
    if (!config) { set_error("null configuration"); return VGA_ERR_ARGUMENT; }
    fileset::start_layout(L, nfiles, false);
    L.layout.resize(nfiles);
    L.sample_rate.resize(nfiles);
    int64_t channels = 0;
    fileset::Images images;
    for (int f = 0; f < nfiles; f++) {
        const vga_idsp_file &F = files[f];
        const vga_idsp_params p = params_of(F, *config);
        vga_idsp_layout &N = L.layout[f];
        if (int rc = gcs::idsp_layout(&p, F.channels, &N)) return name_file(f, rc);
        const int first = (int)channels;
        if (int rc = fileset::count_rows(f, F.channels, channels, "channels")) return rc;
        const fileset::Placed image = images.place(N.file_size);
        L.sample_rate[f] = F.sample_rate;
        L.first_channel[f] = first;
        for (int i = 0; i < F.channels; i++) {
            L.counts.push_back(N.channel_sample_count);
            L.channel.push_back({0, 0, 0, f, N.channel.loop_start, 0, 0});
        }
        FileTab &t = L.tab[f];
        std::memset(&t, 0, sizeof t);
        t.h = {F.channels, F.sample_rate, N.sample_count, N.loop_start, N.loop_end, p.block_size, N.header_size, N.audio_data_size,
               N.channel_sample_count, gc::sample_count_to_nibble_count(N.channel_sample_count), N.looping, N.start_addr, N.end_addr,
               N.cur_addr};
        t.audio.image_off = image.at;
        t.audio.first_channel = first;
        t.audio.channels = F.channels;
        t.audio.input_size = (uint32_t)N.channel_adpcm_bytes;
        t.audio.interleave = (uint32_t)N.interleave_size;
        t.audio.output_size = (uint32_t)N.audio_data_size;
        t.audio_offset = N.header_size;
        L.image_off[f] = image.at;
        L.image_size[f] = N.file_size;
        if (image.verdict & fileset::TOTAL_PAST_MAX) { set_error("file %d: the images of the set exceed 2^62 bytes", f); return VGA_ERR_OUT_OF_RANGE; }
    }
    fileset::lay_out_rows(L.rows, L.counts, L.channel, L.totals);
    L.totals.image_bytes = images.total();
    // (an IDSP header is a multiple of 0x20, so the audio region starts on 16 whenever the image does)
    gcf::cut_writer_items(L.tab, gcf::AudioOf(), L.audio_items, gcf::interleaved_granule16);
    return VGA_OK;
}

// a set for reading, from what vga_idsp_parse returned for every file
inline int make_layout_from_infos(const vga_idsp_info *const *infos, int nfiles, const int64_t *image_offsets, FilesLayout &L)
{
    if (int rc = fileset::check_files(nfiles, infos != nullptr, "infos")) return rc;
    fileset::start_layout(L, nfiles, true);
    L.sample_rate.resize(nfiles);
    int64_t channels = 0;
    fileset::Images images;
    for (int f = 0; f < nfiles; f++) {
        const vga_idsp_info *I = infos[f];
        if (!I) { set_error("file %d: null info", f); return VGA_ERR_ARGUMENT; }
        const int nch = I->channel_count;
        if (int rc = gcs::idsp_check_info(I)) return name_file(f, rc);          // vga_idsp_read_device's check, its code and message
        // the set's own: the image starts the audio inside itself and the rows are the header's (what vga_idsp_parse fills passes)
        if (I->audio_data_offset < 0 || I->sample_count < 0 || I->adpcm_bytes != gc::sample_count_to_byte_count(I->sample_count)) {
            set_error("file %d: the info's rows of %d bytes are not those of its %d samples, or its audio offset %d is negative", f,
                      I->adpcm_bytes, I->sample_count, I->audio_data_offset);
            return VGA_ERR_ARGUMENT;
        }
        const int64_t size = (int64_t)I->audio_data_offset + (int64_t)nch * I->audio_data_length;
        const fileset::Placed image = images.place(size, image_offsets ? image_offsets + f : nullptr);
        const int64_t at = image.at;
        if (image.verdict & fileset::OFFSET_NEGATIVE) { set_error("file %d: negative image offset %lld", f, (long long)at); return VGA_ERR_ARGUMENT; }
        const int first = (int)channels;
        if (int rc = fileset::count_rows(f, nch, channels, "channels")) return rc;
        if (image.verdict & (fileset::IMAGE_PAST_2GIB | fileset::OFFSET_PAST_MAX)) { set_error("file %d: image past 2 GiB or offset past 2^62", f); return VGA_ERR_OUT_OF_RANGE; }
        L.sample_rate[f] = I->sample_rate;
        L.first_channel[f] = first;
        L.image_off[f] = at;
        L.image_size[f] = (int)size;
        for (int i = 0; i < nch; i++) {
            L.counts.push_back(I->sample_count);
            L.channel.push_back({0, 0, 0, f, 0, 0, 0});
            L.meta.push_back(fileset::fill_meta<ChannelMeta>(*I, i));
        }
        FileTab &t = L.tab[f];
        std::memset(&t, 0, sizeof t);
        t.h.nch = nch;
        t.audio.image_off = at;
        t.audio.first_channel = first;
        t.audio.channels = nch;
        t.audio.sample_count = I->sample_count;
        t.audio.output_size = (uint32_t)I->adpcm_bytes;
        t.audio.input_size = (uint32_t)I->audio_data_length;
        t.audio.interleave = (uint32_t)I->interleave;
        // the widest granule the audio's address, the interleave and the bytes per channel are all multiples of
        const uint64_t geometry = (uint64_t)(at + I->audio_data_offset) | t.audio.interleave | t.audio.input_size;
        t.audio.granule16 = geometry % 16 == 0 ? 1u : geometry % 8 == 0 ? 0u : GRANULE1;
        t.audio_offset = I->audio_data_offset;
        // (row, chunk) items over the rows this file fills
        const bool g16 = t.audio.granule16 & 1;
        const uint64_t step = t.audio.granule16 & GRANULE1 ? (uint64_t)CHUNK_BYTES1 : (uint64_t)gcf::CHUNK_GRANULES * (g16 ? 16 : 8);
        for (int i = 0; i < nch; i++)
            for (uint64_t b = 0; b < t.audio.output_size; b += step)
                L.audio_items.push_back({first + i, (uint32_t)(b >> 3) | (g16 ? 0x80000000u : 0u)});
    }
    fileset::lay_out_rows(L.rows, L.counts, L.channel, L.totals);
    L.totals.image_bytes = images.total();
    return VGA_OK;
}

// ---- what the items write (the kernels' own arithmetic): the hook of idsp_files.h
inline void writer_item_range(const gcf::FileGeom &g, const Item &it, uint32_t *start, uint32_t *end, int *granule)
{
    const bool g16 = (it.y >> 31) != 0;
    *start = (it.y & 0x7FFFFFFFu) << 3;
    const uint32_t total = g.output_size * (uint32_t)g.channels;
    const uint32_t out_blocks = (g.output_size + g.interleave - 1) / g.interleave;
    const uint32_t boundary = (out_blocks - 1) * g.interleave * (uint32_t)g.channels;
    const uint32_t part_end = *start < boundary ? boundary : total;
    const uint32_t chunk = (uint32_t)gcf::CHUNK_GRANULES * (g16 ? 16u : 8u);
    *end = part_end - *start < chunk ? part_end : *start + chunk;
    *granule = g16 ? 16 : 8;
}
inline void reader_item_range(const gcf::FileGeom &g, const Item &it, uint32_t *start, uint32_t *end, int *granule)
{
    const bool g16 = (it.y >> 31) != 0, g1 = (g.granule16 & GRANULE1) != 0;
    *start = (it.y & 0x7FFFFFFFu) << 3;
    const uint32_t chunk = g1 ? (uint32_t)CHUNK_BYTES1 : (uint32_t)gcf::CHUNK_GRANULES * (g16 ? 16u : 8u);
    *end = g.output_size - *start < chunk ? g.output_size : *start + chunk;
    *granule = g1 ? 1 : g16 ? 16 : 8;
}
inline void regions_of(const FilesLayout &L, std::vector<vga_idsp_files_region> &out)
{
    out.clear();
    if (!L.from_infos)
        for (int f = 0; f < L.totals.files; f++) out.push_back({VGA_IDSP_FILES_HEADER, f, 0, 0, L.tab[f].h.header_size});
    for (const Item &it : L.audio_items) {
        uint32_t start, end;
        int granule;
        if (L.from_infos) {
            reader_item_range(L.tab[L.channel[it.x].file].audio, it, &start, &end, &granule);
            out.push_back({VGA_IDSP_FILES_AUDIO, it.x, granule, start, end});
        } else {
            writer_item_range(L.tab[it.x].audio, it, &start, &end, &granule);
            const int64_t at = L.tab[it.x].audio_offset;
            out.push_back({VGA_IDSP_FILES_AUDIO, it.x, granule, at + start, at + end});
        }
    }
}
inline int copy_regions(const FilesLayout &L, vga_idsp_files_region *regions_out, int64_t capacity, int64_t *count_out)
{
    std::vector<vga_idsp_files_region> r;
    regions_of(L, r);
    return fileset::copy_regions(r, regions_out, capacity, count_out);
}

// ---- the calls' argument checks
inline int check_write(const FilesLayout &L, const void *d_adpcm, const void *d_coefs, const void *d_images)
{
    const char *what = "vga_idsp_write_device_v";
    if (L.from_infos) { set_error("%s: the set was made from parsed headers (vga_idsp_files_create_from_infos): it serves the read call", what); return VGA_ERR_INVALID_OP; }
    if (!d_adpcm || !d_coefs || !d_images) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (!gcf::aligned16(d_adpcm) || !gcf::aligned16(d_images)) { set_error("%s: d_adpcm and d_images need 16-byte alignment", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}
inline int check_read(const FilesLayout &L, const void *d_images, const void *d_adpcm)
{
    const char *what = "vga_idsp_read_device_v";
    if (!L.from_infos) { set_error("%s: the set was not made from parsed headers (vga_idsp_files_create_from_infos)", what); return VGA_ERR_INVALID_OP; }
    if (!d_images || !d_adpcm) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (!gcf::aligned16(d_adpcm) || !gcf::aligned16(d_images)) { set_error("%s: d_adpcm and d_images need 16-byte alignment", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

}  // namespace idf
}  // namespace vga
