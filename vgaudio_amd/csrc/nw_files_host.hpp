// nw_files_host.hpp -- the host side of include/vgaudio_hip/nw_files.h without HIP: every check, the packed layout of a set of
// BRSTM / BCSTM / BFSTM files (rows, seek tables, images), the per-file table and the work items the kernels of
// nw_files_kernels.hip read.  File f of a set is what nw::nw_layout (vga_nwstm_layout_for's code) says for the set's
// configuration and the file's numbers.  Header-only and free of <hip/hip_runtime.h>, so that a stand-alone host program
// can include it (tests/host/nw_files_host_driver.cpp) as capi_nw_files.hip does; whoever includes it supplies
// vga::set_error and vga::last_error.
#pragma once
#include "gc_files_host.hpp"
#include "nw_host.hpp"
#include "../../include/vgaudio_hip/nw_files.h"

namespace vga {
namespace nwf {

using fileset::name_file;
constexpr int CHUNK_SHORTS = 1024;               // shorts of one seek work item: 256 threads, four each

// What the kernels need of one file (a device table, one per file): the header kernel's numbers, the audio as
// Interleave(rows of channel_adpcm_bytes, interleave_size, audio_data_size) when written and DeInterleave(audio_data_length,
// interleave_size, nch, adpcm_bytes) when read (gcf::FileGeom: image_off, first_channel, channels, input_size, interleave,
// output_size, granule16), and the seek block's geometry.
struct FileTab {
    nw::HeaderGeom h;
    gcf::FileGeom audio;
    int audio_offset;                            // of the audio region in the image
    int seek_src_entries, seek_entries;          // per channel in the packed tables; in the file (zero fill / truncation)
    int seek_body_shorts, seek_big;              // the ADPC / SEEK body, padding included; big-endian only in BRSTM
};
using ChannelRow = gcf::ChannelRow;              // adpcm_off, seek_off, file, entries (pcm_off of the same batch)
using Item = gcf::Item;                          // audio: as gc_files_host.hpp; seek: x = file, y = first short of the body
struct ChannelMeta { int16_t v[23]; };           // the reader's per-channel arrays as the object holds them (fileset::fill_meta)

struct FilesLayout {
    vga_nw_files_totals totals = {};
    bool from_infos = false;
    std::vector<vga_nwstm_layout> layout;        // per file (a set for writing)
    std::vector<int> sample_rate;                // per file
    std::vector<int> first_channel, counts;      // per file; per channel (the ragged batch's sample counts)
    std::vector<int64_t> image_off;              // per file
    std::vector<int> image_size;                 // per file
    gc::RaggedLayout rows;
    std::vector<ChannelRow> channel;
    std::vector<ChannelMeta> meta;               // (from_infos)
    std::vector<FileTab> tab;
    std::vector<Item> audio_items, seek_items;
    bool any_seek = false;
};

inline vga_nwstm_params params_of(const vga_nw_file &F, const vga_nw_file_config &c)
{
    vga_nwstm_params p = {};
    p.target = c.target;
    p.sample_rate = F.sample_rate;
    p.sample_count = F.sample_count;
    p.looping = F.looping;
    p.loop_start = F.loop_start;
    p.loop_end = F.loop_end;
    p.samples_per_interleave = c.samples_per_interleave;
    p.samples_per_seek_table_entry = c.samples_per_seek_table_entry;
    p.loop_point_alignment = c.loop_point_alignment;
    p.track_type = c.track_type;
    p.seek_table_type = c.seek_table_type;
    p.version = c.version;
    p.endianness = c.endianness;
    return p;                                    // track_count 0: the default list; the keep_* flags do not exist here
}

// rows, seek offsets and the sizes of the row buffers once counts / channel[].entries are known
inline void lay_out_rows(FilesLayout &L)
{
    fileset::lay_out_rows(L.rows, L.counts, L.channel, L.totals);
    L.totals.seek_shorts = fileset::lay_out_seek(L.channel);
}

// (file, chunk of CHUNK_SHORTS shorts) items over the body of every ADPC / SEEK block
inline void cut_seek_items(FilesLayout &L)
{
    for (size_t f = 0; f < L.tab.size(); f++)
        for (int at = 0; at < L.tab[f].seek_body_shorts; at += CHUNK_SHORTS) L.seek_items.push_back({(int)f, (uint32_t)at});
}

inline int make_layout(const vga_nw_file *files, int nfiles, const vga_nw_file_config *config, FilesLayout &L)
{
    if (int rc = fileset::check_files(nfiles, files != nullptr, "files")) return rc;
    if (!config) { set_error("null configuration"); return VGA_ERR_ARGUMENT; }
    fileset::start_layout(L, nfiles, false);
    L.layout.resize(nfiles);
    L.sample_rate.resize(nfiles);
    int64_t channels = 0;
    fileset::Images images;
    for (int f = 0; f < nfiles; f++) {
        const vga_nw_file &F = files[f];
        const vga_nwstm_params p = params_of(F, *config);
        vga_nwstm_layout &N = L.layout[f];
        std::memset(&N, 0, sizeof N);
        if (int rc = nw::nw_layout(&p, nw::kCodecGcAdpcm, F.channels, &N)) return name_file(f, rc);
        const int first = (int)channels;
        if (int rc = fileset::count_rows(f, F.channels, channels, "channels")) return rc;
        const fileset::Placed image = images.place(N.file_size);
        L.sample_rate[f] = F.sample_rate;
        L.first_channel[f] = first;
        for (int i = 0; i < F.channels; i++) {
            L.counts.push_back(N.channel_sample_count);
            L.channel.push_back({0, 0, 0, f, N.channel.loop_start, N.channel.samples_per_seek_table_entry, N.channel_seek_entries});
        }
        L.any_seek = L.any_seek || N.channel_seek_entries > 0;
        FileTab &t = L.tab[f];
        std::memset(&t, 0, sizeof t);
        nw::header_geom(N, &p, F.channels, nw::kCodecGcAdpcm, &t.h);
        t.audio.image_off = image.at;
        t.audio.first_channel = first;
        t.audio.channels = F.channels;
        t.audio.input_size = (uint32_t)N.channel_adpcm_bytes;
        t.audio.interleave = (uint32_t)N.interleave_size;
        t.audio.output_size = (uint32_t)N.audio_data_size;
        t.audio_offset = N.audio_data_offset;
        t.seek_src_entries = N.channel_seek_entries;
        t.seek_entries = N.seek_table_entry_count;
        t.seek_body_shorts = (N.seek_block_size - 8) / 2;
        t.seek_big = N.endianness == VGA_NW_BIG_ENDIAN && N.target == VGA_NW_RSTM;
        L.image_off[f] = image.at;
        L.image_size[f] = N.file_size;
        if (image.verdict & fileset::TOTAL_PAST_MAX) { set_error("file %d: the images of the set exceed 2^62 bytes", f); return VGA_ERR_OUT_OF_RANGE; }
    }
    lay_out_rows(L);
    L.totals.image_bytes = images.total();
    // (one channel is no exception to the rule here: its blocks lie `interleave` bytes apart too)
    gcf::cut_writer_items(L.tab, gcf::AudioOf(), L.audio_items, gcf::interleaved_granule16);
    cut_seek_items(L);
    return VGA_OK;
}

// a set for reading, from what vga_nwstm_parse returned for every file
inline int make_layout_from_infos(const vga_nwstm_info *const *infos, int nfiles, const int64_t *image_offsets, FilesLayout &L)
{
    if (int rc = fileset::check_files(nfiles, infos != nullptr, "infos")) return rc;
    fileset::start_layout(L, nfiles, true);
    L.sample_rate.resize(nfiles);
    int64_t channels = 0;
    fileset::Images images;
    for (int f = 0; f < nfiles; f++) {
        const vga_nwstm_info *I = infos[f];
        if (!I) { set_error("file %d: null info", f); return VGA_ERR_ARGUMENT; }
        const int nch = I->channel_count;
        // (vga_nwstm_read_device's checks, and that the rows are the header's; what vga_nwstm_parse fills passes them)
        if (nch < 1 || nch > VGA_NW_MAX_CHANNELS || I->interleave_size <= 0 || I->audio_data_length < 0 || I->audio_data_length % nch ||
            I->audio_data_offset < 0 || I->sample_count < 0 || I->adpcm_bytes != gc::sample_count_to_byte_count(I->sample_count)) {
            set_error("file %d: info does not describe a stream", f);
            return VGA_ERR_ARGUMENT;
        }
        // the set's copies move 8 or 16 bytes at a time
        if (I->audio_data_offset % 8 || I->interleave_size % 8 || (I->audio_data_length / nch) % 8) {
            set_error("file %d: its audio (offset %d, interleave %d, %d bytes per channel) is not laid out in multiples of 8: read it "
                      "with vga_nwstm_read_device", f, I->audio_data_offset, I->interleave_size, I->audio_data_length / nch);
            return VGA_ERR_INVALID_OP;
        }
        const int64_t size = (int64_t)I->audio_data_offset + I->audio_data_length;
        const fileset::Placed image = images.place(size, image_offsets ? image_offsets + f : nullptr);
        const int64_t at = image.at;
        if (at < 0 || at % 8) { set_error("file %d: image offset %lld is not a multiple of 8", f, (long long)at); return VGA_ERR_ARGUMENT; }
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
        t.audio.image_off = at;
        t.audio.first_channel = first;
        t.audio.channels = nch;
        t.audio.sample_count = I->sample_count;
        t.audio.output_size = (uint32_t)I->adpcm_bytes;
        t.audio.input_size = (uint32_t)(I->audio_data_length / nch);
        t.audio.interleave = (uint32_t)I->interleave_size;
        t.audio.granule16 = ((at + I->audio_data_offset) % 16 == 0 && t.audio.interleave % 16 == 0 && t.audio.input_size % 16 == 0) ? 1u : 0u;
        t.audio_offset = I->audio_data_offset;
    }
    lay_out_rows(L);
    L.totals.image_bytes = images.total();
    gcf::cut_reader_items(L.tab, gcf::AudioOf(), L.audio_items);
    return VGA_OK;
}

// ---- the calls' argument checks
inline int check_write(const FilesLayout &L, const void *d_adpcm, const void *d_coefs, const void *d_seek, const void *d_images)
{
    const char *what = "vga_nwstm_write_device_v";
    if (L.from_infos) { set_error("%s: the set was made from parsed headers (vga_nw_files_create_from_infos): it serves the read call", what); return VGA_ERR_INVALID_OP; }
    if (!d_adpcm || !d_coefs || !d_images || (L.any_seek && !d_seek)) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (!gcf::aligned16(d_adpcm) || !gcf::aligned16(d_seek) || !gcf::aligned16(d_images)) {
        set_error("%s: d_adpcm, d_seek and d_images need 16-byte alignment", what);
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}
inline int check_read(const FilesLayout &L, const void *d_images, const void *d_adpcm)
{
    const char *what = "vga_nwstm_read_device_v";
    if (!L.from_infos) { set_error("%s: the set was not made from parsed headers (vga_nw_files_create_from_infos)", what); return VGA_ERR_INVALID_OP; }
    if (!d_images || !d_adpcm) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (!gcf::aligned16(d_adpcm) || !gcf::aligned16(d_images)) { set_error("%s: d_adpcm and d_images need 16-byte alignment", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

}  // namespace nwf
}  // namespace vga
