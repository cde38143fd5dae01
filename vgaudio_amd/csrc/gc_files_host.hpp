// gc_files_host.hpp -- the host side of include/vgaudio_hip/gc_files.h without HIP: every check, the packed layout of a set
// of GC-ADPCM files (rows, seek tables, DSP images) and the work tables the kernels of gc_files_kernels.hip read.
// Header-only and free of <hip/hip_runtime.h>, so that a stand-alone host program can include it
// (tests/host/gc_files_host_driver.cpp) as capi_gc_files.hip does; whoever includes it supplies vga::set_error.
#pragma once
#include "gc_files_layout.hpp"
#include "../../include/vgaudio_hip/gc_files.h"

namespace vga {
namespace gcf {

using fileset::aligned16;
constexpr int DSP_HEADER = 0x60;                 // DspWriter.cs:16, one per channel
constexpr int CHUNK_GRANULES = 1024;             // granules of one audio work item: 256 threads, four each
constexpr int CHUNK_ENTRIES = 1024;              // seek entries of one metadata work item

// What the kernels need of one file (a device table, one per file).  The audio is Interleave(channels, interleave,
// output_size) of rows of input_size bytes when written (Utilities/Interleave.cs:43-78) and DeInterleave(input_size * nch,
// interleave, nch, output_size) when read (:118-167); a single channel is one block either way.
struct FileGeom {
    int64_t image_off;
    int first_channel, channels;
    int sample_count, nibble_count, sample_rate, looping;      // the header's numbers (DspWriter.cs:56-65)
    int start_addr, end_addr, cur_addr, frames_per_interleave;
    uint32_t input_size, interleave, output_size;
    uint32_t granule16;                          // bit 0: the full blocks (the reader: the whole file) move 16-byte granules, bit 1: the last block
};
// per channel (device tables are cut from these)
struct ChannelRow {
    int64_t pcm_off, adpcm_off, seek_off;
    int file, loop_start, spacing, entries;
};
// an audio work item: x = file (writer) or channel (reader), y = its first byte / 8, bit 31: 16-byte granules
struct Item { int x; uint32_t y; };
// a metadata work item: x = channel, y = its first seek entry
struct MetaItem { int x, y; };

struct FilesLayout {
    vga_gc_files_totals totals = {};
    bool has_dsp = false, from_dsp = false;
    std::vector<int> first_channel, counts;      // per file; per channel (the ragged batch's sample counts)
    std::vector<int64_t> image_off;              // per file
    gc::RaggedLayout rows;                       // the GC ragged batch's packed rows
    std::vector<ChannelRow> channel;
    std::vector<FileGeom> geom;                  // (has_dsp or from_dsp)
    std::vector<Item> audio_items;
    std::vector<MetaItem> meta_items;            // chunk 0 of every channel first, then the other chunks
    bool any_seek = false, any_loop_start = false;
    int ctx_past_file = -1;                      // first file whose loop start lies past its data (the loop context's read)
};

// 16-byte granules need the interleave and the rows of the last block on 16: blocks are `interleave` bytes apart in the row
// and in the image alike, and a granule must not straddle two of them (the rule of nw_files and idsp_files)
inline bool interleaved_granule16(const FileGeom &g, bool last_block)
{
    if (g.interleave % 16 != 0) return false;
    if (!last_block) return true;
    const uint32_t out_blocks = (g.output_size + g.interleave - 1) / g.interleave;
    return (g.output_size - (out_blocks - 1) * g.interleave) % 16 == 0;        // rows of the last block lie last_out apart
}
// a DSP file of one channel is one row, copied from a 16-byte boundary to one
inline bool writer_granule16(const FileGeom &g, bool last_block) { return g.channels == 1 || interleaved_granule16(g, last_block); }

// where a per-file table keeps its FileGeom: the table is one (gc_files), or holds it as `audio` (nw_files, idsp_files)
struct Self { template <class T> T &operator()(T &t) const { return t; } };
struct AudioOf { template <class T> auto &operator()(T &t) const { return t.audio; } };

// (file, chunk) items over the audio region of every image: the region of file f is output_size * nch bytes; its full
// blocks and its last block are cut separately (the last block's rows are packed more tightly and may allow only the
// smaller granule), each into chunks of CHUNK_GRANULES granules.  No item lies wholly outside its image.
// granule16(geom, last_block): may that part of the file move 16-byte granules (the container's rule); geom_of: Self / AudioOf
template <class Tab, class GeomOf, class Rule>
inline void cut_writer_items(std::vector<Tab> &tab, GeomOf geom_of, std::vector<Item> &items, Rule granule16)
{
    for (size_t f = 0; f < tab.size(); f++) {
        FileGeom &g = geom_of(tab[f]);
        const uint64_t total = (uint64_t)g.output_size * g.channels;
        if (total == 0) continue;
        const uint32_t out_blocks = (g.output_size + g.interleave - 1) / g.interleave;
        const uint64_t boundary = (uint64_t)(out_blocks - 1) * g.interleave * g.channels;
        g.granule16 = (granule16(g, false) ? 1u : 0u) | (granule16(g, true) ? 2u : 0u);
        const uint64_t from[2] = {0, boundary}, to[2] = {boundary, total};
        for (int part = 0; part < 2; part++) {
            const bool g16 = (g.granule16 >> part) & 1;
            const uint64_t step = (uint64_t)CHUNK_GRANULES * (g16 ? 16 : 8);
            for (uint64_t at = from[part]; at < to[part]; at += step)
                items.push_back({(int)f, (uint32_t)(at >> 3) | (g16 ? 0x80000000u : 0u)});
        }
    }
}
inline void cut_writer_items(FilesLayout &L) { cut_writer_items(L.geom, Self(), L.audio_items, writer_granule16); }

// (channel, chunk) items over the rows the reader fills: output_size bytes each
template <class Tab, class GeomOf>
inline void cut_reader_items(const std::vector<Tab> &tab, GeomOf geom_of, std::vector<Item> &items)
{
    for (size_t f = 0; f < tab.size(); f++) {
        const FileGeom &g = geom_of(tab[f]);
        const bool g16 = g.granule16 & 1;
        const uint64_t step = (uint64_t)CHUNK_GRANULES * (g16 ? 16 : 8);
        for (int i = 0; i < g.channels; i++)
            for (uint64_t at = 0; at < g.output_size; at += step)
                items.push_back({g.first_channel + i, (uint32_t)(at >> 3) | (g16 ? 0x80000000u : 0u)});
    }
}
inline void cut_reader_items(FilesLayout &L) { cut_reader_items(L.geom, Self(), L.audio_items); }

// chunk 0 of every channel first, then the other chunks
template <class Row> inline void cut_meta_items(const std::vector<Row> &channel, std::vector<MetaItem> &items)
{
    const int nch = (int)channel.size();
    for (int c = 0; c < nch; c++) items.push_back({c, 0});
    for (int c = 0; c < nch; c++)
        for (int e = CHUNK_ENTRIES; e < channel[c].entries; e += CHUNK_ENTRIES) items.push_back({c, e});
}

// rows, seek offsets and totals once counts / channel[].entries are known
inline void lay_out_rows(FilesLayout &L)
{
    fileset::lay_out_rows(L.rows, L.counts, L.channel, L.totals);
    L.totals.seek_shorts = fileset::lay_out_seek(L.channel);
    L.totals.build_workspace_bytes = L.totals.files > 0 ? (size_t)L.totals.pcm_samples * 2 : 0;
}

inline int make_layout(const vga_gc_file *files, int nfiles, const vga_dsp_file_config *dsp, FilesLayout &L)
{
    if (int rc = fileset::check_files(nfiles, files != nullptr, "files")) return rc;
    L = FilesLayout();
    L.has_dsp = dsp != nullptr;
    L.totals.files = nfiles;
    L.first_channel.resize(nfiles);
    L.image_off.resize(nfiles);
    if (dsp) L.geom.resize(nfiles);
    int64_t channels = 0;
    fileset::Images images;
    for (int f = 0; f < nfiles; f++) {
        const vga_gc_file &F = files[f];
        const vga_gcadpcm_channel_params &p = F.channel;
        if (F.channels < 1) { set_error("file %d: a file needs at least one channel (%d)", f, F.channels); return VGA_ERR_ARGUMENT; }
        if (F.channels > VGA_DSP_MAX_CHANNELS) {
            set_error("file %d: %d channels, at most %d are handled here", f, F.channels, VGA_DSP_MAX_CHANNELS);
            return VGA_ERR_INVALID_OP;
        }
        if (p.sample_count < 0 || p.loop_start < 0 || p.loop_end < p.loop_start || p.loop_alignment_multiple < 0 ||
            p.samples_per_seek_table_entry < 0) {                               // (gc::channel_layout_for's own check)
            set_error("file %d: channel parameters out of range (samples %d, loop %d..%d, alignment %d, seek entry %d)", f,
                      p.sample_count, p.loop_start, p.loop_end, p.loop_alignment_multiple, p.samples_per_seek_table_entry);
            return VGA_ERR_OUT_OF_RANGE;
        }
        vga_gcadpcm_channel_layout C;
        if (int rc = gc::channel_layout_for(&p, &C)) { set_error("file %d: the aligned sample count overflows", f); return rc; }
        if (C.alignment_needed) {
            set_error("file %d: its loop start (%d) needs alignment to %d: the re-encode is not done for a set, send the file "
                      "through vga_gcadpcm_build_channels_device", f, p.loop_start, p.loop_alignment_multiple);
            return VGA_ERR_INVALID_OP;
        }
        const int first = (int)channels;
        if (int rc = fileset::count_rows(f, F.channels, channels, "channels")) return rc;
        L.first_channel[f] = first;
        const int row_bytes = gc::sample_count_to_byte_count(p.sample_count);
        const bool ctx_past = p.loop_start != 0 && p.loop_start / 14 * 8 >= row_bytes;      // (gc::plan_channels)
        if (ctx_past && L.ctx_past_file < 0) L.ctx_past_file = f;
        for (int i = 0; i < F.channels; i++) {
            L.counts.push_back(p.sample_count);
            L.channel.push_back({0, 0, 0, f, p.loop_start, p.samples_per_seek_table_entry, C.seek_table_entries});
        }
        L.any_seek = L.any_seek || C.seek_table_entries > 0;
        L.any_loop_start = L.any_loop_start || p.loop_start != 0;
        if (dsp) {
            const vga_dsp_params d = {F.sample_rate, p.sample_count, p.looping, p.loop_start, p.loop_end,
                                      dsp->samples_per_interleave, dsp->loop_point_alignment, dsp->trim_file};
            vga_dsp_layout D;
            if (int rc = gc::dsp_layout_for(&d, F.channels, &D)) {
                if (d.samples_per_interleave < 1 || d.samples_per_interleave % 14 != 0)
                    set_error("file %d: Number of samples per interleave must be positive and divisible by 14 (%d)", f, d.samples_per_interleave);
                else
                    set_error("file %d: its DSP image would exceed 2 GiB", f);
                return rc;
            }
            const int mono_bytes = gc::sample_count_to_byte_count(D.sample_count);
            if (F.channels == 1 && mono_bytes > row_bytes) {                    // (vga_dsp_write_device)
                set_error("file %d: channel audio (%d bytes) is shorter than the %d bytes the header's sample count needs", f, row_bytes, mono_bytes);
                return VGA_ERR_ARGUMENT;
            }
            FileGeom &g = L.geom[f];
            g = FileGeom();
            g.image_off = L.image_off[f] = images.place(D.file_size).at;
            g.first_channel = first;
            g.channels = F.channels;
            g.sample_count = D.sample_count;
            g.nibble_count = gc::sample_count_to_nibble_count(D.sample_count);
            g.sample_rate = F.sample_rate;
            g.looping = p.looping ? 1 : 0;
            g.start_addr = D.start_addr;
            g.end_addr = D.end_addr;
            g.cur_addr = D.cur_addr;
            g.frames_per_interleave = D.frames_per_interleave;
            g.input_size = (uint32_t)row_bytes;
            g.output_size = (uint32_t)D.audio_data_size;                        // (one channel: mono_bytes)
            // one channel: a plain copy, one block (container::launch_interleave)
            g.interleave = F.channels == 1 ? (uint32_t)gc::pad_to(std::max(row_bytes, 1), 16) : (uint32_t)D.bytes_per_interleave;
        }
    }
    lay_out_rows(L);
    L.totals.image_bytes = dsp ? images.total() : 0;
    if (dsp) cut_writer_items(L);
    cut_meta_items(L.channel, L.meta_items);
    return VGA_OK;
}

inline int make_layout_from_dsp(const vga_dsp_info *const *infos, int nfiles, const int64_t *image_offsets, FilesLayout &L)
{
    if (int rc = fileset::check_files(nfiles, infos != nullptr, "infos")) return rc;
    L = FilesLayout();
    L.from_dsp = true;
    L.totals.files = nfiles;
    L.first_channel.resize(nfiles);
    L.image_off.resize(nfiles);
    L.geom.resize(nfiles);
    int64_t channels = 0;
    fileset::Images images;
    for (int f = 0; f < nfiles; f++) {
        const vga_dsp_info *I = infos[f];
        if (!I) { set_error("file %d: null info", f); return VGA_ERR_ARGUMENT; }
        const int nch = I->channel_count;
        // (vga_dsp_read_device's checks; what vga_dsp_parse fills passes them)
        if (nch < 1 || nch > VGA_DSP_MAX_CHANNELS || I->sample_count < 0 || I->adpcm_bytes != gc::sample_count_to_byte_count(I->sample_count) ||
            I->data_length < 0 || I->data_length % nch || I->audio_offset != DSP_HEADER * nch ||
            (nch > 1 && (I->interleave_size <= 0 || I->interleave_size % 8 || (I->data_length / nch) % 8 || I->data_length / nch < I->adpcm_bytes)) ||
            (nch == 1 && I->data_length < I->adpcm_bytes)) {
            set_error("file %d: info does not describe a DSP file", f);
            return VGA_ERR_ARGUMENT;
        }
        // (an image past 2 GiB or an offset past 2^62 is not refused here)
        const int64_t at = images.place((int64_t)I->audio_offset + I->data_length, image_offsets ? image_offsets + f : nullptr).at;
        if (at < 0 || at % 8) { set_error("file %d: image offset %lld is not a multiple of 8", f, (long long)at); return VGA_ERR_ARGUMENT; }
        const int first = (int)channels;
        if (int rc = fileset::count_rows(f, nch, channels, "channels")) return rc;
        L.first_channel[f] = first;
        L.image_off[f] = at;
        for (int i = 0; i < nch; i++) {
            L.counts.push_back(I->sample_count);
            L.channel.push_back({0, 0, 0, f, 0, 0, 0});
        }
        FileGeom &g = L.geom[f];
        g = FileGeom();
        g.image_off = at;
        g.first_channel = first;
        g.channels = nch;
        g.sample_count = I->sample_count;
        g.nibble_count = I->nibble_count;
        g.sample_rate = I->sample_rate;
        g.looping = I->looping;
        g.start_addr = I->start_addr;
        g.end_addr = I->end_addr;
        g.cur_addr = I->cur_addr;
        g.frames_per_interleave = I->frames_per_interleave;
        g.output_size = (uint32_t)I->adpcm_bytes;
        // one channel: the bytes verbatim, one block; several: DeInterleave(length, interleave, nch, bytes)
        g.input_size = nch == 1 ? g.output_size : (uint32_t)(I->data_length / nch);
        g.interleave = nch == 1 ? (uint32_t)gc::pad_to(std::max(I->adpcm_bytes, 1), 16) : (uint32_t)I->interleave_size;
        g.granule16 = (at % 16 == 0 && (nch == 1 || (g.interleave % 16 == 0 && g.input_size % 16 == 0))) ? 1u : 0u;
    }
    lay_out_rows(L);
    L.totals.image_bytes = images.total();
    cut_reader_items(L);
    cut_meta_items(L.channel, L.meta_items);
    return VGA_OK;
}

// ---- the calls' argument checks
// need_decode / workspace of vga_gcadpcm_build_channels_device_v
inline bool build_needs_decode(const FilesLayout &L, bool want_pcm, bool want_seek, bool want_ctx)
{
    return want_pcm || (want_seek && L.any_seek) || (want_ctx && L.any_loop_start);
}
inline int check_build(const FilesLayout &L, const void *d_adpcm, const void *d_coefs, const void *d_pcm_out, const void *d_seek_out,
                       const void *d_ctx_out, const void *d_workspace, size_t workspace_bytes)
{
    const char *what = "vga_gcadpcm_build_channels_device_v";
    if (!d_adpcm || !d_coefs) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (!aligned16(d_adpcm) || !aligned16(d_pcm_out) || !aligned16(d_seek_out) || !aligned16(d_workspace)) {
        set_error("%s: d_adpcm, d_pcm_out, d_seek_out and the workspace need 16-byte alignment", what);
        return VGA_ERR_ARGUMENT;
    }
    if (d_ctx_out && L.ctx_past_file >= 0) {
        set_error("file %d: loop context: the loop start lies past the ADPCM data (the reference reads Adpcm: IndexOutOfRangeException)", L.ctx_past_file);
        return VGA_ERR_OUT_OF_RANGE;
    }
    if (!d_pcm_out && build_needs_decode(L, false, d_seek_out != nullptr, d_ctx_out != nullptr) &&
        (!d_workspace || workspace_bytes < L.totals.build_workspace_bytes)) {
        set_error("%s: workspace too small or null: need %zu bytes", what, L.totals.build_workspace_bytes);
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}
inline int check_write(const FilesLayout &L, const void *d_adpcm, const void *d_coefs, const void *d_images)
{
    const char *what = "vga_dsp_write_device_v";
    if (!L.has_dsp) { set_error("%s: the set was made without a DSP configuration", what); return VGA_ERR_INVALID_OP; }
    if (!d_adpcm || !d_coefs || !d_images) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (!aligned16(d_adpcm) || !aligned16(d_images)) { set_error("%s: d_adpcm and d_images need 16-byte alignment", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}
inline int check_read(const FilesLayout &L, const void *d_images, const void *d_adpcm)
{
    const char *what = "vga_dsp_read_device_v";
    if (!L.from_dsp) { set_error("%s: the set was not made from parsed DSP headers (vga_gc_files_create_from_dsp)", what); return VGA_ERR_INVALID_OP; }
    if (!d_images || !d_adpcm) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (!aligned16(d_adpcm) || !aligned16(d_images)) { set_error("%s: d_adpcm and d_images need 16-byte alignment", what); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

}  // namespace gcf
}  // namespace vga
