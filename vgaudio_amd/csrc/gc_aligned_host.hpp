// gc_aligned_host.hpp -- the host side of include/vgaudio_hip/gc_files_aligned.h without HIP: every check, the two packed
// batches of a set of GC-ADPCM files whose loops may need the GcAdpcmAlignment.cs re-encode (input rows over sample_count,
// output rows over sample_count_aligned), the tail batch, the per-channel AlignRow table, the work items of the kernels of
// gc_aligned_kernels.hip and the cut of the workspace.  Header-only and free of <hip/hip_runtime.h>, so that a stand-alone
// host program can include it (tests/host/gc_aligned_host_driver.cpp) as capi_gc_aligned.hip does; whoever includes it
// supplies vga::set_error.  The per-file numbers are gc::channel_layout_for's and gc::plan_channels'; the checks a set
// shares with gc_files.h are gcf::make_layout's.
#pragma once
#include "gc_files_host.hpp"
#include "../../include/vgaudio_hip/gc_files_aligned.h"

namespace vga {
namespace gca {

constexpr int CHUNK_SAMPLES = 1024;              // tail samples of one gather work item: 256 threads, four each
constexpr int CHUNK_GRANULES = 1024;             // granules of one assemble work item
constexpr int CHUNK_ENTRIES = gcf::CHUNK_ENTRIES;

// What the kernels need of one channel (a device table, one per row of the set).  A file that needs no alignment keeps
// everything: bytes_to_keep = its row's bytes, samples_to_keep = its sample count, nothing to encode, tail_row -1.
struct AlignRow {
    int64_t in_pcm_off, in_adpcm_off;            // the input batch's row (samples / bytes)
    int64_t out_pcm_off, out_adpcm_off;          // the output batch's row
    int64_t tail_pcm_off, tail_adpcm_off;        // the tail batch's row (in the workspace)
    int64_t seek_off;
    int file, tail_row;                          // tail_row: row of the tail batch, -1 for a file that needs no alignment
    int bytes_to_keep, samples_to_keep, samples_to_encode, head;       // GcAdpcmAlignment.cs:33-39, :46 (head = loop_end - samples_to_keep)
    int loop_start, loop_length, loop_start_aligned;
    int out_samples, out_bytes;                  // sample_count_aligned, SampleCountToByteCount of it
    int spacing, entries;
};
using Item = gcf::Item;                          // x = channel; gather: y = first tail sample; assemble: y = first byte / 4, bits 30-31: granule
using MetaItem = gcf::MetaItem;                  // x = channel, y = first seek entry

// the granule of an assemble item: 4 << code bytes
inline uint32_t granule_code(int64_t boundary) { return boundary % 16 == 0 ? 2u : boundary % 8 == 0 ? 1u : 0u; }

// where the workspace is cut (bytes from its base, every part on 16)
struct WorkspaceCut {
    size_t in_pcm_at = 0, tail_pcm_at = 0, tail_adpcm_at = 0, tail_coefs_at = 0, hist1_at = 0, hist2_at = 0, scratch_at = 0;
    size_t scratch_bytes = 0, total = 0;
};

struct AlignedLayout {
    vga_gc_aligned_totals totals = {};
    gcf::FilesLayout in;                         // the input side: first_channel, counts, rows (gc_files.h's layout of the same files)
    std::vector<int> out_counts, tail_counts;    // per channel; per aligned channel
    gc::RaggedLayout out_rows, tail_rows;
    std::vector<AlignRow> channel;
    std::vector<Item> gather_items, adpcm_items, pcm_items;
    std::vector<MetaItem> meta_items;            // chunk 0 of every channel first, then the other chunks
    WorkspaceCut ws;
    bool any_aligned = false, any_seek = false, any_loop_start = false;   // any_loop_start: an ALIGNED loop start that is not 0
    int ctx_past_file = -1;                      // first file whose aligned loop start lies past its original data
};

// (channel, chunk) items over a row of `total` bytes made of `keep` bytes from one source and the rest from another: the
// two parts are cut separately, the kept part in 16-byte granules (both rows start on 16), the rest in the largest
// granule that divides `keep` (its source row starts on 16, its place in the output row is `keep`)
inline void cut_assemble_items(std::vector<Item> &items, int c, uint64_t keep, uint64_t total)
{
    const uint64_t from[2] = {0, keep}, to[2] = {keep, total};
    for (int part = 0; part < 2; part++) {
        const uint32_t code = part == 0 ? 2u : granule_code((int64_t)keep);
        const uint64_t step = (uint64_t)CHUNK_GRANULES * (4u << code);
        for (uint64_t at = from[part]; at < to[part]; at += step) items.push_back({c, (uint32_t)(at >> 2) | (code << 30)});
    }
}

// encoder_scratch: gc::encode_scratch_bytes (gc_encode_kernel.hip), handed in because this header is free of HIP
inline int make_layout(const vga_gc_file *files, int nfiles, size_t (*encoder_scratch)(int), AlignedLayout &L)
{
    L = AlignedLayout();
    // everything gc_files.h checks of a set without a configuration, and the input rows, from the same files with the
    // alignment taken out (that header refuses the files this one is for)
    std::vector<vga_gc_file> plain;
    if (nfiles > 0 && files) {
        plain.assign(files, files + nfiles);
        for (vga_gc_file &f : plain) f.channel.loop_alignment_multiple = 0;
    }
    if (int rc = gcf::make_layout(plain.empty() ? files : plain.data(), nfiles, nullptr, L.in)) return rc;
    L.totals.files = nfiles;
    int tail_rows = 0;
    for (int f = 0; f < nfiles; f++) {
        const vga_gcadpcm_channel_params &p = files[f].channel;
        vga_gcadpcm_channel_layout C;
        if (int rc = gc::channel_layout_for(&p, &C)) {
            set_error("file %d: channel parameters out of range or the aligned sample count overflows (loop %d..%d, alignment %d)", f,
                      p.loop_start, p.loop_end, p.loop_alignment_multiple);
            return rc;
        }
        gc::ChannelsPlan plan;
        if (int rc = gc::plan_channels(&p, C, files[f].channels, false, plan)) {
            set_error("file %d: a zero-length loop cannot be aligned (the reference's fill loop never ends, GcAdpcmAlignment.cs:48)", f);
            return rc;
        }
        if (C.alignment_needed && p.loop_end > p.sample_count) {
            set_error("file %d: its loop needs alignment and ends (%d) past its %d samples: the row does not hold the loop (the reference's "
                      "decode of loopEnd samples runs past Adpcm)", f, p.loop_end, p.sample_count);
            return VGA_ERR_OUT_OF_RANGE;
        }
        const int row_bytes = gc::sample_count_to_byte_count(p.sample_count);
        if (C.loop_start_aligned != 0 && C.loop_start_aligned / 14 * 8 >= row_bytes && L.ctx_past_file < 0) L.ctx_past_file = f;   // (gc::plan_channels)
        for (int i = 0; i < files[f].channels; i++) {
            AlignRow r = {};
            r.file = f;
            r.tail_row = C.alignment_needed ? tail_rows++ : -1;
            r.bytes_to_keep = C.alignment_needed ? plan.bytes_to_keep : row_bytes;
            r.samples_to_keep = C.alignment_needed ? plan.samples_to_keep : p.sample_count;
            r.samples_to_encode = C.alignment_needed ? plan.samples_to_encode : 0;
            r.head = C.alignment_needed ? p.loop_end - plan.samples_to_keep : 0;
            r.loop_start = p.loop_start;
            r.loop_length = p.loop_end - p.loop_start;
            r.loop_start_aligned = C.loop_start_aligned;
            r.out_samples = C.sample_count_aligned;
            r.out_bytes = gc::sample_count_to_byte_count(C.sample_count_aligned);
            r.spacing = p.samples_per_seek_table_entry;
            r.entries = C.seek_table_entries;
            L.channel.push_back(r);
            L.out_counts.push_back(C.sample_count_aligned);
            if (C.alignment_needed) L.tail_counts.push_back(plan.samples_to_encode);
        }
        L.any_aligned = L.any_aligned || C.alignment_needed;
        L.any_seek = L.any_seek || C.seek_table_entries > 0;
        L.any_loop_start = L.any_loop_start || C.loop_start_aligned != 0;
    }
    const int nch = (int)L.channel.size();
    L.out_rows.lay_out(L.out_counts.data(), nch, 0, 0);
    L.tail_rows.lay_out(L.tail_counts.data(), tail_rows, 0, 0);
    for (int c = 0; c < nch; c++) {
        AlignRow &r = L.channel[c];
        r.in_pcm_off = L.in.rows.pcm_off[c];
        r.in_adpcm_off = L.in.rows.adpcm_off[c];
        r.out_pcm_off = L.out_rows.pcm_off[c];
        r.out_adpcm_off = L.out_rows.adpcm_off[c];
        if (r.tail_row >= 0) {
            r.tail_pcm_off = L.tail_rows.pcm_off[r.tail_row];
            r.tail_adpcm_off = L.tail_rows.adpcm_off[r.tail_row];
        }
        // work items: no item lies wholly behind its channel's data
        for (int at = 0; at < r.samples_to_encode; at += CHUNK_SAMPLES) L.gather_items.push_back({c, (uint32_t)at});
        cut_assemble_items(L.adpcm_items, c, (uint64_t)r.bytes_to_keep, (uint64_t)r.out_bytes);
        cut_assemble_items(L.pcm_items, c, (uint64_t)r.samples_to_keep * 2, (uint64_t)r.out_samples * 2);
    }
    gcf::cut_meta_items(L.channel, L.meta_items);

    L.totals.channels = nch;
    L.totals.aligned_channels = tail_rows;
    L.totals.pcm_samples = L.in.totals.pcm_samples;
    L.totals.adpcm_bytes = L.in.totals.adpcm_bytes;
    L.totals.out_pcm_samples = L.out_rows.pcm_end + gc::GUARD_BYTES / 2;
    L.totals.out_adpcm_bytes = L.out_rows.adpcm_end + gc::GUARD_BYTES;
    L.totals.seek_shorts = fileset::lay_out_seek(L.channel);
    // the workspace: the plain decode of the input batch; then, when a file needs alignment, the tail batch (PCM rows that
    // the gather fills and the second decode overwrites, ADPCM rows, the tails' coefficients and histories), guards
    // included, and the encoder's scratch
    WorkspaceCut &w = L.ws;
    size_t at = nfiles > 0 ? (size_t)L.totals.pcm_samples * 2 : 0;
    if (tail_rows > 0) {
        w.tail_pcm_at = at;
        at += (size_t)gc::pad_to((L.tail_rows.pcm_end + gc::GUARD_BYTES / 2) * 2, 16);
        w.tail_adpcm_at = at;
        at += (size_t)gc::pad_to(L.tail_rows.adpcm_end + gc::GUARD_BYTES, 16);
        w.tail_coefs_at = at;
        at += (size_t)tail_rows * 32;
        w.hist1_at = at;
        at += (size_t)gc::pad_to((int64_t)tail_rows * 2, 16);
        w.hist2_at = at;
        at += (size_t)gc::pad_to((int64_t)tail_rows * 2, 16);
        w.scratch_at = at;
        w.scratch_bytes = encoder_scratch ? (size_t)gc::pad_to((int64_t)encoder_scratch(tail_rows), 16) : 0;
        at += w.scratch_bytes;
    }
    w.total = at;
    L.totals.workspace_bytes = at;
    return VGA_OK;
}

// ---- the call's argument checks
// does anything read the decoded PCM
inline bool needs_pcm(const AlignedLayout &L, bool want_pcm, bool want_seek, bool want_ctx)
{
    return want_pcm || (want_seek && L.any_seek) || (want_ctx && L.any_loop_start);
}
// the bytes of workspace this call needs: all of it when a file needs alignment; else the plain decode when something reads
// the PCM and the caller does not take it
inline size_t workspace_needed(const AlignedLayout &L, bool want_pcm, bool want_seek, bool want_ctx)
{
    if (L.any_aligned) return L.totals.workspace_bytes;
    return !want_pcm && needs_pcm(L, false, want_seek, want_ctx) ? (size_t)L.totals.pcm_samples * 2 : 0;
}
inline int check_align(const AlignedLayout &L, const void *d_adpcm, const void *d_coefs, const void *d_adpcm_out, const void *d_pcm_out,
                       const void *d_seek_out, const void *d_ctx_out, const void *d_workspace, size_t workspace_bytes)
{
    const char *what = "vga_gcadpcm_align_channels_device_v";
    if (!d_adpcm || !d_coefs || !d_adpcm_out) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (!gcf::aligned16(d_adpcm) || !gcf::aligned16(d_adpcm_out) || !gcf::aligned16(d_pcm_out) || !gcf::aligned16(d_seek_out) ||
        !gcf::aligned16(d_workspace)) {
        set_error("%s: d_adpcm, d_adpcm_out, d_pcm_out, d_seek_out and the workspace need 16-byte alignment", what);
        return VGA_ERR_ARGUMENT;
    }
    if (d_ctx_out && L.ctx_past_file >= 0) {
        set_error("file %d: loop context: the aligned loop start lies past the original ADPCM data (the reference reads Adpcm, not "
                  "AlignedAdpcm: IndexOutOfRangeException)", L.ctx_past_file);
        return VGA_ERR_OUT_OF_RANGE;
    }
    const size_t need = workspace_needed(L, d_pcm_out != nullptr, d_seek_out != nullptr, d_ctx_out != nullptr);
    if (need > 0 && (!d_workspace || workspace_bytes < need)) {
        set_error("%s: workspace too small or null: need %zu bytes", what, need);
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}

}  // namespace gca
}  // namespace vga
