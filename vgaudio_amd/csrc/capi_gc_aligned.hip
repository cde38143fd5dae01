// capi_gc_aligned.hip -- sets of GC-ADPCM files whose loops need the alignment re-encode, on the device: aligned ADPCM, PCM,
// seek tables and loop contexts of every file in one set of launches (include/vgaudio_hip/gc_files_aligned.h).  Host side
// only: checks, layout, work tables and the cut of the workspace come from gc_aligned_host.hpp; create uploads the tables
// the kernels read (gc_aligned_kernels.hpp) and the tail batch's shape through files_object.hpp, a call
// checks its pointers and launches.
#include "gc_capi.hpp"
#include "files_object.hpp"
#include "gc_aligned_kernels.hpp"

#include <cstring>
#include <vector>

using namespace vga;

struct vga_gc_aligned {
    static constexpr const char *type_name = "vga_gc_aligned";
    gca::AlignedLayout L;
    vga_gcadpcm_ragged *ragged_in = nullptr, *ragged_out = nullptr;
    gc::RaggedShape tail;                        // the tails to encode: one row per channel of a file that needs alignment
    gc::Ragged tail_view;
    fileset::TableBlock block;
    gca::DeviceTables tables;
    int files() const { return L.totals.files; }
    ~vga_gc_aligned()
    {
        if (ragged_in) vga_gcadpcm_ragged_destroy(ragged_in);
        if (ragged_out) vga_gcadpcm_ragged_destroy(ragged_out);
    }
};

namespace {

using fileset::check_object;

// the two ragged batches of the rows, the tail batch's shape and the tables in the current device's memory
int finish_create(vga_gc_aligned *s)
{
    gca::AlignedLayout &L = s->L;
    if (L.totals.files == 0) {                                  // an empty set needs no device; with one it has its (empty) batches
        if (vga_gcadpcm_ragged_create(nullptr, 0, &s->ragged_in) != VGA_OK) s->ragged_in = nullptr;
        if (vga_gcadpcm_ragged_create(nullptr, 0, &s->ragged_out) != VGA_OK) s->ragged_out = nullptr;
        return VGA_OK;
    }
    if (int rc = require_device()) return rc;
    (void)hipGetDevice(&s->block.device);
    const int nch = (int)L.channel.size();
    if (int rc = vga_gcadpcm_ragged_create(L.in.counts.data(), nch, &s->ragged_in)) return rc;
    if (int rc = vga_gcadpcm_ragged_create(L.out_counts.data(), nch, &s->ragged_out)) return rc;
    if (vga_gcadpcm_ragged_pcm_samples(s->ragged_in) != L.totals.pcm_samples || vga_gcadpcm_ragged_adpcm_bytes(s->ragged_in) != L.totals.adpcm_bytes ||
        vga_gcadpcm_ragged_pcm_samples(s->ragged_out) != L.totals.out_pcm_samples ||
        vga_gcadpcm_ragged_adpcm_bytes(s->ragged_out) != L.totals.out_adpcm_bytes) {
        set_error("internal: the set's rows are not the ragged batches'");
        return VGA_ERR_DEVICE;
    }
    s->tail.build(L.tail_counts.data(), (int)L.tail_counts.size(), 0, 0);
    if (s->tail.pcm_end != L.tail_rows.pcm_end || s->tail.adpcm_end != L.tail_rows.adpcm_end) {
        set_error("internal: the tail batch is not the host layer's");
        return VGA_ERR_DEVICE;
    }
    fileset::TablePack pack;
    const auto rows = pack.add(L.channel);
    const auto gather = pack.add(L.gather_items);
    const auto adpcm = pack.add(L.adpcm_items);
    const auto pcm = pack.add(L.pcm_items);
    const auto meta = pack.add(L.meta_items);
    const size_t tail_at = pack.add_raw(s->tail.table_bytes());
    std::vector<unsigned char> host = pack.image();
    if (s->tail.count > 0) s->tail.write_tables(host.data() + tail_at);
    if (int rc = s->block.upload(host)) return rc;
    const unsigned char *d = static_cast<const unsigned char *>(s->block.d_tables);
    s->tables.rows = pack.at(rows, d);
    s->tables.gather = pack.at(gather, d);
    s->tables.adpcm = pack.at(adpcm, d);
    s->tables.pcm = pack.at(pcm, d);
    s->tables.meta = pack.at(meta, d);
    s->tables.channels = nch;
    s->tables.gather_items = (int)L.gather_items.size();
    s->tables.adpcm_items = (int)L.adpcm_items.size();
    s->tables.pcm_items = (int)L.pcm_items.size();
    s->tables.meta_items = (int)L.meta_items.size();
    if (s->tail.count > 0) s->tail_view = s->tail.device_view(d + tail_at);
    return VGA_OK;
}

void copy_offsets(const gca::AlignedLayout &L, int *first_channel_out, int64_t *seek_offsets_out)
{
    if (first_channel_out) std::copy(L.in.first_channel.begin(), L.in.first_channel.end(), first_channel_out);
    if (seek_offsets_out)
        for (size_t c = 0; c < L.channel.size(); c++) seek_offsets_out[c] = L.channel[c].seek_off;
}

}  // namespace

extern "C" {

int vga_gc_aligned_layout_for(const vga_gc_file *files, int nfiles, int *first_channel_out, int64_t *seek_offsets_out,
                              vga_gc_aligned_totals *totals_out)
{
    if (!first_channel_out && !seek_offsets_out && !totals_out) { set_error("vga_gc_aligned_layout_for: no output"); return VGA_ERR_ARGUMENT; }
    gca::AlignedLayout L;
    if (int rc = gca::make_layout(files, nfiles, gc::encode_scratch_bytes, L)) return rc;
    copy_offsets(L, first_channel_out, seek_offsets_out);
    if (totals_out) *totals_out = L.totals;
    return VGA_OK;
}

int vga_gc_aligned_create(const vga_gc_file *files, int nfiles, vga_gc_aligned **out)
{
    return fileset::create_with(out, [&](gca::AlignedLayout &L) { return gca::make_layout(files, nfiles, gc::encode_scratch_bytes, L); }, finish_create);
}

void vga_gc_aligned_destroy(vga_gc_aligned *s) { delete s; }

int vga_gc_aligned_totals_of(const vga_gc_aligned *s, vga_gc_aligned_totals *out)
{
    if (!s || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    *out = s->L.totals;
    return VGA_OK;
}

int vga_gc_aligned_offsets(const vga_gc_aligned *s, int *first_channel_out, int64_t *seek_offsets_out)
{
    if (!s) { set_error("null vga_gc_aligned"); return VGA_ERR_ARGUMENT; }
    copy_offsets(s->L, first_channel_out, seek_offsets_out);
    return VGA_OK;
}

const vga_gcadpcm_ragged *vga_gc_aligned_ragged_in(const vga_gc_aligned *s) { return s ? s->ragged_in : nullptr; }
const vga_gcadpcm_ragged *vga_gc_aligned_ragged_out(const vga_gc_aligned *s) { return s ? s->ragged_out : nullptr; }

int vga_gcadpcm_align_channels_device_v(const vga_gc_aligned *s, const uint8_t *d_adpcm, const int16_t *d_coefs, uint8_t *d_adpcm_out,
                                        int16_t *d_pcm_out, int16_t *d_seek_out, int16_t *d_loop_context_out, int *d_status,
                                        void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check_object(s, "vga_gcadpcm_align_channels_device_v")) return rc;
    const gca::AlignedLayout &L = s->L;
    if (L.totals.files == 0) return VGA_OK;
    if (int rc = gca::check_align(L, d_adpcm, d_coefs, d_adpcm_out, d_pcm_out, d_seek_out, d_loop_context_out, d_workspace, workspace_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool want_seek = d_seek_out && L.any_seek;
    const bool pcm_read = gca::needs_pcm(L, d_pcm_out != nullptr, d_seek_out != nullptr, d_loop_context_out != nullptr);
    unsigned char *w = static_cast<unsigned char *>(d_workspace);
    // the plain decode of the input batch (GcAdpcmAlignment.cs:41-43 decodes loopEnd samples: the first loopEnd of these):
    // into the workspace, or, when no file needs alignment and the two batches are one layout, where the caller wants it
    int16_t *in_pcm = (L.any_aligned || !d_pcm_out) ? reinterpret_cast<int16_t *>(w + L.ws.in_pcm_at) : d_pcm_out;
    if (L.any_aligned || pcm_read)                              // EnsurePcmDecoded (GcAdpcmChannelBuilder.cs:202)
        if (int rc = vga_gcadpcm_decode_device_v(s->ragged_in, d_adpcm, d_coefs, nullptr, nullptr, in_pcm, d_status, stream)) return rc;
    const int16_t *tail_pcm = in_pcm;                           // (a set without tails never reads them)
    const uint8_t *tail_adpcm = d_adpcm;
    if (L.any_aligned) {
        int16_t *tp = reinterpret_cast<int16_t *>(w + L.ws.tail_pcm_at), *tc = reinterpret_cast<int16_t *>(w + L.ws.tail_coefs_at);
        int16_t *h1 = reinterpret_cast<int16_t *>(w + L.ws.hist1_at), *h2 = reinterpret_cast<int16_t *>(w + L.ws.hist2_at);
        uint8_t *ta = w + L.ws.tail_adpcm_at;
        // :44-55 the tails to encode and their histories
        if (int rc = gca::launch_gather(s->tables, in_pcm, d_coefs, tp, tc, h1, h2, st)) return rc;
        // :57-59 Encode(newPcm, history of the last kept samples), the time pieces' states in the workspace
        if (int rc = gc::launch_encode_group(s->tail, s->tail_view, tp, tc, h1, h2, ta, st, w + L.ws.scratch_at, L.ws.scratch_bytes)) return rc;
        // :61-62 PcmAligned[samplesToKeep..] = Decode(newAdpcm), over the gathered tails, which the encoder has read
        if (pcm_read)
            if (int rc = gc::launch_decode_group(s->tail, s->tail_view, ta, tc, h1, h2, tp, nullptr, st)) return rc;
        tail_pcm = tp;
        tail_adpcm = ta;
    }
    if (int rc = gca::launch_assemble_adpcm(s->tables, d_adpcm, tail_adpcm, d_adpcm_out, st)) return rc;
    if (d_pcm_out && L.any_aligned)
        if (int rc = gca::launch_assemble_pcm(s->tables, in_pcm, tail_pcm, d_pcm_out, st)) return rc;
    return gca::launch_meta(s->tables, want_seek, d_adpcm, in_pcm, tail_pcm, want_seek ? d_seek_out : nullptr, d_loop_context_out, st);
}

}  // extern "C"
