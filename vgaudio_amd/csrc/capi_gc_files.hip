// capi_gc_files.hip -- sets of GC-ADPCM files on the device: channel metadata and DSP images of every file in one set of
// launches (include/vgaudio_hip/gc_files.h).  Host side only: checks, layout and work tables come from gc_files_host.hpp;
// create uploads the tables the kernels read (gc_files_kernels.hpp) through files_object.hpp, a call checks
// its pointers and launches.
#include "files_object.hpp"
#include "gc_files_kernels.hpp"

#include <cstring>
#include <vector>

using namespace vga;

struct vga_gc_files {
    static constexpr const char *type_name = "vga_gc_files";
    gcf::FilesLayout L;
    vga_gcadpcm_ragged *ragged = nullptr;
    fileset::TableBlock block;
    gcf::DeviceTables tables;
    int files() const { return L.totals.files; }
    ~vga_gc_files()
    {
        if (ragged) vga_gcadpcm_ragged_destroy(ragged);
    }
};

namespace {

using fileset::check_object;

// the ragged batch of the rows and the tables in the current device's memory
int finish_create(vga_gc_files *s)
{
    gcf::FilesLayout &L = s->L;
    if (L.totals.files == 0) {                                  // an empty set needs no device; with one it has its (empty) batch
        if (vga_gcadpcm_ragged_create(nullptr, 0, &s->ragged) != VGA_OK) s->ragged = nullptr;
        return VGA_OK;
    }
    if (int rc = require_device()) return rc;
    (void)hipGetDevice(&s->block.device);
    if (int rc = vga_gcadpcm_ragged_create(L.counts.data(), (int)L.counts.size(), &s->ragged)) return rc;
    if (vga_gcadpcm_ragged_pcm_samples(s->ragged) != L.totals.pcm_samples || vga_gcadpcm_ragged_adpcm_bytes(s->ragged) != L.totals.adpcm_bytes) {
        set_error("internal: the set's rows are not the ragged batch's");
        return VGA_ERR_DEVICE;
    }
    fileset::TablePack pack;
    const auto geom = pack.add(L.geom);
    const auto rows = pack.add(L.channel);
    const auto audio = pack.add(L.audio_items);
    const auto meta = pack.add(L.meta_items);
    if (int rc = s->block.upload(pack)) return rc;
    const void *d = s->block.d_tables;
    s->tables.geom = pack.at(geom, d);
    s->tables.rows = pack.at(rows, d);
    s->tables.audio = pack.at(audio, d);
    s->tables.meta = pack.at(meta, d);
    s->tables.channels = (int)L.channel.size();
    s->tables.audio_items = (int)L.audio_items.size();
    s->tables.meta_items = (int)L.meta_items.size();
    return VGA_OK;
}

void copy_offsets(const gcf::FilesLayout &L, int *first_channel_out, int64_t *seek_offsets_out, int64_t *image_offsets_out)
{
    if (first_channel_out) std::copy(L.first_channel.begin(), L.first_channel.end(), first_channel_out);
    if (seek_offsets_out)
        for (size_t c = 0; c < L.channel.size(); c++) seek_offsets_out[c] = L.channel[c].seek_off;
    if (image_offsets_out && (L.has_dsp || L.from_dsp)) std::copy(L.image_off.begin(), L.image_off.end(), image_offsets_out);
}

}  // namespace

extern "C" {

int vga_gc_files_layout_for(const vga_gc_file *files, int nfiles, const vga_dsp_file_config *dsp, int *first_channel_out,
                            int64_t *seek_offsets_out, int64_t *image_offsets_out, vga_gc_files_totals *totals_out)
{
    if (!first_channel_out && !seek_offsets_out && !image_offsets_out && !totals_out) { set_error("vga_gc_files_layout_for: no output"); return VGA_ERR_ARGUMENT; }
    gcf::FilesLayout L;
    if (int rc = gcf::make_layout(files, nfiles, dsp, L)) return rc;
    copy_offsets(L, first_channel_out, seek_offsets_out, image_offsets_out);
    if (totals_out) *totals_out = L.totals;
    return VGA_OK;
}

int vga_gc_files_create(const vga_gc_file *files, int nfiles, const vga_dsp_file_config *dsp, vga_gc_files **out)
{
    return fileset::create_with(out, [&](gcf::FilesLayout &L) { return gcf::make_layout(files, nfiles, dsp, L); }, finish_create);
}

int vga_gc_files_create_from_dsp(const vga_dsp_info *const *infos, int nfiles, const int64_t *image_offsets, vga_gc_files **out)
{
    return fileset::create_with(out, [&](gcf::FilesLayout &L) { return gcf::make_layout_from_dsp(infos, nfiles, image_offsets, L); }, finish_create);
}

void vga_gc_files_destroy(vga_gc_files *s) { delete s; }

int vga_gc_files_totals_of(const vga_gc_files *s, vga_gc_files_totals *out)
{
    if (!s || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    *out = s->L.totals;
    return VGA_OK;
}

int vga_gc_files_offsets(const vga_gc_files *s, int *first_channel_out, int64_t *seek_offsets_out, int64_t *image_offsets_out)
{
    if (!s) { set_error("null vga_gc_files"); return VGA_ERR_ARGUMENT; }
    copy_offsets(s->L, first_channel_out, seek_offsets_out, image_offsets_out);
    return VGA_OK;
}

const vga_gcadpcm_ragged *vga_gc_files_ragged(const vga_gc_files *s) { return s ? s->ragged : nullptr; }

int vga_gcadpcm_build_channels_device_v(const vga_gc_files *s, const uint8_t *d_adpcm, const int16_t *d_coefs, int16_t *d_pcm_out,
                                        int16_t *d_seek_out, int16_t *d_loop_context_out, int *d_status, void *d_workspace,
                                        size_t workspace_bytes, void *stream)
{
    if (int rc = check_object(s, "vga_gcadpcm_build_channels_device_v")) return rc;
    const gcf::FilesLayout &L = s->L;
    if (L.totals.files == 0) return VGA_OK;
    if (int rc = gcf::check_build(L, d_adpcm, d_coefs, d_pcm_out, d_seek_out, d_loop_context_out, d_workspace, workspace_bytes)) return rc;
    const bool want_seek = d_seek_out && L.any_seek;
    int16_t *pcm = d_pcm_out ? d_pcm_out : static_cast<int16_t *>(d_workspace);
    if (gcf::build_needs_decode(L, d_pcm_out != nullptr, d_seek_out != nullptr, d_loop_context_out != nullptr))   // EnsurePcmDecoded (GcAdpcmChannelBuilder.cs:202)
        if (int rc = vga_gcadpcm_decode_device_v(s->ragged, d_adpcm, d_coefs, nullptr, nullptr, pcm, d_status, stream)) return rc;
    return gcf::launch_meta(s->tables, want_seek, d_adpcm, pcm, want_seek ? d_seek_out : nullptr, d_loop_context_out, (hipStream_t)stream);
}

int vga_dsp_write_device_v(const vga_gc_files *s, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *d_gain,
                           const int16_t *d_start_context, const int16_t *d_loop_context, uint8_t *d_images, void *stream)
{
    if (int rc = check_object(s, "vga_dsp_write_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = gcf::check_write(s->L, d_adpcm, d_coefs, d_images)) return rc;
    return gcf::launch_write_images(s->tables, d_adpcm, d_coefs, d_gain, d_start_context, d_loop_context, d_images, (hipStream_t)stream);
}

int vga_dsp_read_device_v(const vga_gc_files *s, const uint8_t *d_images, uint8_t *d_adpcm, int16_t *d_coefs, int16_t *d_gain,
                          int16_t *d_start_context, int16_t *d_loop_context, void *stream)
{
    if (int rc = check_object(s, "vga_dsp_read_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = gcf::check_read(s->L, d_images, d_adpcm)) return rc;
    return gcf::launch_read_images(s->tables, d_images, d_adpcm, d_coefs, d_gain, d_start_context, d_loop_context, (hipStream_t)stream);
}

}  // extern "C"
