// capi_nw_files.hip -- sets of BRSTM / BCSTM / BFSTM files on the device: the images of every file written and read in one set
// of launches (include/vgaudio_hip/nw_files.h).  Host side only: checks, layout and work tables come from nw_files_host.hpp;
// create uploads the tables the kernels read (nw_files_kernels.hpp) through files_object.hpp, a call checks
// its pointers and launches.
#include "files_object.hpp"
#include "nw_files_kernels.hpp"

#include <cstring>
#include <vector>

using namespace vga;

const char *vga::last_error() { return vga_last_error(); }

struct vga_nw_files {
    static constexpr const char *type_name = "vga_nw_files";
    nwf::FilesLayout L;
    vga_gcadpcm_ragged *ragged = nullptr;
    fileset::TableBlock block;
    nwf::DeviceTables tables;
    int files() const { return L.totals.files; }
    ~vga_nw_files()
    {
        if (ragged) vga_gcadpcm_ragged_destroy(ragged);
    }
};

namespace {

using fileset::check_object;

// the ragged batch of the rows and the tables in the current device's memory
int finish_create(vga_nw_files *s)
{
    nwf::FilesLayout &L = s->L;
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
    const auto tab = pack.add(L.tab);
    const auto rows = pack.add(L.channel);
    const auto meta = pack.add(L.meta);
    const auto audio = pack.add(L.audio_items);
    const auto seek = pack.add(L.seek_items);
    if (int rc = s->block.upload(pack)) return rc;
    const void *d = s->block.d_tables;
    s->tables.tab = pack.at(tab, d);
    s->tables.rows = pack.at(rows, d);
    s->tables.meta = pack.at(meta, d);
    s->tables.audio = pack.at(audio, d);
    s->tables.seek = pack.at(seek, d);
    s->tables.files = L.totals.files;
    s->tables.channels = (int)L.channel.size();
    s->tables.audio_items = (int)L.audio_items.size();
    s->tables.seek_items = (int)L.seek_items.size();
    return VGA_OK;
}

void copy_offsets(const nwf::FilesLayout &L, int *first_channel_out, int64_t *seek_offsets_out, int64_t *image_offsets_out)
{
    if (first_channel_out) std::copy(L.first_channel.begin(), L.first_channel.end(), first_channel_out);
    if (seek_offsets_out)
        for (size_t c = 0; c < L.channel.size(); c++) seek_offsets_out[c] = L.channel[c].seek_off;
    if (image_offsets_out) std::copy(L.image_off.begin(), L.image_off.end(), image_offsets_out);
}

}  // namespace

extern "C" {

int vga_nw_files_layout_for(const vga_nw_file *files, int nfiles, const vga_nw_file_config *config, int *first_channel_out,
                            int64_t *seek_offsets_out, int64_t *image_offsets_out, vga_nw_files_totals *totals_out)
{
    if (!first_channel_out && !seek_offsets_out && !image_offsets_out && !totals_out) { set_error("vga_nw_files_layout_for: no output"); return VGA_ERR_ARGUMENT; }
    nwf::FilesLayout L;
    if (int rc = nwf::make_layout(files, nfiles, config, L)) return rc;
    copy_offsets(L, first_channel_out, seek_offsets_out, image_offsets_out);
    if (totals_out) *totals_out = L.totals;
    return VGA_OK;
}

int vga_nw_files_create(const vga_nw_file *files, int nfiles, const vga_nw_file_config *config, vga_nw_files **out)
{
    return fileset::create_with(out, [&](nwf::FilesLayout &L) { return nwf::make_layout(files, nfiles, config, L); }, finish_create);
}

int vga_nw_files_create_from_infos(const vga_nwstm_info *const *infos, int nfiles, const int64_t *image_offsets, vga_nw_files **out)
{
    return fileset::create_with(out, [&](nwf::FilesLayout &L) { return nwf::make_layout_from_infos(infos, nfiles, image_offsets, L); }, finish_create);
}

void vga_nw_files_destroy(vga_nw_files *s) { delete s; }

int vga_nw_files_totals_of(const vga_nw_files *s, vga_nw_files_totals *out)
{
    if (!s || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    *out = s->L.totals;
    return VGA_OK;
}

int vga_nw_files_offsets(const vga_nw_files *s, int *first_channel_out, int64_t *seek_offsets_out, int64_t *image_offsets_out)
{
    if (!s) { set_error("null vga_nw_files"); return VGA_ERR_ARGUMENT; }
    copy_offsets(s->L, first_channel_out, seek_offsets_out, image_offsets_out);
    return VGA_OK;
}

int vga_nw_files_gc_files(const vga_nw_files *s, vga_gc_file *out)
{
    if (!s || (s->L.totals.files > 0 && !out)) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (s->L.from_infos) { set_error("vga_nw_files_gc_files: the set was made from parsed headers and has no writer configuration"); return VGA_ERR_INVALID_OP; }
    for (int f = 0; f < s->L.totals.files; f++) out[f] = {s->L.tab[f].h.nch, s->L.sample_rate[f], s->L.layout[f].channel};
    return VGA_OK;
}

const vga_gcadpcm_ragged *vga_nw_files_ragged(const vga_nw_files *s) { return s ? s->ragged : nullptr; }

int vga_nwstm_write_device_v(const vga_nw_files *s, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *d_gain,
                             const int16_t *d_start_context, const int16_t *d_loop_context, const int16_t *d_seek, uint8_t *d_images,
                             void *stream)
{
    if (int rc = check_object(s, "vga_nwstm_write_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = nwf::check_write(s->L, d_adpcm, d_coefs, d_seek, d_images)) return rc;
    return nwf::launch_write_images(s->tables, d_adpcm, d_coefs, d_gain, d_start_context, d_loop_context, d_seek, d_images, (hipStream_t)stream);
}

int vga_nwstm_read_device_v(const vga_nw_files *s, const uint8_t *d_images, uint8_t *d_adpcm, int16_t *d_coefs, int16_t *d_gain,
                            int16_t *d_start_context, int16_t *d_loop_context, void *stream)
{
    if (int rc = check_object(s, "vga_nwstm_read_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = nwf::check_read(s->L, d_images, d_adpcm)) return rc;
    return nwf::launch_read_images(s->tables, d_images, d_adpcm, d_coefs, d_gain, d_start_context, d_loop_context, (hipStream_t)stream);
}

}  // extern "C"
