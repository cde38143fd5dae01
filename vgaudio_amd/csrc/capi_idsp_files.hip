// capi_idsp_files.hip -- sets of IDSP files on the device: the images of every file written and read in one set of launches
// (include/vgaudio_hip_files/idsp_files.h).  Host side only: checks, layout and work tables come from idsp_files_host.hpp;
// create uploads the tables the kernels read (idsp_files_kernels.hpp) through files_object.hpp, a call
// checks its pointers and launches.
#include "files_object.hpp"
#include "idsp_files_kernels.hpp"

#include <cstring>
#include <vector>

using namespace vga;

struct vga_idsp_files {
    static constexpr const char *type_name = "vga_idsp_files";
    idf::FilesLayout L;
    vga_gcadpcm_ragged *ragged = nullptr;
    fileset::TableBlock block;
    idf::DeviceTables tables;
    int files() const { return L.totals.files; }
    ~vga_idsp_files()
    {
        if (ragged) vga_gcadpcm_ragged_destroy(ragged);
    }
};

namespace {

using fileset::check_object;

thread_local int t_last_launches = 0;            // of this thread's last _v call (vga_idsp_files_stats): cleared as the call begins

// the ragged batch of the rows and the tables in the current device's memory
int finish_create(vga_idsp_files *s)
{
    idf::FilesLayout &L = s->L;
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
    if (int rc = s->block.upload(pack)) return rc;
    const void *d = s->block.d_tables;
    s->tables.tab = pack.at(tab, d);
    s->tables.rows = pack.at(rows, d);
    s->tables.meta = pack.at(meta, d);
    s->tables.audio = pack.at(audio, d);
    s->tables.files = L.totals.files;
    s->tables.channels = (int)L.channel.size();
    s->tables.audio_items = (int)L.audio_items.size();
    return VGA_OK;
}

void copy_offsets(const idf::FilesLayout &L, int *first_channel_out, int64_t *image_offsets_out)
{
    if (first_channel_out) std::copy(L.first_channel.begin(), L.first_channel.end(), first_channel_out);
    if (image_offsets_out) std::copy(L.image_off.begin(), L.image_off.end(), image_offsets_out);
}

}  // namespace

extern "C" {

int vga_idsp_files_layout_for(const vga_idsp_file *files, int nfiles, const vga_idsp_file_config *config, int *first_channel_out,
                              int64_t *image_offsets_out, vga_idsp_files_totals *totals_out)
{
    if (!first_channel_out && !image_offsets_out && !totals_out) { set_error("vga_idsp_files_layout_for: no output"); return VGA_ERR_ARGUMENT; }
    idf::FilesLayout L;
    if (int rc = idf::make_layout(files, nfiles, config, L)) return rc;
    copy_offsets(L, first_channel_out, image_offsets_out);
    if (totals_out) *totals_out = L.totals;
    return VGA_OK;
}

int vga_idsp_files_create(const vga_idsp_file *files, int nfiles, const vga_idsp_file_config *config, vga_idsp_files **out)
{
    return fileset::create_with(out, [&](idf::FilesLayout &L) { return idf::make_layout(files, nfiles, config, L); }, finish_create);
}

int vga_idsp_files_create_from_infos(const vga_idsp_info *const *infos, int nfiles, const int64_t *image_offsets, vga_idsp_files **out)
{
    return fileset::create_with(out, [&](idf::FilesLayout &L) { return idf::make_layout_from_infos(infos, nfiles, image_offsets, L); }, finish_create);
}

void vga_idsp_files_destroy(vga_idsp_files *s) { delete s; }

int vga_idsp_files_totals_of(const vga_idsp_files *s, vga_idsp_files_totals *out)
{
    if (!s || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    *out = s->L.totals;
    return VGA_OK;
}

int vga_idsp_files_offsets(const vga_idsp_files *s, int *first_channel_out, int64_t *image_offsets_out)
{
    if (!s) { set_error("null vga_idsp_files"); return VGA_ERR_ARGUMENT; }
    copy_offsets(s->L, first_channel_out, image_offsets_out);
    return VGA_OK;
}

int vga_idsp_files_gc_files(const vga_idsp_files *s, vga_gc_file *out)
{
    if (!s || (s->L.totals.files > 0 && !out)) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (s->L.from_infos) { set_error("vga_idsp_files_gc_files: the set was made from parsed headers and has no writer configuration"); return VGA_ERR_INVALID_OP; }
    for (int f = 0; f < s->L.totals.files; f++) out[f] = {s->L.tab[f].h.nch, s->L.sample_rate[f], s->L.layout[f].channel};
    return VGA_OK;
}

const vga_gcadpcm_ragged *vga_idsp_files_ragged(const vga_idsp_files *s) { return s ? s->ragged : nullptr; }

int vga_idsp_write_device_v(const vga_idsp_files *s, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *d_gain,
                            const int16_t *d_start_context, const int16_t *d_loop_context, uint8_t *d_images, void *stream)
{
    t_last_launches = 0;
    if (int rc = check_object(s, "vga_idsp_write_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = idf::check_write(s->L, d_adpcm, d_coefs, d_images)) return rc;
    return idf::launch_write_images(s->tables, d_adpcm, d_coefs, d_gain, d_start_context, d_loop_context, d_images, (hipStream_t)stream,
                                    &t_last_launches);
}

int vga_idsp_read_device_v(const vga_idsp_files *s, const uint8_t *d_images, uint8_t *d_adpcm, int16_t *d_coefs, int16_t *d_gain,
                           int16_t *d_start_context, int16_t *d_loop_context, void *stream)
{
    t_last_launches = 0;
    if (int rc = check_object(s, "vga_idsp_read_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = idf::check_read(s->L, d_images, d_adpcm)) return rc;
    return idf::launch_read_images(s->tables, d_images, d_adpcm, d_coefs, d_gain, d_start_context, d_loop_context, (hipStream_t)stream,
                                   &t_last_launches);
}

int vga_idsp_files_write_regions_for(const vga_idsp_file *files, int nfiles, const vga_idsp_file_config *config,
                                     vga_idsp_files_region *regions_out, int64_t capacity, int64_t *count_out)
{
    idf::FilesLayout L;
    if (int rc = idf::make_layout(files, nfiles, config, L)) return rc;
    return idf::copy_regions(L, regions_out, capacity, count_out);
}

int vga_idsp_files_read_regions_for(const vga_idsp_info *const *infos, int nfiles, const int64_t *image_offsets,
                                    vga_idsp_files_region *regions_out, int64_t capacity, int64_t *count_out)
{
    idf::FilesLayout L;
    if (int rc = idf::make_layout_from_infos(infos, nfiles, image_offsets, L)) return rc;
    return idf::copy_regions(L, regions_out, capacity, count_out);
}

int vga_idsp_files_stats(const vga_idsp_files *s, int64_t *out)
{
    if (!s || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    int64_t wide = 0;
    for (const idf::Item &it : s->L.audio_items) wide += it.y >> 31;
    out[0] = (int64_t)s->L.audio_items.size();
    out[1] = wide;
    out[2] = (int64_t)s->block.table_bytes;
    out[3] = t_last_launches;
    return VGA_OK;
}

}  // extern "C"
