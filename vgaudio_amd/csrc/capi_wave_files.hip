// capi_wave_files.hip -- sets of WAVE files on the device: the data chunks of every file read into planar rows and the
// images written from them in one set of launches (include/vgaudio_hip_files/wave_files.h).  Host side only: checks, layout,
// headers and work items come from wave_files_host.hpp; create uploads the tables the kernels read (wave_files_kernels.hpp)
// through files_object.hpp, a call checks its pointers and launches.
#include "files_object.hpp"
#include "wave_files_kernels.hpp"

#include <cstring>
#include <vector>

using namespace vga;

struct vga_wave_files {
    static constexpr const char *type_name = "vga_wave_files";
    wavf::FilesLayout L;
    fileset::TableBlock block;
    wavf::DeviceTables tables;
    int files() const { return L.totals.files; }
};

namespace {

using fileset::check_object;

thread_local int g_force_general = 0;            // vga_wave_files_force_general_this_thread

// the tables in the current device's memory
int finish_create(vga_wave_files *s)
{
    wavf::FilesLayout &L = s->L;
    if (L.totals.files == 0) return VGA_OK;                   // an empty set needs no device
    if (int rc = require_device()) return rc;
    (void)hipGetDevice(&s->block.device);
    fileset::TablePack pack;
    const auto tab = pack.add(L.tab);
    const auto rows = pack.add(L.row_off);
    const auto file = pack.add(L.row_file);
    const auto headers = pack.add(L.headers);
    const auto own = pack.add(L.items[0]);
    const auto general = pack.add(L.items[1]);
    if (int rc = s->block.upload(pack)) return rc;
    const void *d = s->block.d_tables;
    wavf::DeviceTables &t = s->tables;
    t.tab = pack.at(tab, d);
    t.row_off = pack.at(rows, d);
    t.row_file = pack.at(file, d);
    t.headers = pack.at(headers, d);
    t.items[0] = pack.at(own, d);
    t.items[1] = pack.at(general, d);
    t.files = L.totals.files;
    t.channels = L.totals.channels;
    t.tile_items = L.tile_items;
    t.item_count[0] = (int)L.items[0].size();
    t.item_count[1] = (int)L.items[1].size();
    return VGA_OK;
}

void copy_offsets(const wavf::FilesLayout &L, int *first_channel_out, int64_t *pcm_offsets_out, int64_t *image_offsets_out)
{
    if (first_channel_out) std::copy(L.first_channel.begin(), L.first_channel.end(), first_channel_out);
    if (pcm_offsets_out) std::copy(L.row_off.begin(), L.row_off.end(), pcm_offsets_out);
    if (image_offsets_out) std::copy(L.image_off.begin(), L.image_off.end(), image_offsets_out);
}

int items_out(const wavf::FilesLayout &L, int general, vga_wave_files_item *items, int64_t capacity, int64_t *count_out)
{
    std::vector<vga_wave_files_item> v;
    wavf::describe_items(L, general != 0, v);
    return fileset::copy_capped(v, items, capacity, count_out);
}

}  // namespace

extern "C" {

int vga_wave_files_layout_for(const vga_wave_file *files, int nfiles, const int64_t *pcm_offsets, const int64_t *image_offsets,
                              int *first_channel_out, int64_t *pcm_offsets_out, int64_t *image_offsets_out, vga_wave_files_totals *totals_out)
{
    if (!first_channel_out && !pcm_offsets_out && !image_offsets_out && !totals_out) { set_error("vga_wave_files_layout_for: no output"); return VGA_ERR_ARGUMENT; }
    wavf::FilesLayout L;
    if (int rc = wavf::make_layout(files, nfiles, pcm_offsets, image_offsets, L)) return rc;
    copy_offsets(L, first_channel_out, pcm_offsets_out, image_offsets_out);
    if (totals_out) *totals_out = L.totals;
    return VGA_OK;
}

int vga_wave_files_create(const vga_wave_file *files, int nfiles, const int64_t *pcm_offsets, const int64_t *image_offsets, vga_wave_files **out)
{
    return fileset::create_with(out, [&](wavf::FilesLayout &L) { return wavf::make_layout(files, nfiles, pcm_offsets, image_offsets, L); }, finish_create);
}

int vga_wave_files_create_from_infos(const vga_wave_info *const *infos, int nfiles, const int64_t *pcm_offsets, const int64_t *image_offsets,
                                     vga_wave_files **out)
{
    return fileset::create_with(out, [&](wavf::FilesLayout &L) { return wavf::make_layout_from_infos(infos, nfiles, pcm_offsets, image_offsets, L); },
                                finish_create);
}

void vga_wave_files_destroy(vga_wave_files *s) { delete s; }

int vga_wave_files_totals_of(const vga_wave_files *s, vga_wave_files_totals *out)
{
    if (!s || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    *out = s->L.totals;
    return VGA_OK;
}

int vga_wave_files_offsets(const vga_wave_files *s, int *first_channel_out, int64_t *pcm_offsets_out, int64_t *image_offsets_out)
{
    if (!s) { set_error("null vga_wave_files"); return VGA_ERR_ARGUMENT; }
    copy_offsets(s->L, first_channel_out, pcm_offsets_out, image_offsets_out);
    return VGA_OK;
}

int vga_wave_read_device_v(const vga_wave_files *s, const uint8_t *d_images, int16_t *d_pcm, void *stream)
{
    if (int rc = check_object(s, "vga_wave_read_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = wavf::check_read(s->L, d_images, d_pcm)) return rc;
    return wavf::launch_read_images(s->tables, g_force_general != 0, d_images, d_pcm, (hipStream_t)stream);
}

int vga_wave_write_device_v(const vga_wave_files *s, const int16_t *d_pcm, uint8_t *d_images, void *stream)
{
    if (int rc = check_object(s, "vga_wave_write_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = wavf::check_write(s->L, d_pcm, d_images)) return rc;
    return wavf::launch_write_images(s->tables, g_force_general != 0, d_pcm, d_images, (hipStream_t)stream);
}

// ---- hooks
int vga_wave_files_write_items_for(const vga_wave_file *files, int nfiles, const int64_t *pcm_offsets, const int64_t *image_offsets, int general,
                                   vga_wave_files_item *items, int64_t capacity, int64_t *count_out)
{
    wavf::FilesLayout L;
    if (int rc = wavf::make_layout(files, nfiles, pcm_offsets, image_offsets, L)) return rc;
    return items_out(L, general, items, capacity, count_out);
}

int vga_wave_files_read_items_for(const vga_wave_info *const *infos, int nfiles, const int64_t *pcm_offsets, const int64_t *image_offsets,
                                  int general, vga_wave_files_item *items, int64_t capacity, int64_t *count_out)
{
    wavf::FilesLayout L;
    if (int rc = wavf::make_layout_from_infos(infos, nfiles, pcm_offsets, image_offsets, L)) return rc;
    return items_out(L, general, items, capacity, count_out);
}

int vga_wave_files_stats(const vga_wave_files *s, int64_t *out)
{
    if (!s || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    const wavf::FilesLayout &L = s->L;
    const bool general = g_force_general != 0;
    out[0] = general ? 0 : L.tile_files;
    out[1] = general ? L.moving_files : L.general_files;
    out[2] = general ? 0 : L.tile_items;
    out[3] = (int64_t)L.items[general ? 1 : 0].size() - out[2];
    return VGA_OK;
}

int vga_wave_files_force_general_this_thread(int on)
{
    const int old = g_force_general;
    g_force_general = on ? 1 : 0;
    return old;
}

}  // extern "C"
