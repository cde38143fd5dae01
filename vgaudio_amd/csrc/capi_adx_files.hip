// capi_adx_files.hip -- sets of ADX files on the device: the images of every file written and read in one set of launches
// (include/vgaudio_hip/adx_files.h).  Host side only: checks, layout and work items come from adx_files_host.hpp; create
// uploads the tables the kernels read (adx_files_kernels.hpp) through files_object.hpp, a call checks its
// pointers and launches.
#include "adx_files_object.hpp"

#include <cstring>
#include <vector>

using namespace vga;

thread_local int vga::adxf::g_force_general = 0;  // vga_adx_files_force_general_this_thread

namespace {

using adxf::check_object;
using adxf::g_force_general;

// the tables in the current device's memory
int finish_create(vga_adx_files *s)
{
    adxf::FilesLayout &L = s->L;
    if (L.totals.files == 0) return VGA_OK;                   // an empty set needs no device
    if (int rc = require_device()) return rc;
    (void)hipGetDevice(&s->block.device);
    fileset::TablePack pack;
    const auto tab = pack.add(L.tab);
    const auto rows = pack.add(L.row_off);
    const auto file = pack.add(L.row_file);
    const auto hist = pack.add(L.history);
    const auto own = pack.add(L.items[0]);
    const auto general = pack.add(L.items[1]);
    const auto cipher_own = pack.add(L.cipher_items[0]);
    const auto cipher_general = pack.add(L.cipher_items[1]);
    const auto find = pack.add(L.find_items);
    if (int rc = s->block.upload(pack)) return rc;
    const void *d = s->block.d_tables;
    adxf::DeviceTables &t = s->tables;
    t.tab = pack.at(tab, d);
    t.row_off = pack.at(rows, d);
    t.row_file = pack.at(file, d);
    t.history = pack.at(hist, d);
    t.items[0] = pack.at(own, d);
    t.items[1] = pack.at(general, d);
    t.files = L.totals.files;
    t.channels = L.totals.channels;
    t.span_items = L.span_items;
    t.item_count[0] = (int)L.items[0].size();
    t.item_count[1] = (int)L.items[1].size();
    t.cipher_items[0] = pack.at(cipher_own, d);
    t.cipher_items[1] = pack.at(cipher_general, d);
    t.find_items = pack.at(find, d);
    t.cipher_count[0] = (int)L.cipher_items[0].size();
    t.cipher_count[1] = (int)L.cipher_items[1].size();
    t.find_count = (int)L.find_items.size();
    return VGA_OK;
}

void copy_offsets(const adxf::FilesLayout &L, int *first_channel_out, int64_t *audio_offsets_out, int64_t *image_offsets_out)
{
    if (first_channel_out) std::copy(L.first_channel.begin(), L.first_channel.end(), first_channel_out);
    if (audio_offsets_out) std::copy(L.row_off.begin(), L.row_off.end(), audio_offsets_out);
    if (image_offsets_out) std::copy(L.image_off.begin(), L.image_off.end(), image_offsets_out);
}

int items_out(const adxf::FilesLayout &L, int general, vga_adx_files_item *items, int64_t capacity, int64_t *count_out)
{
    std::vector<vga_adx_files_item> v;
    adxf::describe_items(L, general != 0, v);
    return fileset::copy_capped(v, items, capacity, count_out);
}

}  // namespace

extern "C" {

int vga_adx_files_layout_for(const vga_adx_file *files, int nfiles, const int64_t *audio_offsets, int *first_channel_out,
                             int64_t *audio_offsets_out, int64_t *image_offsets_out, vga_adx_files_totals *totals_out)
{
    if (!first_channel_out && !audio_offsets_out && !image_offsets_out && !totals_out) { set_error("vga_adx_files_layout_for: no output"); return VGA_ERR_ARGUMENT; }
    adxf::FilesLayout L;
    if (int rc = adxf::make_layout(files, nfiles, audio_offsets, L)) return rc;
    copy_offsets(L, first_channel_out, audio_offsets_out, image_offsets_out);
    if (totals_out) *totals_out = L.totals;
    return VGA_OK;
}

int vga_adx_files_create(const vga_adx_file *files, int nfiles, const int64_t *audio_offsets, vga_adx_files **out)
{
    return fileset::create_with(out, [&](adxf::FilesLayout &L) { return adxf::make_layout(files, nfiles, audio_offsets, L); }, finish_create);
}

int vga_adx_files_create_from_infos(const vga_adx_file_info *const *infos, int nfiles, const int64_t *image_offsets, vga_adx_files **out)
{
    return fileset::create_with(out, [&](adxf::FilesLayout &L) { return adxf::make_layout_from_infos(infos, nfiles, image_offsets, L); },
                                finish_create);
}

void vga_adx_files_destroy(vga_adx_files *s) { delete s; }

int vga_adx_files_totals_of(const vga_adx_files *s, vga_adx_files_totals *out)
{
    if (!s || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    *out = s->L.totals;
    return VGA_OK;
}

int vga_adx_files_offsets(const vga_adx_files *s, int *first_channel_out, int64_t *audio_offsets_out, int64_t *image_offsets_out)
{
    if (!s) { set_error("null vga_adx_files"); return VGA_ERR_ARGUMENT; }
    copy_offsets(s->L, first_channel_out, audio_offsets_out, image_offsets_out);
    return VGA_OK;
}

int vga_adx_write_device_v(const vga_adx_files *s, const uint8_t *d_audio, const int16_t *d_history, uint8_t *d_images, void *stream)
{
    if (int rc = check_object(s, "vga_adx_write_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = adxf::check_write(s->L, d_audio, d_history, d_images)) return rc;
    return adxf::launch_write_images(s->tables, g_force_general != 0, d_audio, d_history, d_images, (hipStream_t)stream);
}

int vga_adx_read_device_v(const vga_adx_files *s, const uint8_t *d_images, uint8_t *d_audio, int16_t *d_history_out, void *stream)
{
    if (int rc = check_object(s, "vga_adx_read_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = adxf::check_read(s->L, d_images, d_audio)) return rc;
    return adxf::launch_read_images(s->tables, g_force_general != 0, d_images, d_audio, d_history_out, (hipStream_t)stream);
}

// ---- hooks
int vga_adx_files_write_items_for(const vga_adx_file *files, int nfiles, const int64_t *audio_offsets, int general,
                                  vga_adx_files_item *items, int64_t capacity, int64_t *count_out)
{
    adxf::FilesLayout L;
    if (int rc = adxf::make_layout(files, nfiles, audio_offsets, L)) return rc;
    return items_out(L, general, items, capacity, count_out);
}

int vga_adx_files_read_items_for(const vga_adx_file_info *const *infos, int nfiles, const int64_t *image_offsets, int general,
                                 vga_adx_files_item *items, int64_t capacity, int64_t *count_out)
{
    adxf::FilesLayout L;
    if (int rc = adxf::make_layout_from_infos(infos, nfiles, image_offsets, L)) return rc;
    return items_out(L, general, items, capacity, count_out);
}

int vga_adx_files_stats(const vga_adx_files *s, int64_t *out)
{
    if (!s || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    const adxf::FilesLayout &L = s->L;
    const bool general = g_force_general != 0;
    out[0] = general ? 0 : L.span_files;
    out[1] = general ? L.moving_files : L.general_files;
    out[2] = general ? 0 : L.span_items;
    out[3] = (int64_t)L.items[general ? 1 : 0].size() - out[2];
    return VGA_OK;
}

int vga_adx_files_force_general_this_thread(int on)
{
    const int old = g_force_general;
    g_force_general = on ? 1 : 0;
    return old;
}

}  // extern "C"
