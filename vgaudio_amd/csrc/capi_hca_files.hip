// capi_hca_files.hip -- sets of HCA files on the device: the images of every file written and read in one set of launches,
// keys and frame CRCs on the way (include/vgaudio_hip/hca_files.h).  Host side only: checks, layout, headers and work items
// come from hca_files_host.hpp; create uploads the tables the kernels read (hca_files_kernels.hpp) through files_object.hpp
// (DESIGN.md 4.6n), a call checks its pointers and launches.
#include "hca_capi.hpp"
#include "hca_files_object.hpp"

#include <cstring>
#include <vector>

using namespace vga;

thread_local int vga::hcaf::g_force_general = 0; // vga_hca_files_force_general_this_thread

namespace {

using hcaf::check_object;
using hcaf::g_force_general;

// the tables in the current device's memory
int finish_create(vga_hca_files *s)
{
    hcaf::FilesLayout &L = s->L;
    hcak::make_find_tables(L, s->find);
    if (L.totals.files == 0) return VGA_OK;                   // an empty set needs no device
    if (int rc = require_device()) return rc;
    (void)hipGetDevice(&s->block.device);
    fileset::TablePack pack;
    const auto headers = pack.add(L.headers);
    const auto tab = pack.add(L.tab);
    const auto keys = pack.add(L.tables);
    const auto own = pack.add(L.items[0]);
    const auto general = pack.add(L.items[1]);
    const auto walk = pack.add(s->find.walk);
    const auto find = pack.add(s->find.find_files);
    hcaf::DeviceTables &t = s->tables;
    if (int rc = hca::crc_pow_table(&t.crc_pow)) return rc;
    if (int rc = s->block.upload(pack)) return rc;
    const void *d = s->block.d_tables;
    t.headers = pack.at(headers, d);
    t.tab = pack.at(tab, d);
    t.tables = pack.at(keys, d);
    t.items[0] = pack.at(own, d);
    t.items[1] = pack.at(general, d);
    t.files = L.totals.files;
    t.span_items = L.span_items;
    t.item_count[0] = (int)L.items[0].size();
    t.item_count[1] = (int)L.items[1].size();
    t.walk = pack.at(walk, d);
    t.find_files = pack.at(find, d);
    t.find_file_count = (int)s->find.find_files.size();
    t.find_max_channels = s->find.max_channels;
    return VGA_OK;
}

void copy_offsets(const hcaf::FilesLayout &L, int64_t *frame_offsets_out, int64_t *image_offsets_out)
{
    if (frame_offsets_out) std::copy(L.frame_off.begin(), L.frame_off.end(), frame_offsets_out);
    if (image_offsets_out) std::copy(L.image_off.begin(), L.image_off.end(), image_offsets_out);
}

int items_out(const hcaf::FilesLayout &L, int general, vga_hca_files_item *items, int64_t capacity, int64_t *count_out)
{
    std::vector<vga_hca_files_item> v;
    hcaf::describe_items(L, general != 0, v);
    return fileset::copy_capped(v, items, capacity, count_out);
}

}  // namespace

extern "C" {

int vga_hca_files_layout_for(const vga_hca_file *files, int nfiles, const int64_t *frame_offsets, int64_t *frame_offsets_out,
                             int64_t *image_offsets_out, vga_hca_files_totals *totals_out)
{
    if (!frame_offsets_out && !image_offsets_out && !totals_out) { set_error("vga_hca_files_layout_for: no output"); return VGA_ERR_ARGUMENT; }
    hcaf::FilesLayout L;
    if (int rc = hcaf::make_layout(files, nfiles, frame_offsets, nullptr, 0, false, L)) return rc;
    copy_offsets(L, frame_offsets_out, image_offsets_out);
    if (totals_out) *totals_out = L.totals;
    return VGA_OK;
}

int vga_hca_files_create(const vga_hca_file *files, int nfiles, const int64_t *frame_offsets, const uint8_t *tables, int ntables,
                         vga_hca_files **out)
{
    return fileset::create_with(out, [&](hcaf::FilesLayout &L) { return hcaf::make_layout(files, nfiles, frame_offsets, tables, ntables, true, L); },
                                finish_create);
}

int vga_hca_files_create_from_infos(const vga_hca_file_info *const *infos, int nfiles, const int64_t *image_offsets, const int *keys,
                                    const uint8_t *tables, int ntables, const int64_t *frame_offsets, vga_hca_files **out)
{
    return fileset::create_with(out, [&](hcaf::FilesLayout &L) {
        return hcaf::make_layout_from_infos(infos, nfiles, image_offsets, keys, tables, ntables, true, frame_offsets, L);
    }, finish_create);
}

void vga_hca_files_destroy(vga_hca_files *s) { delete s; }

int vga_hca_files_totals_of(const vga_hca_files *s, vga_hca_files_totals *out)
{
    if (!s || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    *out = s->L.totals;
    return VGA_OK;
}

int vga_hca_files_offsets(const vga_hca_files *s, int64_t *frame_offsets_out, int64_t *image_offsets_out)
{
    if (!s) { set_error("null vga_hca_files"); return VGA_ERR_ARGUMENT; }
    copy_offsets(s->L, frame_offsets_out, image_offsets_out);
    return VGA_OK;
}

int vga_hca_write_device_v(const vga_hca_files *s, const uint8_t *d_frames, uint8_t *d_images, void *stream)
{
    if (int rc = check_object(s, "vga_hca_write_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = hcaf::check_write(s->L, d_frames, d_images)) return rc;
    return hcaf::launch_write_images(s->tables, g_force_general != 0, d_frames, d_images, (hipStream_t)stream);
}

int vga_hca_read_device_v(const vga_hca_files *s, const uint8_t *d_images, uint8_t *d_frames, int *d_bad_crc, void *stream)
{
    if (int rc = check_object(s, "vga_hca_read_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = hcaf::check_read(s->L, d_images, d_frames)) return rc;
    return hcaf::launch_read_images(s->tables, g_force_general != 0, d_images, d_frames, d_bad_crc, (hipStream_t)stream);
}

// ---- hooks
int vga_hca_files_write_items_for(const vga_hca_file *files, int nfiles, const int64_t *frame_offsets, int general,
                                  vga_hca_files_item *items, int64_t capacity, int64_t *count_out)
{
    hcaf::FilesLayout L;
    if (int rc = hcaf::make_layout(files, nfiles, frame_offsets, nullptr, 0, false, L)) return rc;
    return items_out(L, general, items, capacity, count_out);
}

int vga_hca_files_read_items_for(const vga_hca_file_info *const *infos, int nfiles, const int64_t *image_offsets,
                                 const int64_t *frame_offsets, int general, vga_hca_files_item *items, int64_t capacity, int64_t *count_out)
{
    hcaf::FilesLayout L;
    if (int rc = hcaf::make_layout_from_infos(infos, nfiles, image_offsets, nullptr, nullptr, 0, false, frame_offsets, L)) return rc;
    return items_out(L, general, items, capacity, count_out);
}

int vga_hca_files_stats(const vga_hca_files *s, int64_t *out)
{
    if (!s || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    const hcaf::FilesLayout &L = s->L;
    const bool general = g_force_general != 0;
    out[0] = general ? 0 : L.span_files;
    out[1] = general ? L.moving_files : L.general_files;
    out[2] = general ? 0 : L.span_items;
    out[3] = (int64_t)L.items[general ? 1 : 0].size() - out[2];
    return VGA_OK;
}

int vga_hca_files_force_general_this_thread(int on)
{
    const int old = g_force_general;
    g_force_general = on ? 1 : 0;
    return old;
}

}  // extern "C"
