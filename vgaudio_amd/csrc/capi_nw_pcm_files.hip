// capi_nw_pcm_files.hip -- sets of PCM16 / PCM8 NintendoWare stream files on the device: the images of every file written from
// planar int16 rows and read into them in one set of launches (include/vgaudio_hip_files/nw_pcm_files.h).  Host side only:
// checks, layout and work items come from nw_pcm_files_host.hpp; create uploads the tables the kernels read
// (nw_pcm_files_kernels.hpp) through files_object.hpp, a call checks its pointers and launches.
#include "files_object.hpp"
#include "nw_pcm_files_kernels.hpp"

#include <cstring>
#include <vector>

using namespace vga;

struct vga_nw_pcm_files {
    static constexpr const char *type_name = "vga_nw_pcm_files";
    nwpf::FilesLayout L;
    fileset::TableBlock block;
    nwpf::DeviceTables tables;
    int files() const { return L.P.totals.files; }
};

namespace {

using fileset::check_object;

thread_local int g_force_general = 0;            // vga_nw_pcm_files_force_general_this_thread

// the tables in the current device's memory, through the library's allocator
int finish_create(vga_nw_pcm_files *s)
{
    nwpf::FilesLayout &L = s->L;
    if (L.P.totals.files == 0) return VGA_OK;                 // an empty set needs no device
    if (int rc = require_device()) return rc;
    (void)hipGetDevice(&s->block.device);
    fileset::TablePack pack;
    const auto tab = pack.add(L.tab);
    const auto rows = pack.add(L.P.row_off);
    const auto file = pack.add(L.P.row_file);
    const auto own = pack.add(L.items[0]);
    const auto general = pack.add(L.items[1]);
    if (int rc = s->block.upload(pack)) return rc;
    const void *d = s->block.d_tables;
    nwpf::DeviceTables &t = s->tables;
    t.tab = pack.at(tab, d);
    t.row_off = pack.at(rows, d);
    t.row_file = pack.at(file, d);
    t.items[0] = pack.at(own, d);
    t.items[1] = pack.at(general, d);
    t.files = L.P.totals.files;
    t.channels = L.P.totals.channels;
    t.vector_items = L.vector_items;
    t.item_count[0] = (int)L.items[0].size();
    t.item_count[1] = (int)L.items[1].size();
    return VGA_OK;
}

vga_nw_pcm_files_totals totals_of(const nwpf::FilesLayout &L)
{
    return {L.P.totals.files, L.P.totals.channels, L.P.totals.pcm_samples, L.P.totals.image_bytes};
}

void copy_offsets(const nwpf::FilesLayout &L, int *first_channel_out, int64_t *pcm_offsets_out, int64_t *image_offsets_out)
{
    if (first_channel_out) std::copy(L.P.first_channel.begin(), L.P.first_channel.end(), first_channel_out);
    if (pcm_offsets_out) std::copy(L.P.row_off.begin(), L.P.row_off.end(), pcm_offsets_out);
    if (image_offsets_out) std::copy(L.P.image_off.begin(), L.P.image_off.end(), image_offsets_out);
}

int items_out(const nwpf::FilesLayout &L, int general, vga_nw_pcm_files_item *items, int64_t capacity, int64_t *count_out)
{
    std::vector<vga_nw_pcm_files_item> v;
    nwpf::describe_items(L, general != 0, v);
    return fileset::copy_capped(v, items, capacity, count_out);
}

}  // namespace

extern "C" {

int vga_nw_pcm_files_layout_for(const vga_nw_file *files, int nfiles, const vga_nw_file_config *config, int codec, const int64_t *pcm_offsets,
                                const int64_t *image_offsets, int *first_channel_out, int64_t *pcm_offsets_out, int64_t *image_offsets_out,
                                vga_nw_pcm_files_totals *totals_out)
{
    if (!first_channel_out && !pcm_offsets_out && !image_offsets_out && !totals_out) { set_error("vga_nw_pcm_files_layout_for: no output"); return VGA_ERR_ARGUMENT; }
    nwpf::FilesLayout L;
    if (int rc = nwpf::make_layout(files, nfiles, config, codec, pcm_offsets, image_offsets, L)) return rc;
    copy_offsets(L, first_channel_out, pcm_offsets_out, image_offsets_out);
    if (totals_out) *totals_out = totals_of(L);
    return VGA_OK;
}

int vga_nw_pcm_files_create(const vga_nw_file *files, int nfiles, const vga_nw_file_config *config, int codec, const int64_t *pcm_offsets,
                            const int64_t *image_offsets, vga_nw_pcm_files **out)
{
    return fileset::create_with(out, [&](nwpf::FilesLayout &L) { return nwpf::make_layout(files, nfiles, config, codec, pcm_offsets, image_offsets, L); },
                                finish_create);
}

int vga_nw_pcm_files_create_from_infos(const vga_nwstm_info *const *infos, int nfiles, const int64_t *pcm_offsets, const int64_t *image_offsets,
                                       vga_nw_pcm_files **out)
{
    return fileset::create_with(out, [&](nwpf::FilesLayout &L) { return nwpf::make_layout_from_infos(infos, nfiles, pcm_offsets, image_offsets, L); },
                                finish_create);
}

void vga_nw_pcm_files_destroy(vga_nw_pcm_files *s) { delete s; }

int vga_nw_pcm_files_totals_of(const vga_nw_pcm_files *s, vga_nw_pcm_files_totals *out)
{
    if (!s || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    *out = totals_of(s->L);
    return VGA_OK;
}

int vga_nw_pcm_files_offsets(const vga_nw_pcm_files *s, int *first_channel_out, int64_t *pcm_offsets_out, int64_t *image_offsets_out)
{
    if (!s) { set_error("null vga_nw_pcm_files"); return VGA_ERR_ARGUMENT; }
    copy_offsets(s->L, first_channel_out, pcm_offsets_out, image_offsets_out);
    return VGA_OK;
}

int vga_nwstm_pcm_write_device_v(const vga_nw_pcm_files *s, const int16_t *d_pcm, uint8_t *d_images, void *stream)
{
    if (int rc = check_object(s, "vga_nwstm_pcm_write_device_v")) return rc;
    if (s->L.P.totals.files == 0) return VGA_OK;
    if (int rc = nwpf::check_write(s->L, d_pcm, d_images)) return rc;
    const bool general = g_force_general != 0 || !nwpf::bases_aligned(d_pcm, d_images);
    return nwpf::launch_write_images(s->tables, general, d_pcm, d_images, (hipStream_t)stream);
}

int vga_nwstm_pcm_read_device_v(const vga_nw_pcm_files *s, const uint8_t *d_images, int16_t *d_pcm, void *stream)
{
    if (int rc = check_object(s, "vga_nwstm_pcm_read_device_v")) return rc;
    if (s->L.P.totals.files == 0) return VGA_OK;
    if (int rc = nwpf::check_read(s->L, d_images, d_pcm)) return rc;
    const bool general = g_force_general != 0 || !nwpf::bases_aligned(d_pcm, d_images);
    return nwpf::launch_read_images(s->tables, general, d_images, d_pcm, (hipStream_t)stream);
}

// ---- hooks
int vga_nw_pcm_files_write_items_for(const vga_nw_file *files, int nfiles, const vga_nw_file_config *config, int codec, const int64_t *pcm_offsets,
                                     const int64_t *image_offsets, int general, vga_nw_pcm_files_item *items, int64_t capacity, int64_t *count_out)
{
    nwpf::FilesLayout L;
    if (int rc = nwpf::make_layout(files, nfiles, config, codec, pcm_offsets, image_offsets, L)) return rc;
    return items_out(L, general, items, capacity, count_out);
}

int vga_nw_pcm_files_read_items_for(const vga_nwstm_info *const *infos, int nfiles, const int64_t *pcm_offsets, const int64_t *image_offsets,
                                    int general, vga_nw_pcm_files_item *items, int64_t capacity, int64_t *count_out)
{
    nwpf::FilesLayout L;
    if (int rc = nwpf::make_layout_from_infos(infos, nfiles, pcm_offsets, image_offsets, L)) return rc;
    return items_out(L, general, items, capacity, count_out);
}

int vga_nw_pcm_files_stats(const vga_nw_pcm_files *s, int64_t *out)
{
    if (!s || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    const nwpf::FilesLayout &L = s->L;
    const bool general = g_force_general != 0;
    out[0] = general ? 0 : L.vector_files;
    out[1] = general ? L.moving_files : L.general_files;
    out[2] = general ? 0 : L.vector_items;
    out[3] = (int64_t)L.items[general ? 1 : 0].size() - out[2];
    return VGA_OK;
}

int vga_nw_pcm_files_force_general_this_thread(int on)
{
    const int old = g_force_general;
    g_force_general = on ? 1 : 0;
    return old;
}

}  // extern "C"
