// capi_hps_files.hip -- sets of HPS files on the device: the images of every file written and read in one set of launches
// (include/vgaudio_hip_files/hps_files.h).  Host side only: checks, layout, the block table and the work items come from
// hps_files_host.hpp; create uploads the tables the kernels read (hps_files_kernels.hpp) through files_object.hpp
// (DESIGN.md 4.6n), a call checks its pointers and launches.
#include "files_object.hpp"
#include "hps_files_kernels.hpp"

#include <cstring>
#include <vector>

using namespace vga;

struct vga_hps_files {
    static constexpr const char *type_name = "vga_hps_files";
    hpf::FilesLayout L;
    vga_gcadpcm_ragged *ragged = nullptr;
    fileset::TableBlock block;
    hpf::DeviceTables tables;
    int files() const { return L.totals.files; }
    ~vga_hps_files()
    {
        if (ragged) vga_gcadpcm_ragged_destroy(ragged);
    }
};

namespace {

using fileset::check_object;

thread_local int t_last_launches = 0;            // of this thread's last _v call (vga_hps_files_stats): cleared as the call begins

// the ragged batch of the rows and the tables in the current device's memory
int finish_create(vga_hps_files *s)
{
    hpf::FilesLayout &L = s->L;
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
    const auto blocks = pack.add(L.blocks);
    const auto items = pack.add(L.items);
    if (int rc = s->block.upload(pack)) return rc;
    const void *d = s->block.d_tables;
    s->tables.tab = pack.at(tab, d);
    s->tables.rows = pack.at(rows, d);
    s->tables.meta = pack.at(meta, d);
    s->tables.blocks = pack.at(blocks, d);
    s->tables.items = pack.at(items, d);
    s->tables.files = L.totals.files;
    s->tables.channels = (int)L.channel.size();
    s->tables.blocks_n = (int)L.blocks.size();
    s->tables.items_n = (int)L.items.size();
    return VGA_OK;
}

void copy_offsets(const hpf::FilesLayout &L, int *first_channel_out, int64_t *image_offsets_out, int64_t *first_block_out)
{
    if (first_channel_out) std::copy(L.first_channel.begin(), L.first_channel.end(), first_channel_out);
    if (image_offsets_out) std::copy(L.image_off.begin(), L.image_off.end(), image_offsets_out);
    if (first_block_out) std::copy(L.first_block.begin(), L.first_block.end(), first_block_out);
}

}  // namespace

extern "C" {

int vga_hps_files_layout_for(const vga_hps_file *files, int nfiles, int *first_channel_out, int64_t *image_offsets_out,
                             int64_t *first_block_out, vga_hps_files_totals *totals_out)
{
    if (!first_channel_out && !image_offsets_out && !first_block_out && !totals_out) { set_error("vga_hps_files_layout_for: no output"); return VGA_ERR_ARGUMENT; }
    hpf::FilesLayout L;
    if (int rc = hpf::make_layout(files, nfiles, L)) return rc;
    copy_offsets(L, first_channel_out, image_offsets_out, first_block_out);
    if (totals_out) *totals_out = L.totals;
    return VGA_OK;
}

int vga_hps_files_create(const vga_hps_file *files, int nfiles, vga_hps_files **out)
{
    return fileset::create_with(out, [&](hpf::FilesLayout &L) { return hpf::make_layout(files, nfiles, L); }, finish_create);
}

int vga_hps_files_create_from_infos(const vga_hps_info *const *infos, const vga_hps_block_info *const *blocks_per_file, int nfiles,
                                    const int64_t *image_offsets, vga_hps_files **out)
{
    return fileset::create_with(out, [&](hpf::FilesLayout &L) { return hpf::make_layout_from_infos(infos, blocks_per_file, nfiles, image_offsets, L); },
                                finish_create);
}

void vga_hps_files_destroy(vga_hps_files *s) { delete s; }

int vga_hps_files_totals_of(const vga_hps_files *s, vga_hps_files_totals *out)
{
    if (!s || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    *out = s->L.totals;
    return VGA_OK;
}

int vga_hps_files_offsets(const vga_hps_files *s, int *first_channel_out, int64_t *image_offsets_out, int64_t *first_block_out)
{
    if (!s) { set_error("null vga_hps_files"); return VGA_ERR_ARGUMENT; }
    copy_offsets(s->L, first_channel_out, image_offsets_out, first_block_out);
    return VGA_OK;
}

int vga_hps_files_gc_files(const vga_hps_files *s, vga_gc_file *out)
{
    if (!s || (s->L.totals.files > 0 && !out)) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (s->L.from_infos) { set_error("vga_hps_files_gc_files: the set was made from parsed headers and has no writer configuration"); return VGA_ERR_INVALID_OP; }
    for (int f = 0; f < s->L.totals.files; f++) out[f] = {s->L.nch[f], s->L.sample_rate[f], s->L.layout[f].channel};
    return VGA_OK;
}

const vga_gcadpcm_ragged *vga_hps_files_ragged(const vga_hps_files *s) { return s ? s->ragged : nullptr; }

int vga_hps_write_device_v(const vga_hps_files *s, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *d_gain,
                           const int16_t *d_start_context, const int16_t *d_pcm, uint8_t *d_images, void *stream)
{
    t_last_launches = 0;
    if (int rc = check_object(s, "vga_hps_write_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = hpf::check_write(s->L, d_adpcm, d_coefs, d_pcm, d_images)) return rc;
    return hpf::launch_write_images(s->tables, d_adpcm, d_coefs, d_gain, d_start_context, d_pcm, d_images, (hipStream_t)stream,
                                    &t_last_launches);
}

int vga_hps_read_device_v(const vga_hps_files *s, const uint8_t *d_images, uint8_t *d_adpcm, int16_t *d_coefs, int16_t *d_gain,
                          int16_t *d_start_context, int16_t *d_loop_context, void *stream)
{
    t_last_launches = 0;
    if (int rc = check_object(s, "vga_hps_read_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = hpf::check_read(s->L, d_images, d_adpcm)) return rc;
    return hpf::launch_read_images(s->tables, d_images, d_adpcm, d_coefs, d_gain, d_start_context, d_loop_context, (hipStream_t)stream,
                                   &t_last_launches);
}

int vga_hps_files_write_regions_for(const vga_hps_file *files, int nfiles, vga_hps_files_region *regions_out, int64_t capacity,
                                    int64_t *count_out)
{
    hpf::FilesLayout L;
    if (int rc = hpf::make_layout(files, nfiles, L)) return rc;
    return hpf::copy_regions(L, regions_out, capacity, count_out);
}

int vga_hps_files_read_regions_for(const vga_hps_info *const *infos, const vga_hps_block_info *const *blocks_per_file, int nfiles,
                                   const int64_t *image_offsets, vga_hps_files_region *regions_out, int64_t capacity, int64_t *count_out)
{
    hpf::FilesLayout L;
    if (int rc = hpf::make_layout_from_infos(infos, blocks_per_file, nfiles, image_offsets, L)) return rc;
    return hpf::copy_regions(L, regions_out, capacity, count_out);
}

int vga_hps_files_stats(const vga_hps_files *s, int64_t *out)
{
    if (!s || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    out[0] = (int64_t)s->L.items.size();
    out[1] = (int64_t)s->L.blocks.size();
    out[2] = (int64_t)s->block.table_bytes;
    out[3] = t_last_launches;
    return VGA_OK;
}

}  // extern "C"
