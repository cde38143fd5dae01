// capi_hps_files.hip -- sets of HPS files on the device: the images of every file written and read in one set of launches
// (include/vgaudio_hip_files/hps_files.h).  Host side only: checks, layout, the block table and the work items come from
// hps_files_host.hpp; create uploads the tables the kernels read (hps_files_kernels.hpp), a call checks its pointers and
// launches.
#include "common.hpp"
#include "hps_files_kernels.hpp"

#include <cstring>
#include <vector>

using namespace vga;

struct vga_hps_files {
    hpf::FilesLayout L;
    vga_gcadpcm_ragged *ragged = nullptr;
    void *d_tables = nullptr;
    size_t table_bytes = 0;
    hpf::DeviceTables tables;
    int device = 0;
    ~vga_hps_files()
    {
        if (ragged) vga_gcadpcm_ragged_destroy(ragged);
        if (d_tables) (void)hipFree(d_tables);
    }
};

namespace {

thread_local int t_last_launches = 0;            // of this thread's last _v call (vga_hps_files_stats)

template <class T> size_t place(size_t &at, const std::vector<T> &v)
{
    const size_t here = at;
    at += (size_t)round_up((int64_t)(v.size() * sizeof(T)), 16);
    return here;
}
template <class T> void fill(std::vector<unsigned char> &host, size_t at, const std::vector<T> &v)
{
    if (!v.empty()) memcpy(host.data() + at, v.data(), v.size() * sizeof(T));
}

// the ragged batch of the rows and the tables in the current device's memory
int finish_create(vga_hps_files *s)
{
    hpf::FilesLayout &L = s->L;
    if (L.totals.files == 0) {                                  // an empty set needs no device; with one it has its (empty) batch
        if (vga_gcadpcm_ragged_create(nullptr, 0, &s->ragged) != VGA_OK) s->ragged = nullptr;
        return VGA_OK;
    }
    if (int rc = require_device()) return rc;
    (void)hipGetDevice(&s->device);
    if (int rc = vga_gcadpcm_ragged_create(L.counts.data(), (int)L.counts.size(), &s->ragged)) return rc;
    if (vga_gcadpcm_ragged_pcm_samples(s->ragged) != L.totals.pcm_samples || vga_gcadpcm_ragged_adpcm_bytes(s->ragged) != L.totals.adpcm_bytes) {
        set_error("internal: the set's rows are not the ragged batch's");
        return VGA_ERR_DEVICE;
    }
    size_t bytes = 0;
    const size_t tab_at = place(bytes, L.tab), rows_at = place(bytes, L.channel), meta_at = place(bytes, L.meta);
    const size_t blocks_at = place(bytes, L.blocks), items_at = place(bytes, L.items);
    std::vector<unsigned char> host(bytes + 16, 0);
    fill(host, tab_at, L.tab);
    fill(host, rows_at, L.channel);
    fill(host, meta_at, L.meta);
    fill(host, blocks_at, L.blocks);
    fill(host, items_at, L.items);
    VGA_HIP_TRY(device_malloc(&s->d_tables, host.size()));
    VGA_HIP_TRY(hipMemcpy(s->d_tables, host.data(), host.size(), hipMemcpyHostToDevice));
    s->table_bytes = host.size();
    const unsigned char *d = static_cast<const unsigned char *>(s->d_tables);
    s->tables.tab = reinterpret_cast<const hpf::FileTab *>(d + tab_at);
    s->tables.rows = reinterpret_cast<const hpf::Row *>(d + rows_at);
    s->tables.meta = reinterpret_cast<const hpf::ChannelMeta *>(d + meta_at);
    s->tables.blocks = reinterpret_cast<const hpf::Block *>(d + blocks_at);
    s->tables.items = reinterpret_cast<const hpf::Item *>(d + items_at);
    s->tables.files = L.totals.files;
    s->tables.channels = (int)L.channel.size();
    s->tables.blocks_n = (int)L.blocks.size();
    s->tables.items_n = (int)L.items.size();
    return VGA_OK;
}

int check_object(const vga_hps_files *s, const char *what)
{
    t_last_launches = 0;
    if (!s) { set_error("%s: null vga_hps_files", what); return VGA_ERR_ARGUMENT; }
    int device = -1;
    if (s->L.totals.files > 0) (void)hipGetDevice(&device);
    if (s->L.totals.files > 0 && device != s->device) {
        set_error("%s: the set was created on device %d, the current one is %d", what, s->device, device);
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}

void copy_offsets(const hpf::FilesLayout &L, int *first_channel_out, int64_t *image_offsets_out, int64_t *first_block_out)
{
    if (first_channel_out) std::copy(L.first_channel.begin(), L.first_channel.end(), first_channel_out);
    if (image_offsets_out) std::copy(L.image_off.begin(), L.image_off.end(), image_offsets_out);
    if (first_block_out) std::copy(L.first_block.begin(), L.first_block.end(), first_block_out);
}

template <class Make> int create_with(vga_hps_files **out, Make &&make)
{
    if (!out) { set_error("null output"); return VGA_ERR_ARGUMENT; }
    *out = nullptr;
    vga_hps_files *s = new vga_hps_files;
    int rc = make(s->L);
    if (!rc) rc = finish_create(s);
    if (rc) {
        delete s;
        return rc;
    }
    *out = s;
    return VGA_OK;
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
    return create_with(out, [&](hpf::FilesLayout &L) { return hpf::make_layout(files, nfiles, L); });
}

int vga_hps_files_create_from_infos(const vga_hps_info *const *infos, const vga_hps_block_info *const *blocks_per_file, int nfiles,
                                    const int64_t *image_offsets, vga_hps_files **out)
{
    return create_with(out, [&](hpf::FilesLayout &L) { return hpf::make_layout_from_infos(infos, blocks_per_file, nfiles, image_offsets, L); });
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
    if (int rc = check_object(s, "vga_hps_write_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = hpf::check_write(s->L, d_adpcm, d_coefs, d_pcm, d_images)) return rc;
    return hpf::launch_write_images(s->tables, d_adpcm, d_coefs, d_gain, d_start_context, d_pcm, d_images, (hipStream_t)stream,
                                    &t_last_launches);
}

int vga_hps_read_device_v(const vga_hps_files *s, const uint8_t *d_images, uint8_t *d_adpcm, int16_t *d_coefs, int16_t *d_gain,
                          int16_t *d_start_context, int16_t *d_loop_context, void *stream)
{
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
    out[2] = (int64_t)s->table_bytes;
    out[3] = t_last_launches;
    return VGA_OK;
}

}  // extern "C"
