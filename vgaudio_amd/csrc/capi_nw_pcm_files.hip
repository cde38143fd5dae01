// capi_nw_pcm_files.hip -- sets of PCM16 / PCM8 NintendoWare stream files on the device: the images of every file written from
// planar int16 rows and read into them in one set of launches (include/vgaudio_hip_files/nw_pcm_files.h).  Host side only:
// checks, layout and work items come from nw_pcm_files_host.hpp; create uploads the tables the kernels read
// (nw_pcm_files_kernels.hpp), a call checks its pointers and launches.
#include "common.hpp"
#include "nw_pcm_files_kernels.hpp"

#include <cstring>
#include <vector>

using namespace vga;

struct vga_nw_pcm_files {
    nwpf::FilesLayout L;
    void *d_tables = nullptr;
    nwpf::DeviceTables tables;
    int device = 0;
    ~vga_nw_pcm_files()
    {
        if (d_tables) (void)hipFree(d_tables);
    }
};

namespace {

thread_local int g_force_general = 0;            // vga_nw_pcm_files_force_general_this_thread

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

// the tables in the current device's memory, through the library's allocator
int finish_create(vga_nw_pcm_files *s)
{
    nwpf::FilesLayout &L = s->L;
    if (L.P.totals.files == 0) return VGA_OK;                 // an empty set needs no device
    if (int rc = require_device()) return rc;
    (void)hipGetDevice(&s->device);
    size_t bytes = 0;
    const size_t tab_at = place(bytes, L.tab), rows_at = place(bytes, L.P.row_off), file_at = place(bytes, L.P.row_file);
    const size_t own_at = place(bytes, L.items[0]), general_at = place(bytes, L.items[1]);
    std::vector<unsigned char> host(bytes + 16, 0);
    fill(host, tab_at, L.tab);
    fill(host, rows_at, L.P.row_off);
    fill(host, file_at, L.P.row_file);
    fill(host, own_at, L.items[0]);
    fill(host, general_at, L.items[1]);
    VGA_HIP_TRY(device_malloc(&s->d_tables, host.size()));
    VGA_HIP_TRY(hipMemcpy(s->d_tables, host.data(), host.size(), hipMemcpyHostToDevice));
    const unsigned char *d = static_cast<const unsigned char *>(s->d_tables);
    nwpf::DeviceTables &t = s->tables;
    t.tab = reinterpret_cast<const nwpf::FileTab *>(d + tab_at);
    t.row_off = reinterpret_cast<const int64_t *>(d + rows_at);
    t.row_file = reinterpret_cast<const int *>(d + file_at);
    t.items[0] = reinterpret_cast<const nwpf::Item *>(d + own_at);
    t.items[1] = reinterpret_cast<const nwpf::Item *>(d + general_at);
    t.files = L.P.totals.files;
    t.channels = L.P.totals.channels;
    t.vector_items = L.vector_items;
    t.item_count[0] = (int)L.items[0].size();
    t.item_count[1] = (int)L.items[1].size();
    return VGA_OK;
}

int check_object(const vga_nw_pcm_files *s, const char *what)
{
    if (!s) { set_error("%s: null vga_nw_pcm_files", what); return VGA_ERR_ARGUMENT; }
    int device = -1;
    if (s->L.P.totals.files > 0) (void)hipGetDevice(&device);
    if (s->L.P.totals.files > 0 && device != s->device) {
        set_error("%s: the set was created on device %d, the current one is %d", what, s->device, device);
        return VGA_ERR_ARGUMENT;
    }
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

template <class Make> int create_with(vga_nw_pcm_files **out, Make &&make)
{
    if (!out) { set_error("null output"); return VGA_ERR_ARGUMENT; }
    *out = nullptr;
    vga_nw_pcm_files *s = new vga_nw_pcm_files;
    int rc = make(s->L);
    if (!rc) rc = finish_create(s);
    if (rc) {
        delete s;
        return rc;
    }
    *out = s;
    return VGA_OK;
}

int items_out(const nwpf::FilesLayout &L, int general, vga_nw_pcm_files_item *items, int64_t capacity, int64_t *count_out)
{
    std::vector<vga_nw_pcm_files_item> v;
    nwpf::describe_items(L, general != 0, v);
    if (count_out) *count_out = (int64_t)v.size();
    if (!items) return VGA_OK;
    if ((int64_t)v.size() > capacity) { set_error("%lld work items, room for %lld", (long long)v.size(), (long long)capacity); return VGA_ERR_ARGUMENT; }
    std::copy(v.begin(), v.end(), items);
    return VGA_OK;
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
    return create_with(out, [&](nwpf::FilesLayout &L) { return nwpf::make_layout(files, nfiles, config, codec, pcm_offsets, image_offsets, L); });
}

int vga_nw_pcm_files_create_from_infos(const vga_nwstm_info *const *infos, int nfiles, const int64_t *pcm_offsets, const int64_t *image_offsets,
                                       vga_nw_pcm_files **out)
{
    return create_with(out, [&](nwpf::FilesLayout &L) { return nwpf::make_layout_from_infos(infos, nfiles, pcm_offsets, image_offsets, L); });
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
