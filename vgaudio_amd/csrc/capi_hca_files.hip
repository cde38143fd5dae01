// capi_hca_files.hip -- sets of HCA files on the device: the images of every file written and read in one set of launches,
// keys and frame CRCs on the way (include/vgaudio_hip/hca_files.h).  Host side only: checks, layout, headers and work items
// come from hca_files_host.hpp; create uploads the tables the kernels read (hca_files_kernels.hpp), a call checks its
// pointers and launches.
#include "common.hpp"
#include "hca_capi.hpp"
#include "hca_files_object.hpp"

#include <cstring>
#include <vector>

using namespace vga;

thread_local int vga::hcaf::g_force_general = 0; // vga_hca_files_force_general_this_thread

int vga::hcaf::check_object(const vga_hca_files *s, const char *what)
{
    if (!s) { set_error("%s: null vga_hca_files", what); return VGA_ERR_ARGUMENT; }
    int device = -1;
    if (s->L.totals.files > 0) (void)hipGetDevice(&device);
    if (s->L.totals.files > 0 && device != s->device) {
        set_error("%s: the set was created on device %d, the current one is %d", what, s->device, device);
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}

namespace {

using hcaf::check_object;
using hcaf::g_force_general;

template <class T> size_t place(size_t &at, const std::vector<T> &v)
{
    const size_t here = at;
    at += (size_t)hcaf::pad_to((int64_t)(v.size() * sizeof(T)), 16);
    return here;
}
template <class T> void fill(std::vector<unsigned char> &host, size_t at, const std::vector<T> &v)
{
    if (!v.empty()) memcpy(host.data() + at, v.data(), v.size() * sizeof(T));
}

// the tables in the current device's memory
int finish_create(vga_hca_files *s)
{
    hcaf::FilesLayout &L = s->L;
    hcak::make_find_tables(L, s->find);
    if (L.totals.files == 0) return VGA_OK;                   // an empty set needs no device
    if (int rc = require_device()) return rc;
    (void)hipGetDevice(&s->device);
    size_t bytes = 0;
    const size_t headers_at = place(bytes, L.headers), tab_at = place(bytes, L.tab), keys_at = place(bytes, L.tables);
    const size_t own_at = place(bytes, L.items[0]), general_at = place(bytes, L.items[1]);
    const size_t walk_at = place(bytes, s->find.walk), find_at = place(bytes, s->find.find_files);
    std::vector<unsigned char> host(bytes + 16, 0);
    fill(host, headers_at, L.headers);
    fill(host, tab_at, L.tab);
    fill(host, keys_at, L.tables);
    fill(host, own_at, L.items[0]);
    fill(host, general_at, L.items[1]);
    fill(host, walk_at, s->find.walk);
    fill(host, find_at, s->find.find_files);
    hcaf::DeviceTables &t = s->tables;
    if (int rc = hca::crc_pow_table(&t.crc_pow)) return rc;
    VGA_HIP_TRY(device_malloc(&s->d_tables, host.size()));
    VGA_HIP_TRY(hipMemcpy(s->d_tables, host.data(), host.size(), hipMemcpyHostToDevice));
    const unsigned char *d = static_cast<const unsigned char *>(s->d_tables);
    t.headers = d + headers_at;
    t.tab = reinterpret_cast<const hcaf::FileTab *>(d + tab_at);
    t.tables = d + keys_at;
    t.items[0] = reinterpret_cast<const hcaf::Item *>(d + own_at);
    t.items[1] = reinterpret_cast<const hcaf::Item *>(d + general_at);
    t.files = L.totals.files;
    t.span_items = L.span_items;
    t.item_count[0] = (int)L.items[0].size();
    t.item_count[1] = (int)L.items[1].size();
    t.walk = reinterpret_cast<const hcak::WalkFile *>(d + walk_at);
    t.find_files = reinterpret_cast<const int *>(d + find_at);
    t.find_file_count = (int)s->find.find_files.size();
    t.find_max_channels = s->find.max_channels;
    return VGA_OK;
}

void copy_offsets(const hcaf::FilesLayout &L, int64_t *frame_offsets_out, int64_t *image_offsets_out)
{
    if (frame_offsets_out) std::copy(L.frame_off.begin(), L.frame_off.end(), frame_offsets_out);
    if (image_offsets_out) std::copy(L.image_off.begin(), L.image_off.end(), image_offsets_out);
}

template <class Make> int create_with(vga_hca_files **out, Make &&make)
{
    if (!out) { set_error("null output"); return VGA_ERR_ARGUMENT; }
    *out = nullptr;
    vga_hca_files *s = new vga_hca_files;
    int rc = make(s->L);
    if (!rc) rc = finish_create(s);
    if (rc) {
        delete s;
        return rc;
    }
    *out = s;
    return VGA_OK;
}

int items_out(const hcaf::FilesLayout &L, int general, vga_hca_files_item *items, int64_t capacity, int64_t *count_out)
{
    std::vector<vga_hca_files_item> v;
    hcaf::describe_items(L, general != 0, v);
    if (count_out) *count_out = (int64_t)v.size();
    if (!items) return VGA_OK;
    if ((int64_t)v.size() > capacity) { set_error("%lld work items, room for %lld", (long long)v.size(), (long long)capacity); return VGA_ERR_ARGUMENT; }
    std::copy(v.begin(), v.end(), items);
    return VGA_OK;
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
    return create_with(out, [&](hcaf::FilesLayout &L) { return hcaf::make_layout(files, nfiles, frame_offsets, tables, ntables, true, L); });
}

int vga_hca_files_create_from_infos(const vga_hca_file_info *const *infos, int nfiles, const int64_t *image_offsets, const int *keys,
                                    const uint8_t *tables, int ntables, const int64_t *frame_offsets, vga_hca_files **out)
{
    return create_with(out, [&](hcaf::FilesLayout &L) {
        return hcaf::make_layout_from_infos(infos, nfiles, image_offsets, keys, tables, ntables, true, frame_offsets, L);
    });
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
