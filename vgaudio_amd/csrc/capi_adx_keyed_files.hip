// capi_adx_keyed_files.hip -- keyed encryption for sets of ADX files on the device
// (include/vgaudio_hip_files/adx_keyed_files.h).  Host side only: the checks, the workspace's size and the search's work items
// come from adx_keyed_files_host.hpp; the object is capi_adx_files.hip's; a call checks its pointers and launches.
#include "common.hpp"
#include "adx_files_object.hpp"
#include "adx_keyed_files_kernels.hpp"

#include <vector>

using namespace vga;

extern "C" {

int vga_adx_write_keyed_device_v(const vga_adx_files *s, const uint8_t *d_audio, const int16_t *d_history, const vga_adx_key *d_keys,
                                 int nkeys, const int *d_key_index, uint8_t *d_images, int *d_status, void *stream)
{
    if (int rc = adxf::check_object(s, "vga_adx_write_keyed_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = adxk::check_keyed_write(s->L, d_audio, d_history, d_keys, nkeys, d_images)) return rc;
    return adxk::launch_write_keyed(s->tables, adxf::g_force_general != 0, d_audio, d_history, adxk::Keys{d_keys, nkeys, d_key_index}, d_images,
                                    d_status, (hipStream_t)stream);
}

int vga_adx_read_keyed_device_v(const vga_adx_files *s, const uint8_t *d_images, const vga_adx_key *d_keys, int nkeys,
                                const int *d_key_index, uint8_t *d_audio, int16_t *d_history_out, int *d_status, void *stream)
{
    if (int rc = adxf::check_object(s, "vga_adx_read_keyed_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = adxk::check_keyed_read(s->L, d_images, d_keys, nkeys, d_audio)) return rc;
    return adxk::launch_read_keyed(s->tables, adxf::g_force_general != 0, d_images, adxk::Keys{d_keys, nkeys, d_key_index}, d_audio,
                                   d_history_out, d_status, (hipStream_t)stream);
}

size_t vga_adx_find_keys_workspace_bytes(const vga_adx_files *s, int nkeys8, int nkeys9)
{
    return s ? (size_t)adxk::find_workspace_bytes(s->L, nkeys8, nkeys9) : 0;
}

int vga_adx_find_keys_device_v(const vga_adx_files *s, const uint8_t *d_images, const vga_adx_key *d_keys, int nkeys8, int nkeys9,
                               int *d_key_index_out, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = adxf::check_object(s, "vga_adx_find_keys_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = adxk::check_find(s->L, d_images, d_keys, nkeys8, nkeys9, d_key_index_out, d_workspace, workspace_bytes)) return rc;
    return adxk::launch_find_keys(s->tables, d_images, d_keys, nkeys8, nkeys9, d_key_index_out, static_cast<uint32_t *>(d_workspace),
                                  (hipStream_t)stream);
}

int vga_adx_find_keys_items_for(const vga_adx_file_info *const *infos, int nfiles, const int64_t *image_offsets,
                                vga_adx_find_keys_item *items_out, int64_t capacity, int64_t *count_out)
{
    adxf::FilesLayout L;
    if (int rc = adxf::make_layout_from_infos(infos, nfiles, image_offsets, L)) return rc;
    std::vector<vga_adx_find_keys_item> v;
    adxk::describe_find_items(L, v);
    return fileset::copy_capped(v, items_out, capacity, count_out);
}

}  // extern "C"
