// capi_hca_keyed_files.hip -- the key search and the keyed read for sets of HCA files on the device
// (include/vgaudio_hip_files/hca_keyed_files.h).  Host side only: the checks, the workspace's size and the search's work items
// come from hca_keyed_files_host.hpp; the object is capi_hca_files.hip's; a call checks its pointers and launches.
#include "common.hpp"
#include "hca_files_object.hpp"
#include "hca_keyed_files_kernels.hpp"

#include <vector>

using namespace vga;

extern "C" {

size_t vga_hca_find_keys_workspace_bytes(const vga_hca_files *s, int nkeys)
{
    return s ? (size_t)hcak::find_workspace_bytes(s->L, nkeys) : 0;
}

int vga_hca_find_keys_device_v(const vga_hca_files *s, const uint8_t *d_images, const uint8_t *d_tables, int nkeys, int type1_index,
                               int *d_key_index_out, int *d_status, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = hcaf::check_object(s, "vga_hca_find_keys_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = hcak::check_find(s->L, s->find, d_images, d_tables, nkeys, type1_index, d_key_index_out, d_workspace, workspace_bytes)) return rc;
    return hcak::launch_find_keys(s->tables, d_images, d_tables, nkeys, type1_index, d_key_index_out, d_status, d_workspace, (hipStream_t)stream);
}

int vga_hca_read_keyed_device_v(const vga_hca_files *s, const uint8_t *d_images, const uint8_t *d_tables, int ntables,
                                const int *d_key_index, uint8_t *d_frames, int *d_bad_crc, int *d_status, void *stream)
{
    if (int rc = hcaf::check_object(s, "vga_hca_read_keyed_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = hcak::check_keyed_read(s->L, d_images, d_tables, ntables, d_frames)) return rc;
    return hcak::launch_read_keyed(s->tables, hcaf::g_force_general != 0, d_images, d_tables, ntables, d_key_index, d_frames, d_bad_crc, d_status,
                                   (hipStream_t)stream);
}

int vga_hca_find_keys_items_for(const vga_hca_file_info *const *infos, int nfiles, int nkeys, vga_hca_find_keys_item *items_out,
                                int64_t capacity, int64_t *count_out)
{
    if (nkeys < 0) { set_error("vga_hca_find_keys_items_for: negative candidate count %d", nkeys); return VGA_ERR_ARGUMENT; }
    hcaf::FilesLayout L;
    if (int rc = hcaf::make_layout_from_infos(infos, nfiles, nullptr, nullptr, nullptr, 0, false, nullptr, L)) return rc;
    std::vector<vga_hca_find_keys_item> v;
    hcak::describe_find_items(L.encryption_type, nkeys, v);
    return fileset::copy_capped(v, items_out, capacity, count_out);
}

}  // extern "C"
