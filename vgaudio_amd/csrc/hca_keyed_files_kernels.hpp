// hca_keyed_files_kernels.hpp -- launchers of hca_keyed_files_kernels.hip over the device tables of a vga_hca_files object
#pragma once
#include "common.hpp"
#include "hca_files_kernels.hpp"
#include "hca_keyed_files_host.hpp"

namespace vga {
namespace hcak {

// the search: four launches (first tested frame, first frame under every candidate, later frames under the survivors,
// resolve); d_workspace as find_workspace_bytes lays it out
int launch_find_keys(const hcaf::DeviceTables &t, const uint8_t *d_images, const uint8_t *d_tables, int nkeys, int type1_index,
                     int *d_key_index_out, int *d_status, void *d_workspace, hipStream_t stream);
// the read kernels of hca_files_kernels.hip with the caller's tables and per-file indices; one more launch for d_status
int launch_read_keyed(const hcaf::DeviceTables &t, bool general, const uint8_t *d_images, const uint8_t *d_tables, int ntables,
                      const int *d_key_index, uint8_t *d_frames, int *d_bad_crc, int *d_status, hipStream_t stream);

}  // namespace hcak
}  // namespace vga
