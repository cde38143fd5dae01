// adx_keyed_files_kernels.hpp -- launchers of adx_keyed_files_kernels.hip over the device tables of a vga_adx_files object
#pragma once
#include "common.hpp"
#include "adx_files_kernels.hpp"
#include "adx_keyed_files_host.hpp"

namespace vga {
namespace adxk {

// the caller's keys as they lie in device memory
struct Keys {
    const vga_adx_key *keys;
    int nkeys;
    const int *index;                            // per file, or null: key 0
};

int launch_write_keyed(const adxf::DeviceTables &t, bool general, const uint8_t *d_audio, const int16_t *d_history, Keys keys,
                       uint8_t *d_images, int *d_status, hipStream_t stream);
int launch_read_keyed(const adxf::DeviceTables &t, bool general, const uint8_t *d_images, Keys keys, uint8_t *d_audio,
                      int16_t *d_history_out, int *d_status, hipStream_t stream);
int launch_find_keys(const adxf::DeviceTables &t, const uint8_t *d_images, const vga_adx_key *d_keys, int nkeys8, int nkeys9,
                     int *d_key_index_out, uint32_t *d_bits, hipStream_t stream);

}  // namespace adxk
}  // namespace vga
