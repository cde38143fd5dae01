// adx_files_kernels.hpp -- launchers of adx_files_kernels.hip over the device tables of a vga_adx_files object
#pragma once
#include "common.hpp"
#include "adx_files_host.hpp"

namespace vga {
namespace adxf {

// the object's tables in device memory (adx_files_host.hpp has the element types)
struct DeviceTables {
    const FileTab *tab = nullptr;
    const int64_t *row_off = nullptr;
    const int *row_file = nullptr;
    const int16_t *history = nullptr;            // (a set for reading)
    const Item *items[2] = {nullptr, nullptr};   // every file in its own form (span items in front); every file general
    int files = 0, channels = 0;
    int span_items = 0, item_count[2] = {0, 0};
};

// general: the force hook's table
int launch_write_images(const DeviceTables &t, bool general, const uint8_t *d_audio, const int16_t *d_history, uint8_t *d_images,
                        hipStream_t stream);
int launch_read_images(const DeviceTables &t, bool general, const uint8_t *d_images, uint8_t *d_audio, int16_t *d_history_out,
                       hipStream_t stream);

}  // namespace adxf
}  // namespace vga
