// wave_files_kernels.hpp -- launchers of wave_files_kernels.hip over the device tables of a vga_wave_files object
#pragma once
#include "common.hpp"
#include "wave_files_host.hpp"

namespace vga {
namespace wavf {

// the object's tables in device memory (wave_files_host.hpp has the element types)
struct DeviceTables {
    const FileTab *tab = nullptr;
    const int64_t *row_off = nullptr;
    const int *row_file = nullptr;
    const uint8_t *headers = nullptr;            // (a set for writing)
    const Item *items[2] = {nullptr, nullptr};   // every file in its own form (tile items in front); every file general
    int files = 0, channels = 0;
    int tile_items = 0, item_count[2] = {0, 0};
};

// general: the force hook's table
int launch_write_images(const DeviceTables &t, bool general, const int16_t *d_pcm, uint8_t *d_images, hipStream_t stream);
int launch_read_images(const DeviceTables &t, bool general, const uint8_t *d_images, int16_t *d_pcm, hipStream_t stream);

}  // namespace wavf
}  // namespace vga
