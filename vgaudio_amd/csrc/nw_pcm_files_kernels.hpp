// nw_pcm_files_kernels.hpp -- launchers of nw_pcm_files_kernels.hip over the device tables of a vga_nw_pcm_files object
#pragma once
#include "common.hpp"
#include "nw_pcm_files_host.hpp"

namespace vga {
namespace nwpf {

// the object's tables in device memory (nw_pcm_files_host.hpp has the element types)
struct DeviceTables {
    const FileTab *tab = nullptr;
    const int64_t *row_off = nullptr;            // per row, samples
    const int *row_file = nullptr;               // per row
    const Item *items[2] = {nullptr, nullptr};   // [0]: own form, vector items in front; [1]: all general
    int files = 0, channels = 0, vector_items = 0, item_count[2] = {0, 0};
};

int launch_write_images(const DeviceTables &t, bool general, const int16_t *d_pcm, uint8_t *d_images, hipStream_t stream);
int launch_read_images(const DeviceTables &t, bool general, const uint8_t *d_images, int16_t *d_pcm, hipStream_t stream);

}  // namespace nwpf
}  // namespace vga
