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
    // the keyed calls' own (adx_keyed_files_kernels.hpp)
    const Item *cipher_items[2] = {nullptr, nullptr}, *find_items = nullptr;
    int cipher_count[2] = {0, 0}, find_count = 0;
};

// general: the force hook's table
int launch_write_images(const DeviceTables &t, bool general, const uint8_t *d_audio, const int16_t *d_history, uint8_t *d_images,
                        hipStream_t stream);
int launch_read_images(const DeviceTables &t, bool general, const uint8_t *d_images, uint8_t *d_audio, int16_t *d_history_out,
                       hipStream_t stream);

// the launches of those two calls one by one (the span kernels aside), for the keyed calls
int launch_write_headers(const DeviceTables &t, const int16_t *d_history, uint8_t *d_images, hipStream_t stream);
int launch_write_general(const DeviceTables &t, bool general, const uint8_t *d_audio, uint8_t *d_images, hipStream_t stream);
int launch_write_footers(const DeviceTables &t, uint8_t *d_images, hipStream_t stream);
int launch_read_history(const DeviceTables &t, int16_t *d_history_out, hipStream_t stream);
int launch_read_general(const DeviceTables &t, bool general, const uint8_t *d_images, uint8_t *d_audio, hipStream_t stream);

}  // namespace adxf
}  // namespace vga
