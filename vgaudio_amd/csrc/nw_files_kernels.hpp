// nw_files_kernels.hpp -- launchers of nw_files_kernels.hip over the device tables of a vga_nw_files object
#pragma once
#include "common.hpp"
#include "nw_files_host.hpp"

namespace vga {
namespace nwf {

// the object's tables in device memory (nw_files_host.hpp has the element types)
struct DeviceTables {
    const FileTab *tab = nullptr;
    const ChannelRow *rows = nullptr;
    const ChannelMeta *meta = nullptr;           // (a set for reading)
    const Item *audio = nullptr, *seek = nullptr;
    int files = 0, channels = 0, audio_items = 0, seek_items = 0;
};

int launch_write_images(const DeviceTables &t, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *d_gain,
                        const int16_t *d_start_context, const int16_t *d_loop_context, const int16_t *d_seek, uint8_t *d_images,
                        hipStream_t stream);
int launch_read_images(const DeviceTables &t, const uint8_t *d_images, uint8_t *d_adpcm, int16_t *d_coefs, int16_t *d_gain,
                       int16_t *d_start_context, int16_t *d_loop_context, hipStream_t stream);

}  // namespace nwf
}  // namespace vga
