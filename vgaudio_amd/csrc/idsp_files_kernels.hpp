// idsp_files_kernels.hpp -- launchers of idsp_files_kernels.hip over the device tables of a vga_idsp_files object
#pragma once
#include "common.hpp"
#include "idsp_files_host.hpp"

namespace vga {
namespace idf {

// the object's tables in device memory (idsp_files_host.hpp has the element types)
struct DeviceTables {
    const FileTab *tab = nullptr;
    const ChannelRow *rows = nullptr;
    const ChannelMeta *meta = nullptr;           // (a set for reading)
    const Item *audio = nullptr;
    int files = 0, channels = 0, audio_items = 0;
};

// *launches: the kernels launched
int launch_write_images(const DeviceTables &t, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *d_gain,
                        const int16_t *d_start_context, const int16_t *d_loop_context, uint8_t *d_images, hipStream_t stream,
                        int *launches);
int launch_read_images(const DeviceTables &t, const uint8_t *d_images, uint8_t *d_adpcm, int16_t *d_coefs, int16_t *d_gain,
                       int16_t *d_start_context, int16_t *d_loop_context, hipStream_t stream, int *launches);

}  // namespace idf
}  // namespace vga
