// gc_files_kernels.hpp -- launchers of gc_files_kernels.hip over the device tables of a vga_gc_files object
#pragma once
#include "common.hpp"
#include "gc_files_host.hpp"

namespace vga {
namespace gcf {

// the object's tables in device memory (gc_files_host.hpp has the element types)
struct DeviceTables {
    const FileGeom *geom = nullptr;
    const ChannelRow *rows = nullptr;
    const Item *audio = nullptr;
    const MetaItem *meta = nullptr;
    int channels = 0, audio_items = 0, meta_items = 0;
};

// seek tables and loop contexts; all_chunks false: only the first chunk of every channel (loop contexts alone)
int launch_meta(const DeviceTables &t, bool all_chunks, const uint8_t *d_adpcm, const int16_t *d_pcm, int16_t *d_seek, int16_t *d_loop_context,
                hipStream_t stream);
int launch_write_images(const DeviceTables &t, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *d_gain,
                        const int16_t *d_start_context, const int16_t *d_loop_context, uint8_t *d_images, hipStream_t stream);
int launch_read_images(const DeviceTables &t, const uint8_t *d_images, uint8_t *d_adpcm, int16_t *d_coefs, int16_t *d_gain,
                       int16_t *d_start_context, int16_t *d_loop_context, hipStream_t stream);

}  // namespace gcf
}  // namespace vga
