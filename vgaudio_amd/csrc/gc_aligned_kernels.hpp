// gc_aligned_kernels.hpp -- launchers of gc_aligned_kernels.hip over the device tables of a vga_gc_aligned object
#pragma once
#include "common.hpp"
#include "gc_aligned_host.hpp"

namespace vga {
namespace gca {

// the object's tables in device memory (gc_aligned_host.hpp has the element types)
struct DeviceTables {
    const AlignRow *rows = nullptr;
    const Item *gather = nullptr, *adpcm = nullptr, *pcm = nullptr;
    const MetaItem *meta = nullptr;
    int channels = 0, gather_items = 0, adpcm_items = 0, pcm_items = 0, meta_items = 0;
};

// newPcm of GcAdpcmAlignment.cs:44-51 for every aligned channel into the tail batch's PCM rows, its re-encode history
// (:54-55) and its coefficients, the last two indexed by tail row
int launch_gather(const DeviceTables &t, const int16_t *d_in_pcm, const int16_t *d_coefs, int16_t *d_tail_pcm, int16_t *d_tail_coefs,
                  int16_t *d_hist1, int16_t *d_hist2, hipStream_t stream);
// every output row: its kept bytes from the input row, the rest from the tail batch's row
int launch_assemble_adpcm(const DeviceTables &t, const uint8_t *d_adpcm, const uint8_t *d_tail_adpcm, uint8_t *d_adpcm_out, hipStream_t stream);
int launch_assemble_pcm(const DeviceTables &t, const int16_t *d_in_pcm, const int16_t *d_tail_pcm, int16_t *d_pcm_out, hipStream_t stream);
// seek tables and loop contexts from the aligned PCM (its kept samples in d_in_pcm, the rest in d_tail_pcm) and the original
// ADPCM; all_chunks false: only the first chunk of every channel (loop contexts alone)
int launch_meta(const DeviceTables &t, bool all_chunks, const uint8_t *d_adpcm, const int16_t *d_in_pcm, const int16_t *d_tail_pcm,
                int16_t *d_seek, int16_t *d_loop_context, hipStream_t stream);

}  // namespace gca
}  // namespace vga
