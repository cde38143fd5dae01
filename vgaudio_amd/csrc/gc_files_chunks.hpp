// gc_files_chunks.hpp -- the two copies every set of container files is made of, as device functions over one work item:
// Interleave (Utilities/Interleave.cs:43-78) of the packed rows of one file into the audio region of its image, and
// DeInterleave (:118-167) of that region back into one row.  gc_files_kernels.hip (DSP images) and nw_files_kernels.hip
// (BRSTM / BCSTM / BFSTM images) instantiate them; what differs between the containers is where the region starts and
// the granule rule, both the caller's.
#pragma once
#include "common.hpp"
#include "gc_files_host.hpp"

namespace vga {
namespace gcf {

template <int G> struct Granule;                  // (container_kernels.hpp's; that header's launchers would instantiate their kernels in the includer)
template <> struct Granule<1> { using type = uint8_t; };   // the general form of a read (idsp_files_kernels.hip)
template <> struct Granule<8> { using type = uint2; };
template <> struct Granule<16> { using type = uint4; };

// bytes [start, end) of the audio region of one image, G-byte granules (interleave_files_kernel's arithmetic; `total` is the
// region's size, which one channel's need not be a multiple of G)
template <int G>
__device__ __forceinline__ void interleave_chunk(const FileGeom &g, const ChannelRow *__restrict__ rows, const uint8_t *__restrict__ adpcm,
                                                 uint8_t *__restrict__ audio, uint32_t start, uint32_t end, uint32_t total)
{
    using T = typename Granule<G>::type;
    const uint32_t interleave = g.interleave, input_size = g.input_size, output_size = g.output_size;
    const uint32_t in_blocks = (input_size + interleave - 1) / interleave, out_blocks = (output_size + interleave - 1) / interleave;
    const uint32_t stride = interleave * (uint32_t)g.channels;
    const uint32_t last_out = output_size - (out_blocks - 1) * interleave;
#pragma unroll
    for (int k = 0; k < CHUNK_GRANULES / 256; k++) {
        const uint32_t o = start + (uint32_t)(k * 256 + (int)threadIdx.x) * G;
        if (o >= end) return;
        uint32_t b = o / stride;
        if (b > out_blocks - 1) b = out_blocks - 1;        // the (short) last block's rows are packed more tightly
        const uint32_t r = o - b * stride;
        const uint32_t cur_out = b == out_blocks - 1 ? last_out : interleave;
        const uint32_t i = r / cur_out, within = r - i * cur_out;
        uint32_t n = 0;                                    // bytes of this row segment that come from the channel
        if (b < in_blocks) {                               // blocksToCopy = min(inBlockCount, outBlockCount)
            const uint32_t cur_in = b == in_blocks - 1 ? input_size - (in_blocks - 1) * interleave : interleave;
            n = cur_in < cur_out ? cur_in : cur_out;
        }
        const uint8_t *s = adpcm + rows[g.first_channel + (int)i].adpcm_off + (uint64_t)interleave * b + within;
        uint8_t *d = audio + o;
        if (within + G <= n) {
            *reinterpret_cast<T *>(d) = *reinterpret_cast<const T *>(s);
        } else if (o + G <= total) {
            uint8_t tmp[G];
#pragma unroll
            for (int q = 0; q < G; q++) tmp[q] = within + q < n ? s[q] : 0;
            T v;
            memcpy(&v, tmp, G);
            *reinterpret_cast<T *>(d) = v;
        } else {                                           // the end of a single channel's bytes
            for (uint32_t q = 0; o + q < total; q++) d[q] = within + q < n ? s[q] : 0;
        }
    }
}

// bytes [start, end) of one channel's row (deinterleave_kernel's arithmetic)
template <int G>
__device__ __forceinline__ void deinterleave_chunk(const FileGeom &g, int o_ch, const uint8_t *__restrict__ audio, uint8_t *__restrict__ row,
                                                   uint32_t start, uint32_t end)
{
    using T = typename Granule<G>::type;
    const uint32_t interleave = g.interleave, input_size = g.input_size, output_size = g.output_size;
    const uint32_t in_blocks = (input_size + interleave - 1) / interleave, out_blocks = (output_size + interleave - 1) / interleave;
    const uint32_t to_copy = in_blocks < out_blocks ? in_blocks : out_blocks;
#pragma unroll
    for (int k = 0; k < CHUNK_GRANULES / 256; k++) {
        const uint32_t off = start + (uint32_t)(k * 256 + (int)threadIdx.x) * G;
        if (off >= end) return;
        const uint32_t b = off / interleave, within = off - b * interleave;
        uint32_t n = 0, cur_in = interleave;
        if (b < to_copy) {
            cur_in = b == in_blocks - 1 ? input_size - (in_blocks - 1) * interleave : interleave;
            const uint32_t cur_out = b == out_blocks - 1 ? output_size - (out_blocks - 1) * interleave : interleave;
            n = cur_in < cur_out ? cur_in : cur_out;
        }
        const uint8_t *s = audio + (uint64_t)interleave * b * (uint32_t)g.channels + (uint64_t)cur_in * (uint32_t)o_ch + within;
        uint8_t *d = row + off;
        if (within + G <= n && off + G <= output_size) {
            *reinterpret_cast<T *>(d) = *reinterpret_cast<const T *>(s);
        } else {
            for (int q = 0; q < G && off + q < output_size; q++) d[q] = within + q < n ? s[q] : 0;
        }
    }
}

}  // namespace gcf
}  // namespace vga
