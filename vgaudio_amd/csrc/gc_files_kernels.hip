// gc_files_kernels.hip -- the kernels of include/vgaudio_hip/gc_files.h: GC-ADPCM channel metadata and DSP images for a SET
// of files of different shapes, every kernel one launch over tables the set's object holds (gc_files_host.hpp).
//
//   gc_files_meta_kernel        GcAdpcmSeekTable.CreateSeekTable (GcAdpcmSeekTable.cs:25-38) and GcAdpcmLoopContext
//                               (GcAdpcmLoopContext.cs:17-26) of every channel: gc_channel_meta_kernel with per-channel
//                               row offsets, loop start, spacing and entry count
//   gc_files_header_kernel      DspWriter.WriteHeader (DspWriter.cs:52-80): one thread per channel over a channel -> file table
//   gc_files_interleave_kernel  DspWriter.WriteData (:82-94) of every file: interleave_files_kernel (container_kernels.hpp) over
//                               (file, chunk) work items, so that no wave lies wholly behind its file's image
//   gc_files_read_header_kernel, gc_files_deinterleave_kernel   DspReader.ReadHeader's per-channel fields (DspReader.cs:73-85)
//                               and ReadData (:103-115): deinterleave_kernel over (channel, chunk) work items
// The audio kernels are copies: one thread per granule of the OUTPUT (coalesced stores), loads are contiguous runs of one
// channel, no LDS.  The granule (16 or 8 bytes) is uniform per work item.  The copies of one work item are device functions
// in gc_files_chunks.hpp, which nw_files_kernels.hip instantiates as well.
#include "common.hpp"
#include "gc_files_host.hpp"
#include "gc_files_kernels.hpp"
#include "gc_files_chunks.hpp"

namespace vga {
namespace gcf {

__global__ __launch_bounds__(256) void gc_files_meta_kernel(const ChannelRow *__restrict__ rows, const MetaItem *__restrict__ items,
                                                            const uint8_t *__restrict__ adpcm, const int16_t *__restrict__ pcm,
                                                            int16_t *__restrict__ seek, int16_t *__restrict__ loop_context)
{
    const MetaItem it = items[blockIdx.x];
    const ChannelRow r = rows[it.x];
    const int16_t *p = pcm + r.pcm_off;
    if (seek) {
        int16_t *t = seek + r.seek_off;
#pragma unroll
        for (int k = 0; k < CHUNK_ENTRIES / 256; k++) {
            const int i = it.y + k * 256 + (int)threadIdx.x;
            if (i >= r.entries) break;
            const int64_t at = (int64_t)i * r.spacing;                 // the first entry is always 0
            const int16_t h1 = i == 0 ? (int16_t)0 : p[at - 1], h2 = (i == 0 || at < 2) ? (int16_t)0 : p[at - 2];
            *reinterpret_cast<int *>(t + 2 * i) = (int)(uint16_t)h1 | ((int)(uint16_t)h2 << 16);
        }
    }
    if (loop_context && it.y == 0 && threadIdx.x == 0) {
        int16_t *c = loop_context + (int64_t)it.x * 3;
        const int ls = r.loop_start;
        if (ls == 0) {                                                 // "current loop context is valid": the default context
            c[0] = c[1] = c[2] = 0;
        } else {                                                       // the ORIGINAL stream (GcAdpcmChannelBuilder.cs:179)
            c[0] = (int16_t)adpcm[r.adpcm_off + ls / 14 * 8];
            c[1] = ls < 1 ? (int16_t)0 : p[ls - 1];
            c[2] = ls < 2 ? (int16_t)0 : p[ls - 2];
        }
    }
}

// 96 header bytes as 24 big-endian-filled words, stored as six 16-byte granules (images start on 16-byte boundaries)
struct HeaderWords {
    uint32_t w[24];
    __device__ __forceinline__ void be16(int at, int v)                // at: even byte offset
    {
        const uint32_t b = ((uint32_t)(v >> 8) & 0xFF) | (((uint32_t)v & 0xFF) << 8);
        w[at >> 2] |= b << ((at & 2) * 8);
    }
    __device__ __forceinline__ void be32(int at, int v) { be16(at, v >> 16); be16(at + 2, v); }
};

__global__ __launch_bounds__(64) void gc_files_header_kernel(const FileGeom *__restrict__ geom, const ChannelRow *__restrict__ rows, int nch,
                                                             const uint8_t *__restrict__ adpcm, const int16_t *__restrict__ coefs,
                                                             const int16_t *__restrict__ gain, const int16_t *__restrict__ start_context,
                                                             const int16_t *__restrict__ loop_context, uint8_t *__restrict__ images)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= nch) return;
    const ChannelRow r = rows[c];
    const FileGeom g = geom[r.file];
    HeaderWords h;
#pragma unroll
    for (int k = 0; k < 24; k++) h.w[k] = 0;
    h.be32(0x00, g.sample_count);
    h.be32(0x04, g.nibble_count);
    h.be32(0x08, g.sample_rate);
    h.be16(0x0c, g.looping ? 1 : 0);                                   // (0x0e: Format, 0 for ADPCM)
    h.be32(0x10, g.start_addr);
    h.be32(0x14, g.end_addr);
    h.be32(0x18, g.cur_addr);
#pragma unroll
    for (int k = 0; k < 16; k++) h.be16(0x1c + 2 * k, coefs[(int64_t)c * 16 + k]);
    h.be16(0x3c, gain ? gain[c] : 0);
    if (start_context) {
#pragma unroll
        for (int k = 0; k < 3; k++) h.be16(0x3e + 2 * k, start_context[(int64_t)c * 3 + k]);
    } else {                                                           // GcAdpcmChannel.cs:45: (Adpcm[0], 0, 0) for a fresh channel
        h.be16(0x3e, g.input_size > 0 ? (int)adpcm[r.adpcm_off] : 0);
    }
    if (g.looping && loop_context) {
#pragma unroll
        for (int k = 0; k < 3; k++) h.be16(0x44 + 2 * k, loop_context[(int64_t)c * 3 + k]);
    }
    h.be16(0x4a, g.channels == 1 ? 0 : g.channels);
    h.be16(0x4c, g.channels == 1 ? 0 : g.frames_per_interleave);
    uint4 *dst = reinterpret_cast<uint4 *>(images + g.image_off + (int64_t)DSP_HEADER * (c - g.first_channel));
#pragma unroll
    for (int k = 0; k < 6; k++) dst[k] = make_uint4(h.w[4 * k], h.w[4 * k + 1], h.w[4 * k + 2], h.w[4 * k + 3]);
}

__global__ __launch_bounds__(256) void gc_files_interleave_kernel(const FileGeom *__restrict__ geom, const ChannelRow *__restrict__ rows,
                                                                  const Item *__restrict__ items, const uint8_t *__restrict__ adpcm,
                                                                  uint8_t *__restrict__ images)
{
    const Item it = items[blockIdx.x];
    const FileGeom g = geom[it.x];
    const bool g16 = (it.y >> 31) != 0;
    const uint32_t start = (it.y & 0x7FFFFFFFu) << 3;      // images are < 2 GiB (FileSize is an int)
    const uint32_t total = g.output_size * (uint32_t)g.channels;
    const uint32_t out_blocks = (g.output_size + g.interleave - 1) / g.interleave;
    const uint32_t boundary = (out_blocks - 1) * g.interleave * (uint32_t)g.channels;
    const uint32_t part_end = start < boundary ? boundary : total;
    const uint32_t chunk = (uint32_t)CHUNK_GRANULES * (g16 ? 16u : 8u);
    const uint32_t end = part_end - start < chunk ? part_end : start + chunk;
    uint8_t *audio = images + g.image_off + (int64_t)DSP_HEADER * g.channels;
    if (g16) interleave_chunk<16>(g, rows, adpcm, audio, start, end, total);
    else interleave_chunk<8>(g, rows, adpcm, audio, start, end, total);
}

__device__ __forceinline__ int16_t get_be16(const uint8_t *p) { return (int16_t)(((unsigned)p[0] << 8) | p[1]); }

__global__ __launch_bounds__(64) void gc_files_read_header_kernel(const FileGeom *__restrict__ geom, const ChannelRow *__restrict__ rows, int nch,
                                                                  const uint8_t *__restrict__ images, int16_t *__restrict__ coefs,
                                                                  int16_t *__restrict__ gain, int16_t *__restrict__ start_context,
                                                                  int16_t *__restrict__ loop_context)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= nch) return;
    const FileGeom g = geom[rows[c].file];
    const uint8_t *h = images + g.image_off + (int64_t)DSP_HEADER * (c - g.first_channel);
    if (coefs)
        for (int k = 0; k < 16; k++) coefs[(int64_t)c * 16 + k] = get_be16(h + 0x1c + 2 * k);
    if (gain) gain[c] = get_be16(h + 0x3c);
    if (start_context)
        for (int k = 0; k < 3; k++) start_context[(int64_t)c * 3 + k] = get_be16(h + 0x3e + 2 * k);
    if (loop_context)
        for (int k = 0; k < 3; k++) loop_context[(int64_t)c * 3 + k] = get_be16(h + 0x44 + 2 * k);
}

__global__ __launch_bounds__(256) void gc_files_deinterleave_kernel(const FileGeom *__restrict__ geom, const ChannelRow *__restrict__ rows,
                                                                    const Item *__restrict__ items, const uint8_t *__restrict__ images,
                                                                    uint8_t *__restrict__ adpcm)
{
    const Item it = items[blockIdx.x];
    const ChannelRow r = rows[it.x];
    const FileGeom g = geom[r.file];
    const bool g16 = (it.y >> 31) != 0;
    const uint32_t start = (it.y & 0x7FFFFFFFu) << 3;
    const uint32_t chunk = (uint32_t)CHUNK_GRANULES * (g16 ? 16u : 8u);
    const uint32_t end = g.output_size - start < chunk ? g.output_size : start + chunk;
    const uint8_t *audio = images + g.image_off + (int64_t)DSP_HEADER * g.channels;
    if (g16) deinterleave_chunk<16>(g, it.x - g.first_channel, audio, adpcm + r.adpcm_off, start, end);
    else deinterleave_chunk<8>(g, it.x - g.first_channel, audio, adpcm + r.adpcm_off, start, end);
}

// ---------------------------------------------------------------- launchers
int launch_meta(const DeviceTables &t, bool all_chunks, const uint8_t *d_adpcm, const int16_t *d_pcm, int16_t *d_seek, int16_t *d_loop_context,
                hipStream_t stream)
{
    const int blocks = all_chunks ? t.meta_items : t.channels;         // chunk 0 of every channel comes first
    if (blocks <= 0 || (!d_seek && !d_loop_context)) return VGA_OK;
    hipLaunchKernelGGL(gc_files_meta_kernel, dim3(blocks), dim3(256), 0, stream, t.rows, t.meta, d_adpcm, d_pcm, d_seek, d_loop_context);
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

int launch_write_images(const DeviceTables &t, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *d_gain,
                        const int16_t *d_start_context, const int16_t *d_loop_context, uint8_t *d_images, hipStream_t stream)
{
    if (t.channels <= 0) return VGA_OK;
    hipLaunchKernelGGL(gc_files_header_kernel, dim3((t.channels + 63) / 64), dim3(64), 0, stream, t.geom, t.rows, t.channels, d_adpcm, d_coefs,
                       d_gain, d_start_context, d_loop_context, d_images);
    VGA_HIP_TRY(hipGetLastError());
    if (t.audio_items > 0) {
        hipLaunchKernelGGL(gc_files_interleave_kernel, dim3(t.audio_items), dim3(256), 0, stream, t.geom, t.rows, t.audio, d_adpcm, d_images);
        VGA_HIP_TRY(hipGetLastError());
    }
    return VGA_OK;
}

int launch_read_images(const DeviceTables &t, const uint8_t *d_images, uint8_t *d_adpcm, int16_t *d_coefs, int16_t *d_gain,
                       int16_t *d_start_context, int16_t *d_loop_context, hipStream_t stream)
{
    if (t.channels <= 0) return VGA_OK;
    if (d_coefs || d_gain || d_start_context || d_loop_context) {
        hipLaunchKernelGGL(gc_files_read_header_kernel, dim3((t.channels + 63) / 64), dim3(64), 0, stream, t.geom, t.rows, t.channels, d_images,
                           d_coefs, d_gain, d_start_context, d_loop_context);
        VGA_HIP_TRY(hipGetLastError());
    }
    if (t.audio_items > 0) {
        hipLaunchKernelGGL(gc_files_deinterleave_kernel, dim3(t.audio_items), dim3(256), 0, stream, t.geom, t.rows, t.audio, d_images, d_adpcm);
        VGA_HIP_TRY(hipGetLastError());
    }
    return VGA_OK;
}

}  // namespace gcf
}  // namespace vga
