// nw_files_kernels.hip -- the kernels of include/vgaudio_hip/nw_files.h: the BRSTM / BCSTM / BFSTM images of a SET of files of
// different shapes, every kernel one launch over tables the set's object holds (nw_files_host.hpp).
//
//   nw_files_header_kernel       the file header, HEAD / INFO and the block headers of every file: nw_header_body.hpp's body, one
//                                workgroup per file, over the file's table entry, the default track list and packed rows
//   nw_files_seek_kernel         GcAdpcmFormat.BuildSeekTable (GcAdpcmFormat.cs:100-113) into the ADPC / SEEK body of every file:
//                                nw_seek_kernel's arithmetic over (file, chunk) work items, the source the packed tables
//   nw_files_interleave_kernel   Interleave(channels, InterleaveSize, AudioDataSize) of every file: gc_files_chunks.hpp's
//                                interleave_chunk over (file, chunk) work items
//   nw_files_meta_kernel, nw_files_deinterleave_kernel   the read side: the parsed per-channel arrays out of the object's table,
//                                and deinterleave_chunk over (channel, chunk) work items
// The audio kernels are copies: one thread per granule of the OUTPUT (coalesced stores), loads are contiguous runs of one
// channel, no LDS.  The granule (16 or 8 bytes) is uniform per work item and chosen on the host.
#include "common.hpp"
#include "gc_files_chunks.hpp"
#include "nw_files_kernels.hpp"
#include "nw_header_body.hpp"

namespace vga {
namespace nwf {

// the rows of one file of a set, the default track list computed in place
struct PackedRows {
    const FileTab &t;
    const ChannelRow *rows;
    const uint8_t *adpcm;
    __device__ int64_t row(int ch) const { return t.audio.first_channel + ch; }
    __device__ int first_byte(int ch) const { return t.audio.input_size > 0 ? adpcm[rows[t.audio.first_channel + ch].adpcm_off] : 0; }
    __device__ nw::TrackK track(int i) const { return nw::default_track(t.h.nch, i); }
};

__global__ __launch_bounds__(64) void nw_files_header_kernel(const FileTab *__restrict__ tab, const ChannelRow *__restrict__ rows,
                                                             const uint8_t *__restrict__ adpcm, const int16_t *__restrict__ coefs,
                                                             const int16_t *__restrict__ gain, const int16_t *__restrict__ start_ctx,
                                                             const int16_t *__restrict__ loop_ctx, uint8_t *__restrict__ images)
{
    const FileTab &t = tab[blockIdx.x];
    const PackedRows p{t, rows, adpcm};
    nw::write_header(t.h, p, coefs, gain, start_ctx, loop_ctx, images + t.audio.image_off);
}

// One thread per short of the block body, four shorts per thread; the block's padding is written as zeros here.  The
// channels' tables are interleaved by 2 shorts and resized to seek_entries (zero fill / truncation); big-endian only in BRSTM.
__global__ __launch_bounds__(256) void nw_files_seek_kernel(const FileTab *__restrict__ tab, const ChannelRow *__restrict__ rows,
                                                            const Item *__restrict__ items, const int16_t *__restrict__ seek,
                                                            uint8_t *__restrict__ images)
{
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[it.x];
    const int nch = t.h.nch, body_shorts = t.seek_body_shorts, entries = t.seek_entries, src_entries = t.seek_src_entries;
    const int big = t.seek_big, first = t.audio.first_channel;
    uint8_t *body = images + t.audio.image_off + t.h.seek_offset + 8;
#pragma unroll
    for (int q = 0; q < CHUNK_SHORTS / 256; q++) {
        const int k = (int)it.y + q * 256 + (int)threadIdx.x;
        if (k >= body_shorts) return;
        int v = 0;
        if (k < entries * nch * 2) {
            const int e = k / (2 * nch), r = k - e * 2 * nch, ch = r >> 1, j = r & 1;
            if (e < src_entries) v = seek[rows[first + ch].seek_off + 2 * e + j];
        }
        uint8_t *d = body + 2 * k;
        d[0] = (uint8_t)(big ? v >> 8 : v);
        d[1] = (uint8_t)(big ? v : v >> 8);
    }
}

__global__ __launch_bounds__(256) void nw_files_interleave_kernel(const FileTab *__restrict__ tab, const ChannelRow *__restrict__ rows,
                                                                  const Item *__restrict__ items, const uint8_t *__restrict__ adpcm,
                                                                  uint8_t *__restrict__ images)
{
    const Item it = items[blockIdx.x];
    const gcf::FileGeom g = tab[it.x].audio;
    const bool g16 = (it.y >> 31) != 0;
    const uint32_t start = (it.y & 0x7FFFFFFFu) << 3;      // images are < 2 GiB (FileSize is an int)
    const uint32_t total = g.output_size * (uint32_t)g.channels;
    const uint32_t out_blocks = (g.output_size + g.interleave - 1) / g.interleave;
    const uint32_t boundary = (out_blocks - 1) * g.interleave * (uint32_t)g.channels;
    const uint32_t part_end = start < boundary ? boundary : total;
    const uint32_t chunk = (uint32_t)gcf::CHUNK_GRANULES * (g16 ? 16u : 8u);
    const uint32_t end = part_end - start < chunk ? part_end : start + chunk;
    uint8_t *audio = images + g.image_off + tab[it.x].audio_offset;
    if (g16) gcf::interleave_chunk<16>(g, rows, adpcm, audio, start, end, total);
    else gcf::interleave_chunk<8>(g, rows, adpcm, audio, start, end, total);
}

// one thread per channel: the parsed coefficients, gain and contexts
__global__ __launch_bounds__(64) void nw_files_meta_kernel(const ChannelMeta *__restrict__ meta, int nch, int16_t *__restrict__ coefs,
                                                           int16_t *__restrict__ gain, int16_t *__restrict__ start_context,
                                                           int16_t *__restrict__ loop_context)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= nch) return;
    const int16_t *m = meta[c].v;
    if (coefs)
        for (int k = 0; k < 16; k++) coefs[(int64_t)c * 16 + k] = m[k];
    if (gain) gain[c] = m[16];
    if (start_context)
        for (int k = 0; k < 3; k++) start_context[(int64_t)c * 3 + k] = m[17 + k];
    if (loop_context)
        for (int k = 0; k < 3; k++) loop_context[(int64_t)c * 3 + k] = m[20 + k];
}

__global__ __launch_bounds__(256) void nw_files_deinterleave_kernel(const FileTab *__restrict__ tab, const ChannelRow *__restrict__ rows,
                                                                    const Item *__restrict__ items, const uint8_t *__restrict__ images,
                                                                    uint8_t *__restrict__ adpcm)
{
    const Item it = items[blockIdx.x];
    const ChannelRow r = rows[it.x];
    const gcf::FileGeom g = tab[r.file].audio;
    const bool g16 = (it.y >> 31) != 0;
    const uint32_t start = (it.y & 0x7FFFFFFFu) << 3;
    const uint32_t chunk = (uint32_t)gcf::CHUNK_GRANULES * (g16 ? 16u : 8u);
    const uint32_t end = g.output_size - start < chunk ? g.output_size : start + chunk;
    const uint8_t *audio = images + g.image_off + tab[r.file].audio_offset;
    if (g16) gcf::deinterleave_chunk<16>(g, it.x - g.first_channel, audio, adpcm + r.adpcm_off, start, end);
    else gcf::deinterleave_chunk<8>(g, it.x - g.first_channel, audio, adpcm + r.adpcm_off, start, end);
}

// ---------------------------------------------------------------- launchers
int launch_write_images(const DeviceTables &t, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *d_gain,
                        const int16_t *d_start_context, const int16_t *d_loop_context, const int16_t *d_seek, uint8_t *d_images,
                        hipStream_t stream)
{
    if (t.files <= 0) return VGA_OK;
    hipLaunchKernelGGL(nw_files_header_kernel, dim3(t.files), dim3(64), 0, stream, t.tab, t.rows, d_adpcm, d_coefs, d_gain, d_start_context,
                       d_loop_context, d_images);
    VGA_HIP_TRY(hipGetLastError());
    if (t.seek_items > 0) {
        hipLaunchKernelGGL(nw_files_seek_kernel, dim3(t.seek_items), dim3(256), 0, stream, t.tab, t.rows, t.seek, d_seek, d_images);
        VGA_HIP_TRY(hipGetLastError());
    }
    if (t.audio_items > 0) {
        hipLaunchKernelGGL(nw_files_interleave_kernel, dim3(t.audio_items), dim3(256), 0, stream, t.tab, t.rows, t.audio, d_adpcm, d_images);
        VGA_HIP_TRY(hipGetLastError());
    }
    return VGA_OK;
}

int launch_read_images(const DeviceTables &t, const uint8_t *d_images, uint8_t *d_adpcm, int16_t *d_coefs, int16_t *d_gain,
                       int16_t *d_start_context, int16_t *d_loop_context, hipStream_t stream)
{
    if (t.channels <= 0) return VGA_OK;
    if (d_coefs || d_gain || d_start_context || d_loop_context) {
        hipLaunchKernelGGL(nw_files_meta_kernel, dim3((t.channels + 63) / 64), dim3(64), 0, stream, t.meta, t.channels, d_coefs, d_gain,
                           d_start_context, d_loop_context);
        VGA_HIP_TRY(hipGetLastError());
    }
    if (t.audio_items > 0) {
        hipLaunchKernelGGL(nw_files_deinterleave_kernel, dim3(t.audio_items), dim3(256), 0, stream, t.tab, t.rows, t.audio, d_images, d_adpcm);
        VGA_HIP_TRY(hipGetLastError());
    }
    return VGA_OK;
}

}  // namespace nwf
}  // namespace vga
