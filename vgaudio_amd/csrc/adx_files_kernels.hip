// adx_files_kernels.hip -- the kernels of include/vgaudio_hip/adx_files.h: the ADX images of a SET of files of different
// shapes, every kernel one launch over tables the set's object holds (adx_files_host.hpp).
//
//   adx_files_header_kernel        one workgroup per file: zeros up to the audio offset (or the end of the header fields), then
//                                  adx_header_body.hpp's fields and "(c)CRI" by one thread, as the per-file kernel writes them
//   adx_files_interleave_span_kernel, adx_files_deinterleave_span_kernel
//                                  18-byte frames: (file, span of frames) items through LDS, adx_span.hpp's bodies -- the read
//                                  side's is the per-file reader's, the write side's its mirror image
//   adx_files_interleave_kernel, adx_files_deinterleave_kernel
//                                  every other file: one thread per granule of the OUTPUT (coalesced stores; loads are runs of
//                                  one frame of one channel), (file or row, chunk of 2048 granules) items, no LDS
//   adx_files_footer_kernel        one workgroup per file: the four footer bytes where the audio ended, zeros to the image's end
//   adx_files_history_kernel       the read side's parsed start histories out of the object's table
// All of it is byte movement: HBM-bound, every byte read once and written once.
#include "common.hpp"
#include "adx_files_kernels.hpp"
#include "adx_header_body.hpp"
#include "container_kernels.hpp"

namespace vga {
namespace adxf {

using container::Granule;

// [from, to) of an image whose base is 16-byte aligned -> zeros: single bytes up to the grid, vectors, single bytes
__device__ __forceinline__ void zero_range(uint8_t *__restrict__ image, int from, int to)
{
    const int a = min((from + 15) & ~15, to), b = max(to & ~15, a);
    for (int i = from + (int)threadIdx.x; i < a; i += 256) image[i] = 0;
    for (int i = a + 16 * (int)threadIdx.x; i < b; i += 16 * 256) *reinterpret_cast<uint4 *>(image + i) = make_uint4(0, 0, 0, 0);
    for (int i = b + (int)threadIdx.x; i < to; i += 256) image[i] = 0;
}

__global__ __launch_bounds__(256) void adx_files_header_kernel(const FileTab *__restrict__ tab, const int16_t *__restrict__ history,
                                                               uint8_t *__restrict__ images)
{
    const FileTab &t = tab[blockIdx.x];
    uint8_t *image = images + t.image_off;
    zero_range(image, 0, t.header_end);
    __syncthreads();
    if (threadIdx.x == 0) container::adx_write_header(t.h, history + t.first_channel, image);
}

// after the audio: 0x8001 and the padding's size at footer_pos, zeros behind them -- but not over header fields that ran
// past that point (the reference's footer is four bytes into an image that already holds the header)
__global__ __launch_bounds__(256) void adx_files_footer_kernel(const FileTab *__restrict__ tab, uint8_t *__restrict__ images)
{
    const FileTab &t = tab[blockIdx.x];
    uint8_t *image = images + t.image_off;
    zero_range(image, min(max(t.h.footer_pos + 4, t.header_end), t.h.file_size), t.h.file_size);
    if (threadIdx.x == 0) container::adx_write_footer(t.h, image);
}

__global__ __launch_bounds__(256) void adx_files_interleave_span_kernel(const FileTab *__restrict__ tab, const int64_t *__restrict__ row_off,
                                                                        const Item *__restrict__ items, const uint8_t *__restrict__ audio,
                                                                        uint8_t *__restrict__ images)
{
    __shared__ __align__(16) uint8_t lds[adxspan::kLdsBytes];
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[it.x];
    const int64_t *rows = row_off + t.first_channel;
    adxspan::interleave_span(lds, [&](int c) { return audio + rows[c]; }, t.h.nch, t.copy_frames, (int)it.y, t.span_frames,
                             images + t.image_off + t.audio_offset);
}

__global__ __launch_bounds__(256) void adx_files_deinterleave_span_kernel(const FileTab *__restrict__ tab, const int64_t *__restrict__ row_off,
                                                                          const Item *__restrict__ items, const uint8_t *__restrict__ images,
                                                                          uint8_t *__restrict__ audio)
{
    __shared__ __align__(16) uint8_t lds[adxspan::kLdsBytes];
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[it.x];
    const int64_t *rows = row_off + t.first_channel;
    adxspan::deinterleave_span(lds, images + t.image_off + t.audio_offset, t.h.nch, t.copy_frames, (int)it.y, t.span_frames,
                               [&](int c) { return audio + rows[c]; });
}

// G bytes at dst from src, or the first n of them singly (the end of a mono file's plain copy)
template <int G>
__device__ __forceinline__ void move_granule(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, int64_t n)
{
    using T = typename Granule<G>::type;
    if (n >= G) *reinterpret_cast<T *>(dst) = *reinterpret_cast<const T *>(src);
    else for (int k = 0; k < (int)n; k++) dst[k] = src[k];
}

// Interleave(channels, FrameSize, FrameCount * FrameSize) (Interleave.cs:43-78) of the frames the rows hold: output byte o of
// the file's audio is byte w of frame fr of channel c, o = (fr * nch + c) * frame_size + w.  G divides the frame size
// (several channels), every row offset and where the audio starts, so a granule never straddles two runs.
template <int G>
__device__ __forceinline__ void interleave_chunk(const FileTab &t, const int64_t *__restrict__ rows, uint32_t chunk,
                                                 const uint8_t *__restrict__ audio, uint8_t *__restrict__ out)
{
    const int nch = t.h.nch, fs = t.h.frame_size;
    const int64_t total = (int64_t)t.copy_frames * fs * nch, group = (int64_t)fs * nch;
#pragma unroll
    for (int q = 0; q < CHUNK_GRANULES / 256; q++) {
        const int64_t o = ((int64_t)chunk * CHUNK_GRANULES + q * 256 + threadIdx.x) * G;
        if (o >= total) return;
        const int64_t fr = o / group;
        const int r = (int)(o - fr * group), c = r / fs, w = r - c * fs;
        move_granule<G>(out + o, audio + rows[c] + fr * fs + w, total - o);
    }
}

__global__ __launch_bounds__(256) void adx_files_interleave_kernel(const FileTab *__restrict__ tab, const int64_t *__restrict__ row_off,
                                                                   const Item *__restrict__ items, const uint8_t *__restrict__ audio,
                                                                   uint8_t *__restrict__ images)
{
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[it.x];
    const int64_t *rows = row_off + t.first_channel;
    uint8_t *out = images + t.image_off + t.audio_offset;
    switch (t.granule) {                                       // uniform per workgroup
    case 16: interleave_chunk<16>(t, rows, it.y, audio, out); break;
    case 8: interleave_chunk<8>(t, rows, it.y, audio, out); break;
    case 4: interleave_chunk<4>(t, rows, it.y, audio, out); break;
    case 2: interleave_chunk<2>(t, rows, it.y, audio, out); break;
    default: interleave_chunk<1>(t, rows, it.y, audio, out); break;
    }
}

// DeInterleave(audioSize, FrameSize, ChannelCount) (Interleave.cs:118-167): byte `off` of channel c's row is byte
// (fr * nch + c) * frame_size + w of the image's audio, off = fr * frame_size + w
template <int G>
__device__ __forceinline__ void deinterleave_chunk(const FileTab &t, int c, uint32_t chunk, const uint8_t *__restrict__ in,
                                                   uint8_t *__restrict__ row)
{
    const int nch = t.h.nch, fs = t.h.frame_size;
    const int64_t total = (int64_t)t.copy_frames * fs;
#pragma unroll
    for (int q = 0; q < CHUNK_GRANULES / 256; q++) {
        const int64_t off = ((int64_t)chunk * CHUNK_GRANULES + q * 256 + threadIdx.x) * G;
        if (off >= total) return;
        const int64_t fr = off / fs;
        const int w = (int)(off - fr * fs);
        move_granule<G>(row + off, in + (fr * nch + c) * fs + w, total - off);
    }
}

__global__ __launch_bounds__(256) void adx_files_deinterleave_kernel(const FileTab *__restrict__ tab, const int64_t *__restrict__ row_off,
                                                                     const int *__restrict__ row_file, const Item *__restrict__ items,
                                                                     const uint8_t *__restrict__ images, uint8_t *__restrict__ audio)
{
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[row_file[it.x]];
    const int c = it.x - t.first_channel;
    const uint8_t *in = images + t.image_off + t.audio_offset;
    uint8_t *row = audio + row_off[it.x];
    switch (t.granule) {
    case 16: deinterleave_chunk<16>(t, c, it.y, in, row); break;
    case 8: deinterleave_chunk<8>(t, c, it.y, in, row); break;
    case 4: deinterleave_chunk<4>(t, c, it.y, in, row); break;
    case 2: deinterleave_chunk<2>(t, c, it.y, in, row); break;
    default: deinterleave_chunk<1>(t, c, it.y, in, row); break;
    }
}

__global__ __launch_bounds__(256) void adx_files_history_kernel(const int16_t *__restrict__ history, int nch, int16_t *__restrict__ out)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < nch) out[c] = history[c];
}

// ---------------------------------------------------------------- launchers
// The launches of a call one by one: the keyed calls (adx_keyed_files_kernels.hip) put their own between them.
int launch_write_headers(const DeviceTables &t, const int16_t *d_history, uint8_t *d_images, hipStream_t stream)
{
    hipLaunchKernelGGL(adx_files_header_kernel, dim3(t.files), dim3(256), 0, stream, t.tab, d_history, d_images);
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

int launch_write_general(const DeviceTables &t, bool general, const uint8_t *d_audio, uint8_t *d_images, hipStream_t stream)
{
    const int k = general ? 1 : 0, span = general ? 0 : t.span_items, rest = t.item_count[k] - span;
    if (rest <= 0) return VGA_OK;
    hipLaunchKernelGGL(adx_files_interleave_kernel, dim3(rest), dim3(256), 0, stream, t.tab, t.row_off, t.items[k] + span, d_audio, d_images);
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

int launch_write_footers(const DeviceTables &t, uint8_t *d_images, hipStream_t stream)
{
    hipLaunchKernelGGL(adx_files_footer_kernel, dim3(t.files), dim3(256), 0, stream, t.tab, d_images);
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

int launch_read_history(const DeviceTables &t, int16_t *d_history_out, hipStream_t stream)
{
    if (!d_history_out) return VGA_OK;
    hipLaunchKernelGGL(adx_files_history_kernel, dim3((t.channels + 255) / 256), dim3(256), 0, stream, t.history, t.channels, d_history_out);
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

int launch_read_general(const DeviceTables &t, bool general, const uint8_t *d_images, uint8_t *d_audio, hipStream_t stream)
{
    const int k = general ? 1 : 0, span = general ? 0 : t.span_items, rest = t.item_count[k] - span;
    if (rest <= 0) return VGA_OK;
    hipLaunchKernelGGL(adx_files_deinterleave_kernel, dim3(rest), dim3(256), 0, stream, t.tab, t.row_off, t.row_file, t.items[k] + span,
                       d_images, d_audio);
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

int launch_write_images(const DeviceTables &t, bool general, const uint8_t *d_audio, const int16_t *d_history, uint8_t *d_images,
                        hipStream_t stream)
{
    if (t.files <= 0) return VGA_OK;
    const int k = general ? 1 : 0, span = general ? 0 : t.span_items;
    if (int rc = launch_write_headers(t, d_history, d_images, stream)) return rc;
    if (span > 0) {
        hipLaunchKernelGGL(adx_files_interleave_span_kernel, dim3(span), dim3(256), 0, stream, t.tab, t.row_off, t.items[k], d_audio, d_images);
        VGA_HIP_TRY(hipGetLastError());
    }
    if (int rc = launch_write_general(t, general, d_audio, d_images, stream)) return rc;
    return launch_write_footers(t, d_images, stream);
}

int launch_read_images(const DeviceTables &t, bool general, const uint8_t *d_images, uint8_t *d_audio, int16_t *d_history_out,
                       hipStream_t stream)
{
    if (t.channels <= 0) return VGA_OK;
    const int k = general ? 1 : 0, span = general ? 0 : t.span_items;
    if (int rc = launch_read_history(t, d_history_out, stream)) return rc;
    if (span > 0) {
        hipLaunchKernelGGL(adx_files_deinterleave_span_kernel, dim3(span), dim3(256), 0, stream, t.tab, t.row_off, t.items[k], d_images, d_audio);
        VGA_HIP_TRY(hipGetLastError());
    }
    return launch_read_general(t, general, d_images, d_audio, stream);
}

}  // namespace adxf
}  // namespace vga
