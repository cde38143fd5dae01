// pcm_kernels.hip -- PCM in the NintendoWare streams: the writers' Interleave and the readers' DeInterleave fused with
// the sample conversion (a byte swap for PCM16 in the other byte order, Pcm8Codec.EncodeSigned / DecodeSigned for
// PCM8), and Pcm8Codec (Codecs/Pcm8/Pcm8Codec.cs) over pitched planar rows.  Everything here is byte movement:
// HBM-bound, every byte read and written once.
#include "common.hpp"
#include "container_kernels.hpp"
#include "pcm_kernels.hpp"
#include "../../include/vgaudio_hip_pcm.h"

#include <algorithm>

using namespace vga;

namespace vga {
namespace pcm {

using container::Granule;
using container::kMaxGridY;

// N bytes from / to an address aligned to min(N, 16), as whole 16-byte (or smaller) words
template <int N>
__device__ __forceinline__ void load_bytes(const void *p, uint8_t (&out)[N])
{
    constexpr int W = N < 16 ? N : 16;
    using L = typename Granule<W>::type;
    L w[N / W];
#pragma unroll
    for (int j = 0; j < N / W; j++) w[j] = reinterpret_cast<const L *>(p)[j];
    memcpy(out, w, N);
}
template <int N>
__device__ __forceinline__ void store_bytes(void *p, const uint8_t (&in)[N])
{
    constexpr int W = N < 16 ? N : 16;
    using L = typename Granule<W>::type;
    L w[N / W];
    memcpy(w, in, N);
#pragma unroll
    for (int j = 0; j < N / W; j++) reinterpret_cast<L *>(p)[j] = w[j];
}

// The counterpart of container::interleave_files_kernel for int16 rows: blockIdx.y is the file, one thread per G-byte
// granule of the OUTPUT (coalesced stores).  Offsets are in bytes of the channel as stored: byte q of a PCM16 channel
// is byte q ^ 1 of its row (kSwap16), byte q of a PCM8 channel the high byte of row sample q (kPcm8: a granule reads
// 2G bytes).  G divides the interleave and the last block; PCM16 blocks are even, so a sample never straddles two.
// Every byte of the region is written, the zeros the reference leaves in its MemoryStream included.
template <int G, int C>
__global__ __launch_bounds__(256) void pcm_interleave_files_kernel(const int16_t *__restrict__ src, int64_t pitch, int nch,
                                                                   uint32_t input_size, uint32_t interleave,
                                                                   uint32_t output_size, uint8_t *__restrict__ dst,
                                                                   int64_t file_pitch)
{
    using T = typename Granule<G>::type;
    const uint64_t o64 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * G;
    if (o64 >= (uint64_t)output_size * nch) return;
    const uint32_t o = (uint32_t)o64;
    const int f = blockIdx.y;
    const uint32_t in_blocks = (input_size + interleave - 1) / interleave, out_blocks = (output_size + interleave - 1) / interleave;
    const uint32_t stride = interleave * nch;
    uint32_t b = o / stride;
    if (b > out_blocks - 1) b = out_blocks - 1;
    const uint32_t r = o - b * stride;
    const uint32_t cur_out = b == out_blocks - 1 ? output_size - (out_blocks - 1) * interleave : interleave;
    const uint32_t i = r / cur_out, within = r - i * cur_out;
    uint32_t n = 0;
    if (b < in_blocks) {
        const uint32_t cur_in = b == in_blocks - 1 ? input_size - (in_blocks - 1) * interleave : interleave;
        n = cur_in < cur_out ? cur_in : cur_out;
    }
    const int16_t *row = src + (int64_t)(f * nch + (int)i) * pitch;
    const uint32_t q0 = interleave * b + within;           // the channel's stored byte under this granule's first byte
    uint8_t out[G];
    if (within + G <= n && (C == kPcm8 || G >= 2)) {
        if constexpr (C == kSwap16) {
            uint8_t in[G];
            load_bytes<G>(reinterpret_cast<const uint8_t *>(row) + q0, in);
#pragma unroll
            for (int k = 0; k < G; k++) out[k] = in[k ^ 1];
        } else if constexpr (G >= 2) {
            // the high byte of every little-endian short (s >> 8), picked with v_perm from whole words: extracting
            // bytes in C++ lets the compiler narrow the 16-byte loads to byte loads (a third of the rate)
            uint8_t in[2 * G];
            load_bytes<2 * G>(row + q0, in);
            uint32_t w[G / 2], o[(G + 3) / 4];
            memcpy(w, in, 2 * G);
#pragma unroll
            for (int k = 0; k < (G + 3) / 4; k++)
                o[k] = __builtin_amdgcn_perm(G >= 4 ? w[2 * k + 1] : 0u, w[2 * k], 0x07050301u);
            memcpy(out, o, G);
        } else {
            out[0] = (uint8_t)(row[q0] >> 8);
        }
    } else {
        for (int k = 0; k < G; k++) {
            const uint32_t q = q0 + k;
            if (within + k >= n) out[k] = 0;
            else if (C == kSwap16) out[k] = reinterpret_cast<const uint8_t *>(row)[q ^ 1];
            else out[k] = (uint8_t)(row[q] >> 8);
        }
    }
    T v;
    memcpy(&v, out, G);
    *reinterpret_cast<T *>(dst + (int64_t)f * file_pitch + o) = v;
}

// The counterpart of container::deinterleave_kernel: blockIdx.y = file * nch + channel, one thread per G bytes of the
// channel as stored (output_size bytes), coalesced stores into the int16 row: G bytes for kSwap16, 2G for kPcm8.
// Samples no block supplies stay zero, as in the reference's fresh byte[outputSize].
template <int G, int C>
__global__ __launch_bounds__(256) void pcm_deinterleave_kernel(const uint8_t *__restrict__ files, int64_t file_pitch,
                                                               int audio_offset, int nch, uint32_t input_size,
                                                               uint32_t interleave, uint32_t output_size,
                                                               int16_t *__restrict__ dst, int64_t dst_pitch, int row0)
{
    const uint32_t off = ((uint32_t)blockIdx.x * 256 + threadIdx.x) * G;
    if (off >= output_size) return;
    const int row = row0 + blockIdx.y, f = row / nch, o = row - f * nch;
    const uint32_t in_blocks = (input_size + interleave - 1) / interleave, out_blocks = (output_size + interleave - 1) / interleave;
    const uint32_t to_copy = in_blocks < out_blocks ? in_blocks : out_blocks;
    const uint32_t b = off / interleave, within = off - b * interleave;
    uint32_t n = 0, cur_in = interleave;
    if (b < to_copy) {
        cur_in = b == in_blocks - 1 ? input_size - (in_blocks - 1) * interleave : interleave;
        const uint32_t cur_out = b == out_blocks - 1 ? output_size - (out_blocks - 1) * interleave : interleave;
        n = cur_in < cur_out ? cur_in : cur_out;
    }
    const uint8_t *seg = files + (int64_t)f * file_pitch + audio_offset + (uint64_t)interleave * b * nch + (uint64_t)cur_in * o;
    int16_t *d = dst + (int64_t)row * dst_pitch;
    const bool whole = within + G <= n && off + G <= output_size;
    if constexpr (C == kSwap16) {
        uint8_t *db = reinterpret_cast<uint8_t *>(d) + off;
        if (whole && G >= 2) {
            uint8_t in[G], out[G];
            load_bytes<G>(seg + within, in);
#pragma unroll
            for (int k = 0; k < G; k++) out[k] = in[k ^ 1];
            store_bytes<G>(db, out);
            return;
        }
        for (int k = 0; k < G && off + k < output_size; k++) {
            const uint32_t q = within + k;                  // n is even: q < n exactly when q ^ 1 < n
            db[k] = q < n ? seg[q ^ 1] : 0;
        }
    } else {
        if (whole) {
            uint8_t in[G], out[2 * G];
            load_bytes<G>(seg + within, in);
#pragma unroll
            for (int k = 0; k < G; k++) { out[2 * k] = 0; out[2 * k + 1] = in[k]; }   // (short)(b << 8)
            store_bytes<2 * G>(d + off, out);
            return;
        }
        for (int k = 0; k < G && off + k < output_size; k++)
            d[off + k] = within + k < n ? (int16_t)(seg[within + k] << 8) : 0;
    }
}

template <class F>
int pick(uint64_t align, F &&go) { return container::pick_granule(align, std::forward<F>(go)); }

int launch_interleave_files(Conv conv, const int16_t *src, int64_t pitch, int nch, int nfiles, uint32_t input_size,
                            uint32_t interleave, uint32_t output_size, uint8_t *dst, int64_t file_pitch, hipStream_t s)
{
    const uint64_t total = (uint64_t)output_size * nch;
    if (total == 0 || nfiles == 0) return VGA_OK;
    const uint32_t out_blocks = (output_size + interleave - 1) / interleave, last_out = output_size - (out_blocks - 1) * interleave;
    // the output side as container::launch_interleave_files; the row side in bytes (kSwap16) or samples (kPcm8)
    uint64_t align = (uint64_t)(uintptr_t)dst | (uint64_t)(nfiles > 1 ? file_pitch : 0) | interleave | last_out;
    align |= conv == kSwap16 ? ((uint64_t)(uintptr_t)src | (uint64_t)pitch * 2) : ((uint64_t)(uintptr_t)src >> 1 | (uint64_t)pitch);
    for (int f0 = 0; f0 < nfiles; f0 += kMaxGridY) {
        const int nf = std::min(nfiles - f0, kMaxGridY);
        const int16_t *s0 = src ? src + (int64_t)f0 * nch * pitch : nullptr;
        uint8_t *d0 = dst + (int64_t)f0 * file_pitch;
        if (int rc = pick(align, [&](auto g) {
                constexpr int G = decltype(g)::value;
                const dim3 grid((unsigned)((total / G + 255) / 256), nf);
                if (conv == kSwap16)
                    hipLaunchKernelGGL((pcm_interleave_files_kernel<G, kSwap16>), grid, dim3(256), 0, s, s0, pitch, nch,
                                       input_size, interleave, output_size, d0, file_pitch);
                else
                    hipLaunchKernelGGL((pcm_interleave_files_kernel<G, kPcm8>), grid, dim3(256), 0, s, s0, pitch, nch,
                                       input_size, interleave, output_size, d0, file_pitch);
            }))
            return rc;
    }
    return VGA_OK;
}

int launch_deinterleave(Conv conv, const uint8_t *files, int64_t file_pitch, int audio_offset, int nch, int rows,
                        uint32_t input_size, uint32_t interleave, uint32_t output_size, int16_t *dst, int64_t dst_pitch,
                        hipStream_t s)
{
    if (rows == 0 || output_size == 0) return VGA_OK;
    const uint32_t in_blocks = input_size ? (input_size + interleave - 1) / interleave : 0;
    const uint32_t last_in = input_size ? input_size - (in_blocks - 1) * interleave : 0;
    uint64_t align = (uint64_t)(uintptr_t)files | (uint64_t)(rows > nch ? file_pitch : 0) | (uint64_t)audio_offset | interleave | last_in;
    align |= conv == kSwap16 ? ((uint64_t)(uintptr_t)dst | (uint64_t)dst_pitch * 2) : ((uint64_t)(uintptr_t)dst >> 1 | (uint64_t)dst_pitch);
    for (int r0 = 0; r0 < rows; r0 += kMaxGridY) {
        const int nr = std::min(rows - r0, kMaxGridY);
        if (int rc = pick(align, [&](auto g) {
                constexpr int G = decltype(g)::value;
                const dim3 grid((unsigned)(((output_size + G - 1) / G + 255) / 256), nr);
                if (conv == kSwap16)
                    hipLaunchKernelGGL((pcm_deinterleave_kernel<G, kSwap16>), grid, dim3(256), 0, s, files, file_pitch,
                                       audio_offset, nch, input_size, interleave, output_size, dst, dst_pitch, r0);
                else
                    hipLaunchKernelGGL((pcm_deinterleave_kernel<G, kPcm8>), grid, dim3(256), 0, s, files, file_pitch,
                                       audio_offset, nch, input_size, interleave, output_size, dst, dst_pitch, r0);
            }))
            return rc;
    }
    return VGA_OK;
}

// ---------------------------------------------------------------- Pcm8Codec over pitched rows
// Unsigned and signed bytes differ by their top bit: (s + 0x8000) >> 8 == (s >> 8) ^ 0x80, (b - 0x80) << 8 ==
// (sbyte)(b ^ 0x80) << 8.  One thread per sample, blockIdx.y the row.
__global__ __launch_bounds__(256) void pcm8_encode_kernel(const int16_t *__restrict__ in, int64_t in_pitch, int n,
                                                          uint8_t flip, uint8_t *__restrict__ out, int64_t out_pitch, int row0)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int64_t r = row0 + blockIdx.y;
    out[r * out_pitch + k] = (uint8_t)(in[r * in_pitch + k] >> 8) ^ flip;
}

__global__ __launch_bounds__(256) void pcm8_decode_kernel(const uint8_t *__restrict__ in, int64_t in_pitch, int n,
                                                          uint8_t flip, int16_t *__restrict__ out, int64_t out_pitch, int row0)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int64_t r = row0 + blockIdx.y;
    out[r * out_pitch + k] = (int16_t)((int8_t)(in[r * in_pitch + k] ^ flip) * 256);
}

}  // namespace pcm
}  // namespace vga

extern "C" {

int vga_pcm8_encode_device(const int16_t *d_pcm, int64_t pcm_pitch, int n, int nrows, int signed_, uint8_t *d_out,
                           int64_t out_pitch, void *stream)
{
    if (n < 0 || nrows < 0) { set_error("negative size"); return VGA_ERR_ARGUMENT; }
    if (n == 0 || nrows == 0) return VGA_OK;
    if (!d_pcm || !d_out || pcm_pitch < n || out_pitch < n) { set_error("null pointer / pitch < sample count"); return VGA_ERR_ARGUMENT; }
    for (int r0 = 0; r0 < nrows; r0 += pcm::kMaxGridY) {
        const int nr = std::min(nrows - r0, pcm::kMaxGridY);
        hipLaunchKernelGGL(pcm::pcm8_encode_kernel, dim3((n + 255) / 256, nr), dim3(256), 0, (hipStream_t)stream, d_pcm,
                           pcm_pitch, n, (uint8_t)(signed_ ? 0 : 0x80), d_out, out_pitch, r0);
        VGA_HIP_TRY(hipGetLastError());
    }
    return VGA_OK;
}

int vga_pcm8_decode_device(const uint8_t *d_in, int64_t in_pitch, int n, int nrows, int signed_, int16_t *d_pcm,
                           int64_t pcm_pitch, void *stream)
{
    if (n < 0 || nrows < 0) { set_error("negative size"); return VGA_ERR_ARGUMENT; }
    if (n == 0 || nrows == 0) return VGA_OK;
    if (!d_in || !d_pcm || pcm_pitch < n || in_pitch < n) { set_error("null pointer / pitch < sample count"); return VGA_ERR_ARGUMENT; }
    for (int r0 = 0; r0 < nrows; r0 += pcm::kMaxGridY) {
        const int nr = std::min(nrows - r0, pcm::kMaxGridY);
        hipLaunchKernelGGL(pcm::pcm8_decode_kernel, dim3((n + 255) / 256, nr), dim3(256), 0, (hipStream_t)stream, d_in,
                           in_pitch, n, (uint8_t)(signed_ ? 0 : 0x80), d_pcm, pcm_pitch, r0);
        VGA_HIP_TRY(hipGetLastError());
    }
    return VGA_OK;
}

}  // extern "C"
