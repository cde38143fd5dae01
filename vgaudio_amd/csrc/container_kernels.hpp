// container_kernels.hpp -- launchers for the container-image kernels
#pragma once
#include "common.hpp"
#include "adx_file_host.hpp"

#include <algorithm>
#include <cstring>
#include <type_traits>

namespace vga {
namespace container {

// Host tables and headers reach the device as kernel arguments, in stream order: no staging copy from pageable memory, no
// wait for the stream, and nothing to keep alive after the launch (the *_device entry points never synchronise).  A launch
// carries N elements of T (at most a few KiB of arguments); longer tables take several launches.
template <class T, int N> struct TableChunk { T v[N]; };
template <class T, int N>
__global__ __launch_bounds__(256) void table_upload_kernel(TableChunk<T, N> c, int n, T *__restrict__ dst)
{
    for (int i = threadIdx.x; i < n; i += 256) dst[i] = c.v[i];
}

// host[0 .. n) -> dst[0 .. n) on stream s (dst: device memory at T's alignment)
template <class T, int N = 64>
int upload_to(const T *host, int n, T *dst, hipStream_t s)
{
    static_assert(sizeof(TableChunk<T, N>) <= 2048, "a chunk must stay well under the 4 KiB kernel-argument limit");
    for (int i = 0; i < n; i += N) {
        TableChunk<T, N> c;
        const int k = std::min(N, n - i);
        std::memcpy(c.v, host + i, (size_t)k * sizeof(T));
        hipLaunchKernelGGL((table_upload_kernel<T, N>), dim3(1), dim3(256), 0, s, c, k, dst + i);
        VGA_HIP_TRY(hipGetLastError());
    }
    return VGA_OK;
}

// the same into stream-ordered scratch that lives until `buf` goes out of scope (hipFreeAsync on s)
template <class T>
int upload_table(const T *host, int n, AsyncBuf &buf, hipStream_t s)
{
    VGA_HIP_TRY(buf.alloc((size_t)n * sizeof(T), s));
    return upload_to(host, n, buf.as<T>(), s);
}

// header bytes (built on the host) -> dst, 1 KiB per launch
inline int upload_bytes(const uint8_t *host, int n, uint8_t *dst, hipStream_t s) { return upload_to<uint8_t, 1024>(host, n, dst, s); }

// InterleaveExtensions.Interleave(byte[][], Stream, interleaveSize, outputSize) (Utilities/Interleave.cs:43-78) from
// `count` rows of `input_size` bytes (row r at src + r * pitch) into dst (output_size * count bytes, already zeroed).
int launch_interleave(const uint8_t *src, int64_t pitch, int input_size, int count, int interleave, int output_size,
                      uint8_t *dst, hipStream_t stream);

// (AdxHeaderArgs: adx_file_host.hpp, with the host code that fills it)
// AdxWriter.WriteHeader (:81-117); the footer (:133-138) is a second launch AFTER the audio, as in the reference
int launch_adx_header(const AdxHeaderArgs &a, const int16_t *d_history, uint8_t *d_file, hipStream_t stream);
int launch_adx_footer(const AdxHeaderArgs &a, uint8_t *d_file, hipStream_t stream);

// copies one header_size-byte header (device) to the front of `count` images `pitch` bytes apart
int launch_replicate(const uint8_t *d_header, int header_size, uint8_t *d_files, int64_t pitch, int count, hipStream_t stream);

// WAVE 16-bit PCM <-> planar channels (Utilities/Interleave.cs:188-207 InterleavedByteToShort, :168-186
// ShortToInterleavedByte).  `interleaved` is a little-endian byte stream at ANY alignment; planar row c at
// pcm + c * pitch (in samples).
int launch_pcm16_deinterleave(const uint8_t *interleaved, int sample_count, int nch, int16_t *pcm, int64_t pitch, hipStream_t stream);
int launch_pcm16_interleave(const int16_t *pcm, int64_t pitch, int sample_count, int nch, uint8_t *interleaved, hipStream_t stream);
// WAVE 8-bit PCM <-> planar rows: int16 rows (s16, through Pcm8Codec.Encode / Decode) or unsigned byte rows as stored
int launch_pcm8_deinterleave(const uint8_t *interleaved, int sample_count, int nch, void *rows, bool s16, int64_t pitch,
                             hipStream_t stream);
int launch_pcm8_interleave(const void *rows, bool s16, int64_t pitch, int sample_count, int nch, uint8_t *interleaved,
                           hipStream_t stream);


// ---------------------------------------------------------------- shared by the container readers
// (nwstm.hip: BRSTM / BCSTM / BFSTM; container_readers.hip: DSP and the general ADX path)

template <int G> struct Granule;
template <> struct Granule<1> { using type = uint8_t; };
template <> struct Granule<2> { using type = uint16_t; };
template <> struct Granule<4> { using type = uint32_t; };
template <> struct Granule<8> { using type = uint2; };
template <> struct Granule<16> { using type = uint4; };

constexpr int kMaxGridY = 65535;                 // rows of one de-interleave launch (grid y)

// DeInterleave(stream, length, InterleaveSize, ChannelCount, outputSize) (Utilities/Interleave.cs:118-167): the gather
// back to one row per channel.  blockIdx.y = file * nch + channel, one thread per G-byte granule of the output row
// (coalesced stores), reading the channel's contiguous run of its interleave block (coalesced loads).  Bytes of the
// row that no block supplies stay zero, as in the reference's fresh byte[outputSize].
template <int G>
__global__ __launch_bounds__(256) void deinterleave_kernel(const uint8_t *__restrict__ files, int64_t file_pitch,
                                                           int audio_offset, int nch, uint32_t input_size,
                                                           uint32_t interleave, uint32_t output_size,
                                                           uint8_t *__restrict__ dst, int64_t dst_pitch, int row0)
{
    using T = typename Granule<G>::type;
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
    const uint8_t *s = files + (int64_t)f * file_pitch + audio_offset + (uint64_t)interleave * b * nch + (uint64_t)cur_in * o + within;
    uint8_t *d = dst + (int64_t)row * dst_pitch + off;
    if (within + G <= n && off + G <= output_size) {
        *reinterpret_cast<T *>(d) = *reinterpret_cast<const T *>(s);
        return;
    }
    for (int k = 0; k < G && off + k < output_size; k++) d[k] = within + k < n ? s[k] : 0;
}

// Interleave(channels, InterleaveSize, outputSize) (Utilities/Interleave.cs:43-78) into the audio region of every
// image at once (the NW stream and IDSP writers): blockIdx.y is the file, one thread per G-byte granule of the OUTPUT
// (coalesced stores; the loads are contiguous runs inside one interleave block of one channel).  G divides the
// interleave and the last block, so a granule never straddles two rows.  Every byte of the region is written: what
// the reference leaves untouched in its zeroed MemoryStream is written as zero here, so the images need no memset.
template <int G>
__global__ __launch_bounds__(256) void interleave_files_kernel(const uint8_t *__restrict__ src, int64_t pitch, int nch,
                                                               uint32_t input_size, uint32_t interleave, uint32_t output_size,
                                                               uint8_t *__restrict__ dst, int64_t file_pitch)
{
    using T = typename Granule<G>::type;
    const uint64_t o64 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * G;
    if (o64 >= (uint64_t)output_size * nch) return;
    const uint32_t o = (uint32_t)o64;                      // images are < 2 GiB (FileSize is an int)
    const int f = blockIdx.y;
    const uint32_t in_blocks = (input_size + interleave - 1) / interleave, out_blocks = (output_size + interleave - 1) / interleave;
    const uint32_t stride = interleave * nch;
    uint32_t b = o / stride;
    if (b > out_blocks - 1) b = out_blocks - 1;            // the (short) last block's rows are packed more tightly
    const uint32_t r = o - b * stride;
    const uint32_t cur_out = b == out_blocks - 1 ? output_size - (out_blocks - 1) * interleave : interleave;
    const uint32_t i = r / cur_out, within = r - i * cur_out;
    uint32_t n = 0;                                        // bytes of this row segment that come from the channel
    if (b < in_blocks) {                                   // blocksToCopy = min(inBlockCount, outBlockCount)
        const uint32_t cur_in = b == in_blocks - 1 ? input_size - (in_blocks - 1) * interleave : interleave;
        n = cur_in < cur_out ? cur_in : cur_out;
    }
    const uint8_t *s = src + (int64_t)(f * nch + (int)i) * pitch + (uint64_t)interleave * b + within;
    T v;
    if (within + G <= n) {
        v = *reinterpret_cast<const T *>(s);
    } else {
        uint8_t tmp[G];
        for (int k = 0; k < G; k++) tmp[k] = within + k < n ? s[k] : 0;
        memcpy(&v, tmp, G);
    }
    *reinterpret_cast<T *>(dst + (int64_t)f * file_pitch + o) = v;
}

template <class F>
int pick_granule(uint64_t align, F &&go)
{
    if (!(align & 15)) go(std::integral_constant<int, 16>{});
    else if (!(align & 7)) go(std::integral_constant<int, 8>{});
    else if (!(align & 3)) go(std::integral_constant<int, 4>{});
    else if (!(align & 1)) go(std::integral_constant<int, 2>{});
    else go(std::integral_constant<int, 1>{});
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

// DeInterleave for `rows` rows (file = row / nch, channel = row % nch) of equally shaped images at files + f * file_pitch,
// each channel's audio `input_size` bytes in blocks of `interleave` bytes from audio_offset on, into rows of output_size
// bytes; `align` ORs every address and size the granule must divide.  One launch per 65535 rows.
inline int launch_deinterleave(uint64_t align, const uint8_t *files, int64_t file_pitch, int audio_offset, int nch, int rows,
                               uint32_t input_size, uint32_t interleave, uint32_t output_size, uint8_t *dst, int64_t dst_pitch,
                               hipStream_t s)
{
    for (int r0 = 0; r0 < rows; r0 += kMaxGridY) {
        const int nr = std::min(rows - r0, kMaxGridY);
        if (int rc = pick_granule(align, [&](auto g) {
                constexpr int G = decltype(g)::value;
                hipLaunchKernelGGL(deinterleave_kernel<G>, dim3((unsigned)(((output_size + G - 1) / G + 255) / 256), nr), dim3(256), 0, s,
                                   files, file_pitch, audio_offset, nch, input_size, interleave, output_size, dst, dst_pitch, r0);
            }))
            return rc;
    }
    return VGA_OK;
}

// Interleave for nfiles equally shaped images: file f's channel c is row f*nch+c of src (input_size bytes each),
// interleaved in blocks of `interleave` bytes into output_size * nch bytes at dst + f * file_pitch; `align` ORs every
// address, pitch and block size the granule must divide.  One launch per 65535 files.
inline int launch_interleave_files(uint64_t align, const uint8_t *src, int64_t pitch, int nch, int nfiles, uint32_t input_size,
                                   uint32_t interleave, uint32_t output_size, uint8_t *dst, int64_t file_pitch, hipStream_t s)
{
    const uint64_t total = (uint64_t)output_size * nch;
    if (total == 0) return VGA_OK;
    for (int f0 = 0; f0 < nfiles; f0 += kMaxGridY) {
        const int nf = std::min(nfiles - f0, kMaxGridY);
        if (int rc = pick_granule(align, [&](auto g) {
                constexpr int G = decltype(g)::value;
                hipLaunchKernelGGL(interleave_files_kernel<G>, dim3((unsigned)((total / G + 255) / 256), nf), dim3(256), 0, s,
                                   src ? src + (int64_t)f0 * nch * pitch : nullptr, pitch, nch, input_size, interleave,
                                   output_size, dst + (int64_t)f0 * file_pitch, file_pitch);
            }))
            return rc;
    }
    return VGA_OK;
}

}  // namespace container
}  // namespace vga
