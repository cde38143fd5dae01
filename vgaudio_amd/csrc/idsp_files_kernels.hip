// idsp_files_kernels.hip -- the kernels of include/vgaudio_hip_files/idsp_files.h: the IDSP images of a SET of files of different
// shapes, every kernel one launch over tables the set's object holds (idsp_files_host.hpp).
//
//   idsp_files_header_kernel        IdspWriter.WriteHeader (:63-96) of every file: one workgroup per file, a thread builds one
//                                   word of four bytes and stores it (headers are multiples of 0x20 at 16-byte offsets)
//   idsp_files_interleave_kernel    Interleave(channels, InterleaveSize, AudioDataSize) of every file: gc_files_chunks.hpp's
//                                   interleave_chunk over (file, chunk) work items
//   idsp_files_meta_kernel, idsp_files_deinterleave_kernel   the read side: the parsed per-channel arrays out of the object's
//                                   table, and deinterleave_chunk over (row, chunk) work items
// The audio kernels are copies: one thread per granule of the OUTPUT (coalesced stores), loads are contiguous runs of one
// channel, no LDS.  The granule (16 or 8 bytes; single bytes for a foreign file read whose geometry is on no 8) is uniform
// per work item and chosen on the host.
#include "common.hpp"
#include "gc_files_chunks.hpp"
#include "idsp_files_kernels.hpp"

namespace vga {
namespace idf {

// the memory word of a big-endian int / of two big-endian shorts
__device__ __forceinline__ uint32_t be32(int v) { return __builtin_bswap32((uint32_t)v); }
__device__ __forceinline__ uint32_t be16x2(int first, int second) { return be32((int)(((uint32_t)first << 16) | ((uint32_t)second & 0xFFFFu))); }

// word w (bytes 4 * w .. 4 * w + 3) of the header of the file of table entry t: idsp_header_kernel's fields (gc_containers.hip),
// every one of which lies on 4 bytes or is one of two shorts that share a word
__device__ __forceinline__ uint32_t header_word(const FileTab &t, int w, const ChannelRow *__restrict__ rows, const uint8_t *__restrict__ adpcm,
                                                const int16_t *__restrict__ coefs, const int16_t *__restrict__ gain,
                                                const int16_t *__restrict__ start, const int16_t *__restrict__ loop)
{
    const HeaderGeom &a = t.h;
    constexpr int kStreamWords = gcs::kIdspStreamInfoSize / 4, kChannelWords = gcs::kIdspChannelInfoSize / 4;
    if (w < kStreamWords) {
        switch (w) {
        case 0: return 0x50534449u;                            // "IDSP"
        case 2: return be32(a.nch);
        case 3: return be32(a.sample_rate);
        case 4: return be32(a.sample_count);
        case 5: return be32(a.loop_start);
        case 6: return be32(a.loop_end);
        case 7: return be32(a.block_size);
        case 8: return be32(gcs::kIdspStreamInfoSize);
        case 9: return be32(gcs::kIdspChannelInfoSize);
        case 10: return be32(a.header_size);
        case 11: return be32(a.audio_data_size);
        default: return 0;
        }
    }
    const int c = (w - kStreamWords) / kChannelWords, q = (w - kStreamWords) % kChannelWords;
    const int64_t row = (int64_t)t.audio.first_channel + c;
    if (q >= 7 && q < 15) return be16x2(coefs[row * 16 + (q - 7) * 2], coefs[row * 16 + (q - 7) * 2 + 1]);
    // GcAdpcmChannel.StartContext: the caller's, or (adpcm[0], 0, 0) -- 0 for a row of no bytes
    auto start_ctx = [&](int i) -> int {
        if (start) return start[row * 3 + i];
        return i == 0 && t.audio.input_size > 0 ? adpcm[rows[row].adpcm_off] : 0;
    };
    switch (q) {
    case 0: return be32(a.channel_sample_count);
    case 1: return be32(a.channel_nibble_count);
    case 2: return be32(a.sample_rate);
    case 3: return be16x2(a.looping, 0);                       // (short)Looping, (short)0
    case 4: return be32(a.start_addr);
    case 5: return be32(a.end_addr);
    case 6: return be32(a.cur_addr);
    case 15: return be16x2(gain ? gain[row] : 0, start_ctx(0));
    case 16: return be16x2(start_ctx(1), start_ctx(2));
    case 17: return be16x2(loop ? loop[row * 3] : 0, loop ? loop[row * 3 + 1] : 0);
    case 18: return be16x2(loop ? loop[row * 3 + 2] : 0, 0);
    default: return 0;
    }
}

// one workgroup per file, one thread per word: headers are multiples of 0x20 at 16-byte offsets
__global__ __launch_bounds__(64) void idsp_files_header_kernel(const FileTab *__restrict__ tab, const ChannelRow *__restrict__ rows,
                                                               const uint8_t *__restrict__ adpcm, const int16_t *__restrict__ coefs,
                                                               const int16_t *__restrict__ gain, const int16_t *__restrict__ start_ctx,
                                                               const int16_t *__restrict__ loop_ctx, uint8_t *__restrict__ images)
{
    const FileTab &t = tab[blockIdx.x];
    uint32_t *image = reinterpret_cast<uint32_t *>(images + t.audio.image_off);
    const int words = t.h.header_size / 4;
    for (int w = (int)threadIdx.x; w < words; w += 64) image[w] = header_word(t, w, rows, adpcm, coefs, gain, start_ctx, loop_ctx);
}

__global__ __launch_bounds__(256) void idsp_files_interleave_kernel(const FileTab *__restrict__ tab, const ChannelRow *__restrict__ rows,
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
__global__ __launch_bounds__(64) void idsp_files_meta_kernel(const ChannelMeta *__restrict__ meta, int nch, int16_t *__restrict__ coefs,
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

__global__ __launch_bounds__(256) void idsp_files_deinterleave_kernel(const FileTab *__restrict__ tab, const ChannelRow *__restrict__ rows,
                                                                      const Item *__restrict__ items, const uint8_t *__restrict__ images,
                                                                      uint8_t *__restrict__ adpcm)
{
    const Item it = items[blockIdx.x];
    const ChannelRow r = rows[it.x];
    const gcf::FileGeom g = tab[r.file].audio;
    const bool g16 = (it.y >> 31) != 0, g1 = (g.granule16 & GRANULE1) != 0;
    const uint32_t start = (it.y & 0x7FFFFFFFu) << 3;
    const uint32_t chunk = g1 ? (uint32_t)CHUNK_BYTES1 : (uint32_t)gcf::CHUNK_GRANULES * (g16 ? 16u : 8u);
    const uint32_t end = g.output_size - start < chunk ? g.output_size : start + chunk;
    const uint8_t *audio = images + g.image_off + tab[r.file].audio_offset;
    if (g1) gcf::deinterleave_chunk<1>(g, it.x - g.first_channel, audio, adpcm + r.adpcm_off, start, end);
    else if (g16) gcf::deinterleave_chunk<16>(g, it.x - g.first_channel, audio, adpcm + r.adpcm_off, start, end);
    else gcf::deinterleave_chunk<8>(g, it.x - g.first_channel, audio, adpcm + r.adpcm_off, start, end);
}

// ---------------------------------------------------------------- launchers
int launch_write_images(const DeviceTables &t, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *d_gain,
                        const int16_t *d_start_context, const int16_t *d_loop_context, uint8_t *d_images, hipStream_t stream, int *launches)
{
    *launches = 0;
    if (t.files <= 0) return VGA_OK;
    hipLaunchKernelGGL(idsp_files_header_kernel, dim3(t.files), dim3(64), 0, stream, t.tab, t.rows, d_adpcm, d_coefs, d_gain, d_start_context,
                       d_loop_context, d_images);
    VGA_HIP_TRY(hipGetLastError());
    ++*launches;
    if (t.audio_items > 0) {
        hipLaunchKernelGGL(idsp_files_interleave_kernel, dim3(t.audio_items), dim3(256), 0, stream, t.tab, t.rows, t.audio, d_adpcm, d_images);
        VGA_HIP_TRY(hipGetLastError());
        ++*launches;
    }
    return VGA_OK;
}

int launch_read_images(const DeviceTables &t, const uint8_t *d_images, uint8_t *d_adpcm, int16_t *d_coefs, int16_t *d_gain,
                       int16_t *d_start_context, int16_t *d_loop_context, hipStream_t stream, int *launches)
{
    *launches = 0;
    if (t.channels <= 0) return VGA_OK;
    if (d_coefs || d_gain || d_start_context || d_loop_context) {
        hipLaunchKernelGGL(idsp_files_meta_kernel, dim3((t.channels + 63) / 64), dim3(64), 0, stream, t.meta, t.channels, d_coefs, d_gain,
                           d_start_context, d_loop_context);
        VGA_HIP_TRY(hipGetLastError());
        ++*launches;
    }
    if (t.audio_items > 0) {
        hipLaunchKernelGGL(idsp_files_deinterleave_kernel, dim3(t.audio_items), dim3(256), 0, stream, t.tab, t.rows, t.audio, d_images, d_adpcm);
        VGA_HIP_TRY(hipGetLastError());
        ++*launches;
    }
    return VGA_OK;
}

}  // namespace idf
}  // namespace vga
