// hps_files_kernels.hip -- the kernels of include/vgaudio_hip_files/hps_files.h: the HPS images of a SET of files of different
// shapes, every kernel one launch over tables the set's object holds (hps_files_host.hpp).
//
//   hps_files_header_kernel   one workgroup per file, then one per block of the set's block table.  A file's: the stream header
//                             and channel infos (HpsWriter.cs:59-83), zero up to HeaderSize.  A block's: WrittenSize, EndNibble,
//                             NextOffset, then per channel the pred/scale byte at start_sample / 14 * 8 of the row, hist1 and
//                             hist2 from the PCM row (:91-106), zero up to the written block header size.  A thread builds one
//                             word of four bytes and stores it: every field lies on 4 bytes or is one of two shorts of a word.
//   hps_files_body_kernel     the block bodies (:108-112) over (block, chunk) work items: channel c's ChannelSize bytes from
//                             ByteInIndex of its row, zero-padded to 0x20, one after the other; one 16-byte granule per thread
//                             and trip.  Every padded channel size is a multiple of 0x20, so a granule never straddles two
//                             channels; the granule that holds a channel's last byte writes the zeros behind it.
//   hps_files_meta_kernel, hps_files_gather_kernel   the read side: the parsed per-channel arrays out of the object's table,
//                             and HpsReader.ReadData (:89-128) over (block, channel, chunk) work items, 16-byte granules with
//                             a byte-wise ragged end, or byte by byte for a block of foreign geometry.
// The audio kernels are copies: coalesced 16-byte loads and stores, no LDS.
#include "common.hpp"
#include "hps_files_kernels.hpp"

namespace vga {
namespace hpf {

// the memory word of a big-endian int / of two big-endian shorts
__device__ __forceinline__ uint32_t be32(int v) { return __builtin_bswap32((uint32_t)v); }
__device__ __forceinline__ uint32_t be16x2(int first, int second) { return be32((int)(((uint32_t)first << 16) | ((uint32_t)second & 0xFFFFu))); }

// word w of the stream header and channel infos of the file of table entry t (hps_header_kernel's fields, gc_containers.hip)
__device__ __forceinline__ uint32_t stream_word(const FileTab &t, int w, const Row *__restrict__ rows, const uint8_t *__restrict__ adpcm,
                                                const int16_t *__restrict__ coefs, const int16_t *__restrict__ gain,
                                                const int16_t *__restrict__ start)
{
    constexpr int kChannelWords = 0x38 / 4;
    if (w == 0) return 0x4C414820u;                            // " HAL"
    if (w == 1) return 0x00545350u;                            // "PST\0"
    if (w == 2) return be32(t.sample_rate);
    if (w == 3) return be32(t.nch);
    const int c = (w - 4) / kChannelWords, q = (w - 4) % kChannelWords;
    if (c >= t.nch) return 0;
    const int64_t row = (int64_t)t.first_channel + c;
    if (q >= 4 && q < 12) return be16x2(coefs[row * 16 + (q - 4) * 2], coefs[row * 16 + (q - 4) * 2 + 1]);
    // GcAdpcmChannel.StartContext: the caller's, or (adpcm[0], 0, 0)
    auto start_ctx = [&](int i) -> int {
        if (start) return start[row * 3 + i];
        return i == 0 ? adpcm[rows[row].adpcm_off] : 0;
    };
    switch (q) {
    case 0: return be32(gcs::kHpsMaxBlockSize);
    case 1: return be32(2);                                    // SampleToNibble(0)
    case 2: return be32(t.end_address);
    case 3: return be32(2);
    case 12: return be16x2(gain ? gain[row] : 0, start_ctx(0));
    default: return be16x2(start_ctx(1), start_ctx(2));        // 13
    }
}

// word w of the header of block B
__device__ __forceinline__ uint32_t block_word(const FileTab &t, const Block &B, int w, const Row *__restrict__ rows,
                                               const uint8_t *__restrict__ adpcm, const int16_t *__restrict__ pcm)
{
    if (w == 0) return be32(B.w.written_size);
    if (w == 1) return be32(B.w.end_nibble);
    if (w == 2) return be32(B.w.next_offset);
    const int c = (w - 3) >> 1;
    if (c >= t.nch) return 0;
    const Row r = rows[t.first_channel + c];
    // GcAdpcmLoopContext.GetHist1 / GetHist2 over the Pcm field
    auto hist = [&](int k) -> int {
        const int i = B.w.start_sample - k;
        return i < 0 || !pcm ? 0 : pcm[r.pcm_off + i];
    };
    if (((w - 3) & 1) == 0) return be16x2(adpcm[r.adpcm_off + B.w.start_sample / 14 * 8], hist(1));   // GetPredScale(StartSample)
    return be16x2(hist(2), 0);
}

__global__ __launch_bounds__(64) void hps_files_header_kernel(const FileTab *__restrict__ tab, const Block *__restrict__ blocks, int files,
                                                              const Row *__restrict__ rows, const uint8_t *__restrict__ adpcm,
                                                              const int16_t *__restrict__ coefs, const int16_t *__restrict__ gain,
                                                              const int16_t *__restrict__ start_ctx, const int16_t *__restrict__ pcm,
                                                              uint8_t *__restrict__ images)
{
    if ((int)blockIdx.x < files) {
        const FileTab t = tab[blockIdx.x];
        uint32_t *image = reinterpret_cast<uint32_t *>(images + t.image_off);
        const int words = t.header_size / 4;
        for (int w = (int)threadIdx.x; w < words; w += 64) image[w] = stream_word(t, w, rows, adpcm, coefs, gain, start_ctx);
        return;
    }
    const Block B = blocks[(int)blockIdx.x - files];
    const FileTab t = tab[B.w.file];
    uint32_t *header = reinterpret_cast<uint32_t *>(images + t.image_off + B.w.offset);
    const int words = t.block_header_size / 4;
    for (int w = (int)threadIdx.x; w < words; w += 64) header[w] = block_word(t, B, w, rows, adpcm, pcm);
}

__global__ __launch_bounds__(256) void hps_files_body_kernel(const FileTab *__restrict__ tab, const Block *__restrict__ blocks,
                                                             const Row *__restrict__ rows, const Item *__restrict__ items,
                                                             const uint8_t *__restrict__ adpcm, uint8_t *__restrict__ images)
{
    const Item it = items[blockIdx.x];
    const Block B = blocks[it.block];
    const FileTab t = tab[B.w.file];
    const uint32_t padded = (uint32_t)B.w.written_size / (uint32_t)t.nch, n = (uint32_t)B.w.channel_size;
    uint8_t *body = images + t.image_off + B.w.offset + t.block_header_size;
    for (uint32_t o = it.start + threadIdx.x * 16u; o < it.end; o += 256u * 16u) {
        const uint32_t c = o / padded, within = o - c * padded;
        const uint8_t *s = adpcm + rows[t.first_channel + (int)c].adpcm_off + B.w.byte_in_index + within;
        uint4 v;
        if (within + 16 <= n) {
            v = *reinterpret_cast<const uint4 *>(s);
        } else {
            uint8_t tmp[16];
            for (int k = 0; k < 16; k++) tmp[k] = within + k < n ? s[k] : 0;
            memcpy(&v, tmp, 16);
        }
        *reinterpret_cast<uint4 *>(body + o) = v;
    }
}

// one thread per channel: the parsed coefficients, gain and contexts
__global__ __launch_bounds__(64) void hps_files_meta_kernel(const ChannelMeta *__restrict__ meta, int nch, int16_t *__restrict__ coefs,
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

__global__ __launch_bounds__(256) void hps_files_gather_kernel(const Block *__restrict__ blocks, const Row *__restrict__ rows,
                                                               const Item *__restrict__ items, const uint8_t *__restrict__ images,
                                                               uint8_t *__restrict__ adpcm)
{
    const Item it = items[blockIdx.x];
    const Block B = blocks[it.block];
    const uint8_t *s = images + B.r.src + (int64_t)B.r.stride * (it.row - B.r.first_channel);
    uint8_t *d = adpcm + rows[it.row].adpcm_off + B.r.out_offset;
    if (B.r.granule != 16) {                                   // the general form
        for (uint32_t o = it.start + threadIdx.x; o < it.end; o += 256u) d[o] = s[o];
        return;
    }
    for (uint32_t o = it.start + threadIdx.x * 16u; o < it.end; o += 256u * 16u) {
        if (o + 16 <= it.end) {
            *reinterpret_cast<uint4 *>(d + o) = *reinterpret_cast<const uint4 *>(s + o);
        } else {
            for (uint32_t k = o; k < it.end; k++) d[k] = s[k];  // the block's ragged end
        }
    }
}

// ---------------------------------------------------------------- launchers
int launch_write_images(const DeviceTables &t, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *d_gain,
                        const int16_t *d_start_context, const int16_t *d_pcm, uint8_t *d_images, hipStream_t stream, int *launches)
{
    *launches = 0;
    if (t.files <= 0) return VGA_OK;
    hipLaunchKernelGGL(hps_files_header_kernel, dim3(t.files + t.blocks_n), dim3(64), 0, stream, t.tab, t.blocks, t.files, t.rows, d_adpcm,
                       d_coefs, d_gain, d_start_context, d_pcm, d_images);
    VGA_HIP_TRY(hipGetLastError());
    ++*launches;
    if (t.items_n > 0) {
        hipLaunchKernelGGL(hps_files_body_kernel, dim3(t.items_n), dim3(256), 0, stream, t.tab, t.blocks, t.rows, t.items, d_adpcm, d_images);
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
        hipLaunchKernelGGL(hps_files_meta_kernel, dim3((t.channels + 63) / 64), dim3(64), 0, stream, t.meta, t.channels, d_coefs, d_gain,
                           d_start_context, d_loop_context);
        VGA_HIP_TRY(hipGetLastError());
        ++*launches;
    }
    if (t.items_n > 0) {
        hipLaunchKernelGGL(hps_files_gather_kernel, dim3(t.items_n), dim3(256), 0, stream, t.blocks, t.rows, t.items, d_images, d_adpcm);
        VGA_HIP_TRY(hipGetLastError());
        ++*launches;
    }
    return VGA_OK;
}

}  // namespace hpf
}  // namespace vga
