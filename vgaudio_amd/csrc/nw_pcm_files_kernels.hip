// nw_pcm_files_kernels.hip -- the kernels of include/vgaudio_hip_files/nw_pcm_files.h: the BRSTM / BCSTM / BFSTM images of a SET
// of PCM16 / PCM8 files of different shapes written from planar int16 rows and taken apart into them, every kernel one launch
// over tables the set's object holds (nw_pcm_files_host.hpp).
//
//   nw_pcm_files_header_kernel          the file header, HEAD / INFO and the DATA header of every file: nw_header_body.hpp's body
//                                       (its PCM branches), one workgroup per file, the default track list computed in place
//   nw_pcm_files_write_vector_kernel    Interleave(rows, InterleaveSize, AudioDataSize) fused with the sample conversion over
//   nw_pcm_files_read_vector_kernel     (file, chunk) items, and DeInterleave over (row, chunk) items: one 16-byte granule of the
//                                       FILE side per thread, aligned 16-byte vector accesses on both sides, whole dwords
//                                       converted with v_perm_b32 (pcm_kernels.hip says why); the zero fill comes from the same
//                                       threads; a granule a row supplies in part, or that crosses a row's end, goes singly
//   nw_pcm_files_write_general_kernel   the same addressing one sample per thread, byte accesses on the file side: files whose
//   nw_pcm_files_read_general_kernel    interleave, offsets or row offsets do not allow the granules
// Everything is a converting copy: every byte read and written once, no LDS.  Offsets inside an image are 32-bit (FileSize
// is an int), image and row bases int64_t.
#include "common.hpp"
#include "nw_pcm_files_kernels.hpp"
#include "nw_header_body.hpp"

namespace vga {
namespace nwpf {

constexpr uint32_t kSelSwap16 = 0x02030001u;     // v_perm_b32: the two bytes of every short swapped
constexpr uint32_t kSelHigh = 0x07050301u;       // the high bytes of four shorts held by two dwords (s >> 8)
constexpr uint32_t kSelWidenLo = 0x010c000cu, kSelWidenHi = 0x030c020cu;   // bytes 0, 1 / 2, 3 of a dword as (short)(b << 8)

// a PCM stream has no per-channel arrays: the header body asks for none of them
struct DefaultTracks {
    int nch;
    __device__ int row(int) const { return 0; }
    __device__ int first_byte(int) const { return 0; }
    __device__ nw::TrackK track(int i) const { return nw::default_track(nch, i); }
};

__global__ __launch_bounds__(64) void nw_pcm_files_header_kernel(const FileTab *__restrict__ tab, uint8_t *__restrict__ images)
{
    const FileTab &t = tab[blockIdx.x];
    nw::write_header(t.h, DefaultTracks{t.h.nch}, nullptr, nullptr, nullptr, nullptr, images + t.image_off);
}

// Where byte o of a file's audio region comes from (Interleave.cs:43-78, gc_files_chunks.hpp's arithmetic): channel i, its
// stored byte q0, and how many bytes from there on the row supplies inside this (block, channel) segment (<= 0: zeros)
struct Source { uint32_t i, q0; int avail; };
__device__ __forceinline__ Source locate(const FileTab &t, uint32_t o)
{
    const uint32_t il = t.interleave, in = t.input_size, out = t.output_size;
    const uint32_t in_blocks = (in + il - 1) / il, out_blocks = (out + il - 1) / il;
    const uint32_t stride = il * (uint32_t)t.nch;           // the host holds il <= out: below 2^31
    uint32_t b = o / stride;
    if (b > out_blocks - 1) b = out_blocks - 1;             // the (short) last block's rows are packed more tightly
    const uint32_t r = o - b * stride;
    const uint32_t cur_out = b == out_blocks - 1 ? out - (out_blocks - 1) * il : il;
    const uint32_t i = r / cur_out, within = r - i * cur_out;
    uint32_t n = 0;
    if (b < in_blocks) {
        const uint32_t cur_in = b == in_blocks - 1 ? in - (in_blocks - 1) * il : il;
        n = cur_in < cur_out ? cur_in : cur_out;
    }
    return {i, il * b + within, (int)n - (int)within};
}

// stored byte q of a channel from its int16 row
__device__ __forceinline__ uint32_t stored_byte(int conv, const int16_t *__restrict__ row, uint32_t q)
{
    if (conv == kPcm8) return (uint8_t)(row[q] >> 8);
    return reinterpret_cast<const uint8_t *>(row)[conv == kSwap16 ? q ^ 1u : q];
}

__global__ __launch_bounds__(256) void nw_pcm_files_write_vector_kernel(const FileTab *__restrict__ tab, const int64_t *__restrict__ row_off,
                                                                        const Item *__restrict__ items, const int16_t *__restrict__ pcm,
                                                                        uint8_t *__restrict__ images)
{
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[it.x];
    const int conv = t.conv;
    const uint32_t total = t.output_size * (uint32_t)t.nch, start = it.y * (uint32_t)CHUNK_BYTES;
    const uint32_t end = total - start < (uint32_t)CHUNK_BYTES ? total : start + CHUNK_BYTES;
    uint8_t *audio = images + t.audio_at;
#pragma unroll
    for (int k = 0; k < CHUNK_GRANULES / 256; k++) {
        const uint32_t o = start + (uint32_t)(k * 256 + (int)threadIdx.x) * GRANULE_BYTES;
        if (o >= end) return;
        const Source s = locate(t, o);
        const int16_t *row = pcm + row_off[t.first_channel + (int)s.i];
        uint4 v = {0u, 0u, 0u, 0u};
        if (s.avail >= GRANULE_BYTES) {
            if (conv == kPcm8) {
                const uint4 a = *reinterpret_cast<const uint4 *>(row + s.q0), b = *reinterpret_cast<const uint4 *>(row + s.q0 + 8);
                v.x = __builtin_amdgcn_perm(a.y, a.x, kSelHigh);
                v.y = __builtin_amdgcn_perm(a.w, a.z, kSelHigh);
                v.z = __builtin_amdgcn_perm(b.y, b.x, kSelHigh);
                v.w = __builtin_amdgcn_perm(b.w, b.z, kSelHigh);
            } else {
                v = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(row) + s.q0);
                if (conv == kSwap16) {
                    v.x = __builtin_amdgcn_perm(0u, v.x, kSelSwap16);
                    v.y = __builtin_amdgcn_perm(0u, v.y, kSelSwap16);
                    v.z = __builtin_amdgcn_perm(0u, v.z, kSelSwap16);
                    v.w = __builtin_amdgcn_perm(0u, v.w, kSelSwap16);
                }
            }
        } else if (s.avail > 0) {                           // the end of what the row supplies: nothing behind it is read
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int q = 0; q < GRANULE_BYTES; q++)
                if (q < s.avail) w[q >> 2] |= stored_byte(conv, row, s.q0 + q) << (8 * (q & 3));
            v = {w[0], w[1], w[2], w[3]};
        }
        *reinterpret_cast<uint4 *>(audio + o) = v;          // total is a multiple of 0x20: a granule never passes the region's end
    }
}

__global__ __launch_bounds__(256) void nw_pcm_files_write_general_kernel(const FileTab *__restrict__ tab, const int64_t *__restrict__ row_off,
                                                                         const Item *__restrict__ items, const int16_t *__restrict__ pcm,
                                                                         uint8_t *__restrict__ images)
{
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[it.x];
    const int conv = t.conv;
    const uint32_t bps = (uint32_t)t.bps;
    const uint32_t total = t.output_size * (uint32_t)t.nch, start = it.y * (uint32_t)CHUNK_BYTES;
    const uint32_t end = total - start < (uint32_t)CHUNK_BYTES ? total : start + CHUNK_BYTES;
    uint8_t *audio = images + t.audio_at;
    // one stored sample per thread and trip; PCM16 segments are even, so a sample never straddles two
    for (uint32_t o = start + threadIdx.x * bps; o < end; o += 256 * bps) {
        const Source s = locate(t, o);
        int v = 0;
        if (s.avail > 0) v = pcm[row_off[t.first_channel + (int)s.i] + (s.q0 >> (bps - 1))];
        if (bps == 1) {
            audio[o] = (uint8_t)(v >> 8);
        } else {
            audio[o] = (uint8_t)(conv == kSwap16 ? v >> 8 : v);
            audio[o + 1] = (uint8_t)(conv == kSwap16 ? v : v >> 8);
        }
    }
}

// Where stored byte `off` of a row lies in its image (Interleave.cs:118-167, gc_files_chunks.hpp's arithmetic): the segment
// of its block and channel, the offset inside it and the segment's bytes the row takes (0: zeros)
struct Segment { const uint8_t *seg; uint32_t within, n; };
__device__ __forceinline__ Segment locate_row(const FileTab &t, const uint8_t *__restrict__ audio, int o_ch, uint32_t off)
{
    const uint32_t il = t.interleave, in = t.input_size, out = t.output_size;
    const uint32_t in_blocks = (in + il - 1) / il, out_blocks = (out + il - 1) / il;
    const uint32_t to_copy = in_blocks < out_blocks ? in_blocks : out_blocks;
    const uint32_t b = off / il, within = off - b * il;
    uint32_t n = 0, cur_in = il;
    if (b < to_copy) {
        cur_in = b == in_blocks - 1 ? in - (in_blocks - 1) * il : il;
        const uint32_t cur_out = b == out_blocks - 1 ? out - (out_blocks - 1) * il : il;
        n = cur_in < cur_out ? cur_in : cur_out;
    }
    return {audio + (uint64_t)il * b * (uint32_t)t.nch + (uint64_t)cur_in * (uint32_t)o_ch, within, n};
}

// the sample at stored byte `within` of a segment (PCM16: an even offset)
__device__ __forceinline__ int16_t stored_sample(int conv, const uint8_t *__restrict__ seg, uint32_t within)
{
    if (conv == kPcm8) return (int16_t)(seg[within] << 8);
    const uint32_t a = seg[within], b = seg[within + 1];
    return (int16_t)(conv == kSwap16 ? a << 8 | b : b << 8 | a);
}

__global__ __launch_bounds__(256) void nw_pcm_files_read_vector_kernel(const FileTab *__restrict__ tab, const int64_t *__restrict__ row_off,
                                                                       const int *__restrict__ row_file, const Item *__restrict__ items,
                                                                       const uint8_t *__restrict__ images, int16_t *__restrict__ pcm)
{
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[row_file[it.x]];
    const int conv = t.conv;
    const uint32_t out = t.output_size, start = it.y * (uint32_t)CHUNK_BYTES;
    const uint32_t end = out - start < (uint32_t)CHUNK_BYTES ? out : start + CHUNK_BYTES;
    const uint8_t *audio = images + t.audio_at;
    int16_t *row = pcm + row_off[it.x];
#pragma unroll
    for (int k = 0; k < CHUNK_GRANULES / 256; k++) {
        const uint32_t off = start + (uint32_t)(k * 256 + (int)threadIdx.x) * GRANULE_BYTES;
        if (off >= end) return;
        const Segment s = locate_row(t, audio, it.x - t.first_channel, off);
        if (s.within + GRANULE_BYTES <= s.n && off + GRANULE_BYTES <= out) {
            const uint4 v = *reinterpret_cast<const uint4 *>(s.seg + s.within);
            if (conv == kPcm8) {
                uint4 *d = reinterpret_cast<uint4 *>(row + off);
                d[0] = {__builtin_amdgcn_perm(0u, v.x, kSelWidenLo), __builtin_amdgcn_perm(0u, v.x, kSelWidenHi),
                        __builtin_amdgcn_perm(0u, v.y, kSelWidenLo), __builtin_amdgcn_perm(0u, v.y, kSelWidenHi)};
                d[1] = {__builtin_amdgcn_perm(0u, v.z, kSelWidenLo), __builtin_amdgcn_perm(0u, v.z, kSelWidenHi),
                        __builtin_amdgcn_perm(0u, v.w, kSelWidenLo), __builtin_amdgcn_perm(0u, v.w, kSelWidenHi)};
            } else {
                uint4 w = v;
                if (conv == kSwap16) {
                    w.x = __builtin_amdgcn_perm(0u, v.x, kSelSwap16);
                    w.y = __builtin_amdgcn_perm(0u, v.y, kSelSwap16);
                    w.z = __builtin_amdgcn_perm(0u, v.z, kSelSwap16);
                    w.w = __builtin_amdgcn_perm(0u, v.w, kSelSwap16);
                }
                *reinterpret_cast<uint4 *>(reinterpret_cast<uint8_t *>(row) + off) = w;
            }
            continue;
        }
        // the end of a segment or of the row: sample by sample, nothing behind the row's end is written
        const uint32_t bps = (uint32_t)t.bps;
        for (uint32_t q = 0; q < (uint32_t)GRANULE_BYTES && off + q < out; q += bps)
            row[(off + q) >> (bps - 1)] = s.within + q < s.n ? stored_sample(conv, s.seg, s.within + q) : (int16_t)0;
    }
}

__global__ __launch_bounds__(256) void nw_pcm_files_read_general_kernel(const FileTab *__restrict__ tab, const int64_t *__restrict__ row_off,
                                                                        const int *__restrict__ row_file, const Item *__restrict__ items,
                                                                        const uint8_t *__restrict__ images, int16_t *__restrict__ pcm)
{
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[row_file[it.x]];
    const int conv = t.conv;
    const uint32_t bps = (uint32_t)t.bps;
    const uint32_t out = t.output_size, start = it.y * (uint32_t)CHUNK_BYTES;
    const uint32_t end = out - start < (uint32_t)CHUNK_BYTES ? out : start + CHUNK_BYTES;
    const uint8_t *audio = images + t.audio_at;
    int16_t *row = pcm + row_off[it.x];
    for (uint32_t off = start + threadIdx.x * bps; off < end; off += 256 * bps) {
        const Segment s = locate_row(t, audio, it.x - t.first_channel, off);
        row[off >> (bps - 1)] = s.within < s.n ? stored_sample(conv, s.seg, s.within) : (int16_t)0;
    }
}

// ---------------------------------------------------------------- launchers
int launch_write_images(const DeviceTables &t, bool general, const int16_t *d_pcm, uint8_t *d_images, hipStream_t stream)
{
    if (t.files <= 0) return VGA_OK;
    const int k = general ? 1 : 0, vec = general ? 0 : t.vector_items, rest = t.item_count[k] - vec;
    hipLaunchKernelGGL(nw_pcm_files_header_kernel, dim3(t.files), dim3(64), 0, stream, t.tab, d_images);
    VGA_HIP_TRY(hipGetLastError());
    if (vec > 0) {
        hipLaunchKernelGGL(nw_pcm_files_write_vector_kernel, dim3(vec), dim3(256), 0, stream, t.tab, t.row_off, t.items[k], d_pcm, d_images);
        VGA_HIP_TRY(hipGetLastError());
    }
    if (rest > 0) {
        hipLaunchKernelGGL(nw_pcm_files_write_general_kernel, dim3(rest), dim3(256), 0, stream, t.tab, t.row_off, t.items[k] + vec, d_pcm, d_images);
        VGA_HIP_TRY(hipGetLastError());
    }
    return VGA_OK;
}

int launch_read_images(const DeviceTables &t, bool general, const uint8_t *d_images, int16_t *d_pcm, hipStream_t stream)
{
    if (t.files <= 0) return VGA_OK;
    const int k = general ? 1 : 0, vec = general ? 0 : t.vector_items, rest = t.item_count[k] - vec;
    if (vec > 0) {
        hipLaunchKernelGGL(nw_pcm_files_read_vector_kernel, dim3(vec), dim3(256), 0, stream, t.tab, t.row_off, t.row_file, t.items[k], d_images, d_pcm);
        VGA_HIP_TRY(hipGetLastError());
    }
    if (rest > 0) {
        hipLaunchKernelGGL(nw_pcm_files_read_general_kernel, dim3(rest), dim3(256), 0, stream, t.tab, t.row_off, t.row_file, t.items[k] + vec, d_images,
                           d_pcm);
        VGA_HIP_TRY(hipGetLastError());
    }
    return VGA_OK;
}

}  // namespace nwpf
}  // namespace vga
