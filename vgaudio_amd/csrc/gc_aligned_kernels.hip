// gc_aligned_kernels.hip -- the kernels of include/vgaudio_hip/gc_files_aligned.h: the GcAdpcmAlignment.cs re-encode for a
// SET of files of different shapes, every kernel one launch over tables the set's object holds (gc_aligned_host.hpp).  The
// decode and encode steps in between are the ragged codec launches (gc_capi.hpp), unchanged.
//
//   gc_aligned_gather_kernel    newPcm of GcAdpcmAlignment.cs:44-51 -- the rest of the last kept-from frame, then the loop,
//                               wrapped with a modulo per sample -- into the tail batch's PCM rows, over (channel, chunk of
//                               the tail) items; the first chunk also leaves the re-encode history (:54-55) and the
//                               channel's coefficients at the tail batch's row index
//   gc_aligned_assemble_kernel  one body for AdpcmAligned (:57-59) and PcmAligned (:41-43, :61-62): an output row is `keep`
//                               bytes of the input row, then the tail batch's row; a file that needs no alignment keeps its
//                               whole row.  (channel, chunk) items cut per part, granule 16, 8 or 4 bytes per item
//   gc_aligned_meta_kernel      gc_files_meta_kernel on the aligned PCM without assembling it: sample k is the input
//                               batch's decode below samples_to_keep and the tail's above; the loop context's pred/scale
//                               byte is the ORIGINAL stream's at the aligned loop start (GcAdpcmChannelBuilder.cs:179)
// The copies are one thread per granule of the OUTPUT (coalesced stores), no LDS.
#include "common.hpp"
#include "gc_aligned_host.hpp"
#include "gc_aligned_kernels.hpp"

namespace vga {
namespace gca {

template <int G> struct Granule;
template <> struct Granule<4> { using type = uint32_t; };
template <> struct Granule<8> { using type = uint2; };
template <> struct Granule<16> { using type = uint4; };

__global__ __launch_bounds__(256) void gc_aligned_gather_kernel(const AlignRow *__restrict__ rows, const Item *__restrict__ items,
                                                                const int16_t *__restrict__ in_pcm, const int16_t *__restrict__ coefs,
                                                                int16_t *__restrict__ tail_pcm, int16_t *__restrict__ tail_coefs,
                                                                int16_t *__restrict__ hist1, int16_t *__restrict__ hist2)
{
    const Item it = items[blockIdx.x];
    const AlignRow r = rows[it.x];
    const int16_t *src = in_pcm + r.in_pcm_off;
    int16_t *dst = tail_pcm + r.tail_pcm_off;
#pragma unroll
    for (int k = 0; k < CHUNK_SAMPLES / 256; k++) {
        const int i = (int)it.y + k * 256 + (int)threadIdx.x;
        if (i >= r.samples_to_encode) break;
        dst[i] = i < r.head ? src[r.samples_to_keep + i] : src[r.loop_start + (i - r.head) % r.loop_length];
    }
    if (it.y == 0) {
        if (threadIdx.x == 0) {
            hist1[r.tail_row] = r.samples_to_keep < 1 ? (int16_t)0 : src[r.samples_to_keep - 1];
            hist2[r.tail_row] = r.samples_to_keep < 2 ? (int16_t)0 : src[r.samples_to_keep - 2];
        }
        if (threadIdx.x >= 64 && threadIdx.x < 80)
            tail_coefs[(int64_t)r.tail_row * 16 + (threadIdx.x - 64)] = coefs[(int64_t)it.x * 16 + (threadIdx.x - 64)];
    }
}

// bytes [start, end) of one output row: below `keep` from a, from `keep` on from b; [start, end) lies on one side of it
template <int G>
__device__ __forceinline__ void assemble_chunk(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, uint8_t *__restrict__ out,
                                               uint64_t keep, uint64_t start, uint64_t end)
{
    using T = typename Granule<G>::type;
    const uint8_t *s = start < keep ? a : b - keep;
#pragma unroll
    for (int k = 0; k < CHUNK_GRANULES / 256; k++) {
        const uint64_t o = start + (uint64_t)(k * 256 + (int)threadIdx.x) * G;
        if (o >= end) return;
        if (o + G <= end) {
            *reinterpret_cast<T *>(out + o) = *reinterpret_cast<const T *>(s + o);
        } else {                                           // the end of a part goes byte by byte
            for (uint64_t q = o; q < end; q++) out[q] = s[q];
        }
    }
}

template <bool PCM>
__global__ __launch_bounds__(256) void gc_aligned_assemble_kernel(const AlignRow *__restrict__ rows, const Item *__restrict__ items,
                                                                  const uint8_t *__restrict__ in, const uint8_t *__restrict__ tail,
                                                                  uint8_t *__restrict__ out)
{
    const Item it = items[blockIdx.x];
    const AlignRow r = rows[it.x];
    const uint64_t keep = PCM ? (uint64_t)r.samples_to_keep * 2 : (uint64_t)r.bytes_to_keep;
    const uint64_t total = PCM ? (uint64_t)r.out_samples * 2 : (uint64_t)r.out_bytes;
    const uint8_t *a = in + (PCM ? r.in_pcm_off * 2 : r.in_adpcm_off);
    const uint8_t *b = tail + (PCM ? r.tail_pcm_off * 2 : r.tail_adpcm_off);
    uint8_t *o = out + (PCM ? r.out_pcm_off * 2 : r.out_adpcm_off);
    const uint32_t code = it.y >> 30;
    const uint64_t start = (uint64_t)(it.y & 0x3FFFFFFFu) << 2;
    const uint64_t part_end = start < keep ? keep : total;
    const uint64_t chunk = (uint64_t)CHUNK_GRANULES * (4u << code);
    const uint64_t end = part_end - start < chunk ? part_end : start + chunk;
    if (code == 2) assemble_chunk<16>(a, b, o, keep, start, end);
    else if (code == 1) assemble_chunk<8>(a, b, o, keep, start, end);
    else assemble_chunk<4>(a, b, o, keep, start, end);
}

__global__ __launch_bounds__(256) void gc_aligned_meta_kernel(const AlignRow *__restrict__ rows, const MetaItem *__restrict__ items,
                                                              const uint8_t *__restrict__ adpcm, const int16_t *__restrict__ in_pcm,
                                                              const int16_t *__restrict__ tail_pcm, int16_t *__restrict__ seek,
                                                              int16_t *__restrict__ loop_context)
{
    const MetaItem it = items[blockIdx.x];
    const AlignRow r = rows[it.x];
    const int16_t *kept = in_pcm + r.in_pcm_off;
    const int16_t *rest = tail_pcm + r.tail_pcm_off - r.samples_to_keep;      // (never read by a file that needs no alignment)
    const int64_t keep = r.samples_to_keep;
    if (seek) {
        int16_t *t = seek + r.seek_off;
#pragma unroll
        for (int k = 0; k < CHUNK_ENTRIES / 256; k++) {
            const int i = it.y + k * 256 + (int)threadIdx.x;
            if (i >= r.entries) break;
            const int64_t at = (int64_t)i * r.spacing;                 // the first entry is always 0
            int16_t h1 = 0, h2 = 0;
            if (i != 0) {
                h1 = at - 1 < keep ? kept[at - 1] : rest[at - 1];
                if (at >= 2) h2 = at - 2 < keep ? kept[at - 2] : rest[at - 2];
            }
            *reinterpret_cast<int *>(t + 2 * i) = (int)(uint16_t)h1 | ((int)(uint16_t)h2 << 16);
        }
    }
    if (loop_context && it.y == 0 && threadIdx.x == 0) {
        int16_t *c = loop_context + (int64_t)it.x * 3;
        const int ls = r.loop_start_aligned;
        if (ls == 0) {                                                 // "current loop context is valid": the default context
            c[0] = c[1] = c[2] = 0;
        } else {                                                       // the ORIGINAL stream (GcAdpcmChannelBuilder.cs:179)
            c[0] = (int16_t)adpcm[r.in_adpcm_off + ls / 14 * 8];
            c[1] = ls < 1 ? (int16_t)0 : (ls - 1 < keep ? kept[ls - 1] : rest[ls - 1]);
            c[2] = ls < 2 ? (int16_t)0 : (ls - 2 < keep ? kept[ls - 2] : rest[ls - 2]);
        }
    }
}

// ---------------------------------------------------------------- launchers
int launch_gather(const DeviceTables &t, const int16_t *d_in_pcm, const int16_t *d_coefs, int16_t *d_tail_pcm, int16_t *d_tail_coefs,
                  int16_t *d_hist1, int16_t *d_hist2, hipStream_t stream)
{
    if (t.gather_items <= 0) return VGA_OK;
    hipLaunchKernelGGL(gc_aligned_gather_kernel, dim3(t.gather_items), dim3(256), 0, stream, t.rows, t.gather, d_in_pcm, d_coefs, d_tail_pcm,
                       d_tail_coefs, d_hist1, d_hist2);
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

int launch_assemble_adpcm(const DeviceTables &t, const uint8_t *d_adpcm, const uint8_t *d_tail_adpcm, uint8_t *d_adpcm_out, hipStream_t stream)
{
    if (t.adpcm_items <= 0) return VGA_OK;
    hipLaunchKernelGGL(gc_aligned_assemble_kernel<false>, dim3(t.adpcm_items), dim3(256), 0, stream, t.rows, t.adpcm, d_adpcm, d_tail_adpcm,
                       d_adpcm_out);
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

int launch_assemble_pcm(const DeviceTables &t, const int16_t *d_in_pcm, const int16_t *d_tail_pcm, int16_t *d_pcm_out, hipStream_t stream)
{
    if (t.pcm_items <= 0) return VGA_OK;
    hipLaunchKernelGGL(gc_aligned_assemble_kernel<true>, dim3(t.pcm_items), dim3(256), 0, stream, t.rows, t.pcm,
                       reinterpret_cast<const uint8_t *>(d_in_pcm), reinterpret_cast<const uint8_t *>(d_tail_pcm),
                       reinterpret_cast<uint8_t *>(d_pcm_out));
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

int launch_meta(const DeviceTables &t, bool all_chunks, const uint8_t *d_adpcm, const int16_t *d_in_pcm, const int16_t *d_tail_pcm,
                int16_t *d_seek, int16_t *d_loop_context, hipStream_t stream)
{
    const int blocks = all_chunks ? t.meta_items : t.channels;         // chunk 0 of every channel comes first
    if (blocks <= 0 || (!d_seek && !d_loop_context)) return VGA_OK;
    hipLaunchKernelGGL(gc_aligned_meta_kernel, dim3(blocks), dim3(256), 0, stream, t.rows, t.meta, d_adpcm, d_in_pcm, d_tail_pcm, d_seek,
                       d_loop_context);
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

}  // namespace gca
}  // namespace vga
