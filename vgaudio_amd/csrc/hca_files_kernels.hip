// hca_files_kernels.hip -- the kernels of include/vgaudio_hip/hca_files.h: the HCA images of a SET of files of different
// shapes, every kernel one launch over tables the set's object holds (hca_files_host.hpp).
//
//   hca_files_header_kernel   (write) one workgroup per file: the header built at create, out of the object's blob
//   hca_files_span_kernel     frames of up to 4096 bytes: (file, span of whole frames) items.  The span is one contiguous
//                             run of bytes on both sides, at two unrelated alignments: aligned 16-byte loads into LDS, the
//                             stored-bytes CRC (read, when counts are asked for), the substitution through the file's table
//                             and the refreshed CRC on the copy in LDS, aligned 16-byte stores out of a byte-shifted view of
//                             it; lead and tail bytes singly.  A frame is shared by 1 .. 64 lanes, about 16 .. 32 bytes each.
//   hca_files_general_kernel  every other frame size: (file, whole frames) items, a workgroup per item, 256 lanes per frame,
//                             byte by byte in global memory
// The CRC is Utilities/Crc16.cs with polynomial 0x8005, MSB first, initial value 0: every lane CRCs its own chunk through a
// 256-entry table in LDS, the chunk CRCs are moved to their place with hca_frame_crc.hpp's x^(8k) table and XOR-reduced.
// Without a key and without counts a span is a plain copy through LDS and no CRC is computed.
#include "common.hpp"
#include "hca_files_kernels.hpp"
#include "hca_frame_crc.hpp"

namespace vga {
namespace hcaf {

constexpr int kLdsBytes = SPAN_BYTES + 48;       // a lead of up to 15 bytes, the last granule's overhang, the shifted view's fifth dword

// one byte into a running CRC through the table of step(0, b)
__device__ __forceinline__ unsigned table_step(const uint16_t *crc_tab, unsigned crc, unsigned byte)
{
    return ((crc << 8) ^ crc_tab[(crc >> 8) ^ byte]) & 0xFFFFu;
}

// the table of an item's file: the object's own, or the caller's through the per-file index (KeySource), -1 = none
__device__ __forceinline__ int item_key(const KeySource &keys, int own, int file)
{
    if (!keys.external) return own;
    const int k = keys.index ? keys.index[file] : 0;
    return k >= 0 && k < keys.ntables ? k : -1;
}

__global__ __launch_bounds__(256) void hca_files_header_kernel(const FileTab *__restrict__ tab, const uint8_t *__restrict__ headers,
                                                               uint8_t *__restrict__ images)
{
    const FileTab &t = tab[blockIdx.x];
    const uint8_t *src = headers + t.header_off;                       // both on 16
    uint8_t *dst = images + t.image_off;
    const int whole = t.header_size >> 4;
    for (int g = threadIdx.x; g < whole; g += 256) reinterpret_cast<uint4 *>(dst)[g] = reinterpret_cast<const uint4 *>(src)[g];
    for (int i = 16 * whole + (int)threadIdx.x; i < t.header_size; i += 256) dst[i] = src[i];
}

// the frames of one item in place at `a` (LDS), n frames of fs bytes: counts the frames whose stored CRC does not match
// (check) into *bad, substitutes the first fs - 2 bytes and refreshes the CRC (keyed)
__device__ __forceinline__ void crypt_frames_lds(uint8_t *a0, int n, int fs, bool check, bool keyed, const uint8_t *sub,
                                                 const uint16_t *crc_tab, const uint16_t *__restrict__ crc_pow, int *bad)
{
    const int nb = fs - 2;
    int lanes = 1;                                                     // per frame: uniform over the workgroup
    while (lanes < 64 && nb >= 32 * lanes) lanes <<= 1;
    const int groups = 256 / lanes, group = (int)threadIdx.x / lanes, sl = (int)threadIdx.x % lanes;
    const int chunk = (nb + lanes - 1) / lanes;
    const int begin = min(sl * chunk, nb), end = min(begin + chunk, nb);
    for (int j0 = 0; j0 < n; j0 += groups) {
        const int j = j0 + group;
        const bool active = j < n;
        uint8_t *a = a0 + (active ? j : 0) * fs;
        unsigned was = 0, now = 0;
        if (active) {
            for (int i = begin; i < end; i++) {
                unsigned b = a[i];
                if (check) was = table_step(crc_tab, was, b);
                if (keyed) {
                    b = sub[b];
                    a[i] = (uint8_t)b;
                    now = table_step(crc_tab, now, b);
                }
            }
        }
        unsigned part = 0;                                             // stored-bytes CRC low, refreshed CRC high
        if (active && begin < end) {
            const unsigned shift = crc_pow[nb - end];
            if (check) part = hca_crc::gf_mul16(was, shift);
            if (keyed) part |= hca_crc::gf_mul16(now, shift) << 16;
        }
        for (int o = 32; o >= 1; o >>= 1)
            if (o < lanes) part ^= (unsigned)__shfl_xor((int)part, o);
        if (active && sl == 0) {
            if (check && (part & 0xFFFFu) != ((unsigned)a[nb] << 8 | a[nb + 1])) atomicAdd(bad, 1);
            if (keyed) {
                a[nb] = (uint8_t)(part >> 24);
                a[nb + 1] = (uint8_t)(part >> 16);
            }
        }
    }
}

template <bool READ>
__global__ __launch_bounds__(256) void hca_files_span_kernel(const FileTab *__restrict__ tab, const Item *__restrict__ items,
                                                             KeySource keys, const uint16_t *__restrict__ crc_pow,
                                                             const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                             int *__restrict__ bad_crc)
{
    __shared__ __align__(16) uint8_t lds[kLdsBytes];
    __shared__ uint8_t sub[256];
    __shared__ uint16_t crc_tab[256];
    __shared__ int bad;
    const int tid = threadIdx.x;
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[it.file];
    const int fs = t.frame_size, n = min(t.item_frames, t.frame_count - it.first_frame);
    const int bytes = n * fs;                                          // at most SPAN_BYTES: the form's condition
    const uint8_t *s = src + t.src_off + (int64_t)it.first_frame * fs;
    uint8_t *d = dst + t.dst_off + (int64_t)it.first_frame * fs;
    const int key = item_key(keys, t.key, it.file);
    const bool keyed = key >= 0, check = READ && bad_crc != nullptr;

    // in: the 16-byte granules that hold the span; byte i of the span is lds[lead + i]
    const int lead = (int)((uintptr_t)s & 15);
    const uint4 *s16 = reinterpret_cast<const uint4 *>(s - lead);
    const int granules = (lead + bytes + 15) >> 4;
    for (int g = tid; g < granules; g += 256) reinterpret_cast<uint4 *>(lds)[g] = s16[g];
    if (keyed || check) {
        if (keyed) sub[tid] = keys.tables[(size_t)key * 256 + tid];
        crc_tab[tid] = (uint16_t)hca_crc::step(0u, (unsigned)tid);
        if (tid == 0) bad = 0;
        __syncthreads();
        crypt_frames_lds(lds + lead, n, fs, check, keyed, sub, crc_tab, crc_pow, &bad);
        __syncthreads();
        if (check && tid == 0 && bad) atomicAdd(bad_crc + it.file, bad);
    } else {
        __syncthreads();
    }

    // out: single bytes up to the destination's grid, granules out of the view of LDS shifted by whole dwords and r bytes
    const int head = min((16 - (int)((uintptr_t)d & 15)) & 15, bytes);
    const int whole = (bytes - head) >> 4, tail_at = head + 16 * whole;
    if (tid < head) d[tid] = lds[lead + tid];
    const int q = (lead + head) >> 2, r = (lead + head) & 3;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(lds);
    for (int g = tid; g < whole; g += 256) {
        const uint32_t *p = w + 4 * g + q;
        const uint32_t w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3], w4 = p[4];
        uint4 v;
        v.x = __builtin_amdgcn_alignbyte(w1, w0, r);
        v.y = __builtin_amdgcn_alignbyte(w2, w1, r);
        v.z = __builtin_amdgcn_alignbyte(w3, w2, r);
        v.w = __builtin_amdgcn_alignbyte(w4, w3, r);
        reinterpret_cast<uint4 *>(d + head)[g] = v;
    }
    if (tid < bytes - tail_at) d[tail_at + tid] = lds[lead + tail_at + tid];
    // behind a stream's last frame: zeros up to the next multiple of 4
    if (READ && it.first_frame + n == t.frame_count) {
        const int64_t total = (int64_t)t.frame_count * fs;
        if (tid < (int)((4 - (total & 3)) & 3)) d[bytes + tid] = 0;
    }
}

template <bool READ>
__global__ __launch_bounds__(256) void hca_files_general_kernel(const FileTab *__restrict__ tab, const Item *__restrict__ items,
                                                                KeySource keys, const uint16_t *__restrict__ crc_pow,
                                                                const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                                int *__restrict__ bad_crc)
{
    __shared__ uint8_t sub[256];
    __shared__ uint16_t crc_tab[256];
    __shared__ unsigned acc;
    const int tid = threadIdx.x;
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[it.file];
    const int fs = t.frame_size, n = min(t.item_frames, t.frame_count - it.first_frame);
    const uint8_t *s = src + t.src_off + (int64_t)it.first_frame * fs;
    uint8_t *d = dst + t.dst_off + (int64_t)it.first_frame * fs;
    const int key = item_key(keys, t.key, it.file);
    const bool keyed = key >= 0, check = READ && bad_crc != nullptr;
    const int64_t bytes = (int64_t)n * fs;
    if (!keyed && !check) {
        for (int64_t i = tid; i < bytes; i += 256) d[i] = s[i];
    } else {
        if (keyed) sub[tid] = keys.tables[(size_t)key * 256 + tid];
        crc_tab[tid] = (uint16_t)hca_crc::step(0u, (unsigned)tid);
        const int nb = fs - 2, chunk = (nb + 255) / 256;
        const int begin = min(tid * chunk, nb), end = min(begin + chunk, nb);
        int bad = 0;                                                   // (thread 0's)
        for (int j = 0; j < n; j++) {
            const uint8_t *a = s + (int64_t)j * fs;
            uint8_t *o = d + (int64_t)j * fs;
            if (tid == 0) acc = 0;
            __syncthreads();                                           // (the first trip: the tables as well)
            unsigned was = 0, now = 0;
            for (int i = begin; i < end; i++) {
                unsigned b = a[i];
                if (check) was = table_step(crc_tab, was, b);
                if (keyed) {
                    b = sub[b];
                    now = table_step(crc_tab, now, b);
                }
                o[i] = (uint8_t)b;
            }
            if (begin < end) {
                const unsigned shift = crc_pow[nb - end];
                unsigned part = 0;
                if (check) part = hca_crc::gf_mul16(was, shift);
                if (keyed) part |= hca_crc::gf_mul16(now, shift) << 16;
                atomicXor(&acc, part);
            }
            __syncthreads();
            if (tid == 0) {
                const unsigned part = acc, stored = (unsigned)a[nb] << 8 | a[nb + 1];
                if (check && (part & 0xFFFFu) != stored) bad++;
                const unsigned crc = keyed ? part >> 16 : stored;
                o[nb] = (uint8_t)(crc >> 8);
                o[nb + 1] = (uint8_t)crc;
            }
        }
        if (tid == 0 && bad) atomicAdd(bad_crc + it.file, bad);
    }
    if (READ && it.first_frame + n == t.frame_count) {
        const int64_t total = (int64_t)t.frame_count * fs;
        if (tid < (int)((4 - (total & 3)) & 3)) d[bytes + tid] = 0;
    }
}

// ---------------------------------------------------------------- launchers
template <bool READ>
static int launch_items(const DeviceTables &t, bool general, const uint8_t *src, uint8_t *dst, int *d_bad_crc, hipStream_t stream, KeySource keys)
{
    if (!keys.external) keys.tables = t.tables;
    const int k = general ? 1 : 0, span = general ? 0 : t.span_items, rest = t.item_count[k] - span;
    if (span > 0) {
        hipLaunchKernelGGL(hca_files_span_kernel<READ>, dim3(span), dim3(256), 0, stream, t.tab, t.items[k], keys, t.crc_pow, src, dst, d_bad_crc);
        VGA_HIP_TRY(hipGetLastError());
    }
    if (rest > 0) {
        hipLaunchKernelGGL(hca_files_general_kernel<READ>, dim3(rest), dim3(256), 0, stream, t.tab, t.items[k] + span, keys, t.crc_pow, src, dst,
                           d_bad_crc);
        VGA_HIP_TRY(hipGetLastError());
    }
    return VGA_OK;
}

int launch_write_images(const DeviceTables &t, bool general, const uint8_t *d_frames, uint8_t *d_images, hipStream_t stream)
{
    if (t.files <= 0) return VGA_OK;
    hipLaunchKernelGGL(hca_files_header_kernel, dim3(t.files), dim3(256), 0, stream, t.tab, t.headers, d_images);
    VGA_HIP_TRY(hipGetLastError());
    return launch_items<false>(t, general, d_frames, d_images, nullptr, stream, KeySource());
}

int launch_read_images(const DeviceTables &t, bool general, const uint8_t *d_images, uint8_t *d_frames, int *d_bad_crc, hipStream_t stream,
                       const KeySource &keys)
{
    if (t.files <= 0) return VGA_OK;
    return launch_items<true>(t, general, d_images, d_frames, d_bad_crc, stream, keys);
}

}  // namespace hcaf
}  // namespace vga
