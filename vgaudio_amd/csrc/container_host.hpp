// container_host.hpp -- the host layer of the container files (nwstm.hip, nwwav.hip, gc_containers.hip,
// container_readers.hip, capi_containers.hip): byte readers (byte_reader.hpp) and writers over files in host memory, the reference's small helpers, the batch
// argument checks, the granule choice of the batched (de-)interleaves, and the staging of the host-pointer forms.
// Host code only; the kernels stay in container_kernels.hpp / pcm_kernels.hpp.
#pragma once
#include "common.hpp"
#include "container_kernels.hpp"
#include "byte_reader.hpp"
#include "container_math.hpp"
#include "../../include/vgaudio_hip_pcm.h"

#include <algorithm>
#include <cstring>
#include <deque>

namespace vga {
namespace container {

// Big- or little-endian writes into `size` bytes of host memory; what does not fit sets `overflow` and is dropped.
struct ByteWriter {
    uint8_t *buf;
    int64_t size, pos = 0;
    bool big = false, overflow = false;
    void put8(int v) { if (pos < size) buf[pos] = (uint8_t)v; else overflow = true; pos++; }
    void put16(int v) { if (big) { put8(v >> 8); put8(v); } else { put8(v); put8(v >> 8); } }
    void put32(int v) { if (big) { put16(v >> 16); put16(v); } else { put16(v); put16(v >> 16); } }
    void bytes(const void *src, int n) { for (int i = 0; i < n; i++) put8(static_cast<const uint8_t *>(src)[i]); }
    void tag(const char *t) { bytes(t, 4); }
};

// A _write_device call's images: at least the file size apart (a multiple of 16 when there are several), and few
// enough of them for the launches' 32-bit byte offsets.
inline int check_write_files(int nfiles, int nch, int64_t file_pitch, int file_size)
{
    if (file_pitch < file_size || (nfiles > 1 && (file_pitch & 15))) {
        set_error("file pitch %lld: at least the file size %d and a multiple of 16", (long long)file_pitch, file_size);
        return VGA_ERR_ARGUMENT;
    }
    if ((int64_t)nfiles * nch > 0x7FFFFFFF / 16) { set_error("too many files in one call"); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

// A _read_device call's rows (`row` elements of each at least, `pitch` elements apart) and images (at least `image`
// bytes apart when there are several).
inline int check_read_batch(const void *d_files, const void *d_rows, int64_t pitch, int64_t row, int nfiles, int64_t file_pitch,
                            int64_t image)
{
    if (!d_files || !d_rows || pitch < row) { set_error("null pointer / pitch < %lld", (long long)row); return VGA_ERR_ARGUMENT; }
    if (nfiles > 1 && file_pitch < image) { set_error("file pitch smaller than the file"); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

// DeInterleave (Interleave.cs:118-167) of nfiles images, each channel's `in` bytes in blocks of `il` from audio_offset
// on, into rows of `out` bytes; picks the widest granule G that divides every address and pitch.  One channel's single
// block is a plain copy, so the block sizes enter only when there are several channels or blocks.  The last block
// starts at last_in * channel in every row: it enters when it holds a granule, and is otherwise free to be shorter,
// since deinterleave_kernel moves a whole granule only where within + G <= n, and n <= last_in there.
inline int deinterleave_images(const uint8_t *d_files, int64_t file_pitch, int nfiles, int audio_offset, int nch, uint32_t in,
                               uint32_t il, uint32_t out, uint8_t *d_dst, int64_t dst_pitch, hipStream_t s)
{
    const uint32_t in_blocks = in ? (in + il - 1) / il : 0, last_in = in ? in - (in_blocks - 1) * il : 0;
    const bool several = nch > 1 || in_blocks > 1;
    const uint64_t base = (uint64_t)(uintptr_t)d_files | (uint64_t)(nfiles > 1 ? file_pitch : 0) | (uint64_t)(uint32_t)audio_offset |
                          (several ? (uint64_t)il : 0) | (uint64_t)(uintptr_t)d_dst | (uint64_t)dst_pitch;
    uint64_t align = 1;
    for (uint32_t g = 16; g > 1; g >>= 1)
        if (!(base & (g - 1)) && (!several || last_in % g == 0 || last_in < g)) { align = base | g; break; }
    return launch_deinterleave(align, d_files, file_pitch, audio_offset, nch, nfiles * nch, in, il, out, d_dst, dst_pitch, s);
}

// Interleave (Interleave.cs:43-78) of rows of `in` bytes (`pitch` apart, file f's channel c in row f * nch + c) into
// `out` bytes per channel at d_dst of each of nfiles images: G divides the rows, the interleave, the last block and
// where the region starts in every image.
inline int interleave_images(const uint8_t *d_src, int64_t pitch, int nch, int nfiles, uint32_t in, uint32_t il, uint32_t out,
                             uint8_t *d_dst, int64_t file_pitch, hipStream_t s)
{
    if (out == 0) return VGA_OK;
    const uint32_t out_blocks = (out + il - 1) / il, last_out = out - (out_blocks - 1) * il;
    const uint64_t align = (uint64_t)(uintptr_t)d_src | (uint64_t)pitch | il | last_out | (uint64_t)(uintptr_t)d_dst |
                           (uint64_t)(nfiles > 1 ? file_pitch : 0);
    return launch_interleave_files(align, d_src, pitch, nch, nfiles, in, il, out, d_dst, file_pitch, s);
}

// The host-pointer forms: the caller's data goes up on a stream of its own, the _device form runs there, the results
// come back, and finish() synchronises once.  Staged rows are the row length rounded up to 16 ELEMENTS apart, whatever
// the element size: the int16 rows of the PCM8 kernels are aligned by their pitch in elements.
class HostStage {
public:
    int open()
    {
        if (int rc = require_device()) return rc;
        VGA_HIP_TRY(st_.create());
        return VGA_OK;
    }
    hipStream_t stream() const { return st_.s; }

    // device memory of `bytes` bytes, freed with the stage
    int alloc(size_t bytes, void **d)
    {
        bufs_.emplace_back();
        VGA_HIP_TRY(bufs_.back().alloc(bytes));
        *d = bufs_.back().p;
        return VGA_OK;
    }
    // nrows host rows of n elements of `elem` bytes -> device rows *pitch elements apart; nothing is copied for n <= 0
    // or a null row list (rows for the device to fill)
    int rows(const void *const *src, int nrows, int n, int elem, void **d, int64_t *pitch)
    {
        *pitch = round_up(std::max(n, 1), 16);
        if (int rc = alloc((size_t)nrows * *pitch * elem, d)) return rc;
        for (int r = 0; src && r < nrows && n > 0; r++)
            VGA_HIP_TRY(hipMemcpyAsync(static_cast<uint8_t *>(*d) + r * *pitch * elem, src[r], (size_t)n * elem, hipMemcpyHostToDevice,
                                       st_.s));
        return VGA_OK;
    }
    template <class T> int rows(const T *const *src, int nrows, int n, T **d, int64_t *pitch)
    {
        void *p = nullptr;
        const int rc = rows(reinterpret_cast<const void *const *>(src), nrows, n, (int)sizeof(T), &p, pitch);
        *d = static_cast<T *>(p);
        return rc;
    }
    // `bytes` of a file (or of a region of it)
    int image(const uint8_t *src, size_t bytes, const uint8_t **d)
    {
        void *p = nullptr;
        if (int rc = alloc(bytes, &p)) return rc;
        if (bytes) VGA_HIP_TRY(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, st_.s));
        *d = static_cast<const uint8_t *>(p);
        return VGA_OK;
    }
    // a small int16 table (coefficients, gains, contexts, histories) of n entries; a null table stays null
    int table(const int16_t *src, size_t n, const int16_t **d)
    {
        *d = nullptr;
        if (!src) return VGA_OK;
        void *p = nullptr;
        if (int rc = alloc(n * 2, &p)) return rc;
        VGA_HIP_TRY(hipMemcpyAsync(p, src, n * 2, hipMemcpyHostToDevice, st_.s));
        *d = static_cast<const int16_t *>(p);
        return VGA_OK;
    }

    // device rows `pitch` elements apart -> nrows host rows of n elements of `elem` bytes
    int rows_back(void *const *dst, int nrows, int n, int elem, const void *d, int64_t pitch)
    {
        for (int r = 0; r < nrows; r++)
            VGA_HIP_TRY(hipMemcpyAsync(dst[r], static_cast<const uint8_t *>(d) + r * pitch * elem, (size_t)n * elem, hipMemcpyDeviceToHost,
                                       st_.s));
        return VGA_OK;
    }
    template <class T> int rows_back(T *const *dst, int nrows, int n, const T *d, int64_t pitch)
    {
        return rows_back(reinterpret_cast<void *const *>(dst), nrows, n, (int)sizeof(T), d, pitch);
    }
    int back(void *dst, const void *d, size_t bytes)
    {
        VGA_HIP_TRY(hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, st_.s));
        return VGA_OK;
    }
    int finish()
    {
        VGA_HIP_TRY(hipStreamSynchronize(st_.s));
        return VGA_OK;
    }

    // The writers' host forms, after the rows and tables are up: room for the `bytes` of the image, run(d_file, stream)
    // -- the _device form -- writes it, and it comes back to out.
    template <class F>
    int write_image(uint8_t *out, size_t bytes, F &&run)
    {
        void *d_file = nullptr;
        if (int rc = alloc(bytes, &d_file)) return rc;
        if (int rc = run(static_cast<uint8_t *>(d_file), st_.s)) return rc;
        if (int rc = back(out, d_file, bytes)) return rc;
        return finish();
    }
    // The readers' host forms:`bytes` of the file go up, run(d_file, d_rows, pitch, stream) -- the _device form --
    // fills nrows rows of n elements of `elem` bytes, and they come back to out[0 .. nrows).
    template <class T, class F>
    int read_rows(const uint8_t *file, size_t bytes, T *const *out, int nrows, int n, int elem, F &&run)
    {
        const uint8_t *d_file = nullptr;
        void *d_rows = nullptr;
        int64_t pitch = 0;
        if (int rc = open()) return rc;
        if (int rc = image(file, bytes, &d_file)) return rc;
        if (int rc = rows(nullptr, nrows, n, elem, &d_rows, &pitch)) return rc;
        if (int rc = run(d_file, d_rows, pitch, st_.s)) return rc;
        if (int rc = rows_back(reinterpret_cast<void *const *>(out), nrows, n, elem, d_rows, pitch)) return rc;
        return finish();
    }

private:
    Stream st_;
    std::deque<DevBuf> bufs_;                               // destroyed before the stream
};

}  // namespace container
}  // namespace vga
