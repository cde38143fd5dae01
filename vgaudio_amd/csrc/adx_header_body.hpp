// adx_header_body.hpp -- AdxWriter.WriteHeader (:81-117) and the footer (:133-138) as device functions: one body for the
// per-file kernels (container_kernels.hip) and the kernels of a set of files (adx_files_kernels.hip).  One thread runs them.
#pragma once
#include "adx_file_host.hpp"

namespace vga {
namespace container {

// A positioned big-endian writer over the image, as the reference's BinaryWriter over MemoryStream(byte[FileSize]).
struct AdxCursor {
    uint8_t *buf;
    int size, pos;
    __device__ void put8(int v) { if (pos < size) buf[pos] = (uint8_t)v; pos++; }
    __device__ void put16(int v) { put8(v >> 8); put8(v); }
    __device__ void put32(int v) { put16(v >> 16); put16(v); }
};

// Fields are written one after the other whatever HeaderSize is; "(c)CRI" and then the audio overwrite what ran past it --
// the later launches on the same stream reproduce that order.  history: the file's channels'.
__device__ inline void adx_write_header(const AdxHeaderArgs &a, const int16_t *__restrict__ history, uint8_t *__restrict__ file)
{
    AdxCursor c{file, a.file_size, 0};
    c.put16(0x8000);
    c.put16(a.header_size);
    c.put8(a.type);
    c.put8(a.frame_size);
    c.put8(4);                                             // bit depth
    c.put8(a.nch);
    c.put32(a.sample_rate);
    c.put32(a.sample_count);
    c.put16(a.type != 2 ? a.highpass_frequency : 0);       // CriAdxType.Fixed
    c.put8(a.version);
    c.put8(a.encryption_type);
    if (a.version == 4) {
        c.put32(0);
        for (int i = 0; i < a.nch; i++) { c.put16(history[i]); c.put16(history[i]); }
        if (a.nch == 1) c.put32(0);
    }
    c.put16(a.alignment_samples);
    c.put16(a.looping ? 1 : 0);
    c.put32(a.looping ? 1 : 0);
    c.put32(a.loop_start);
    c.put32(a.loop_start_offset);
    c.put32(a.loop_end);
    c.put32(a.loop_end_offset);
    c.pos = a.header_size - 2;
    const char sig[6] = {'(', 'c', ')', 'C', 'R', 'I'};
    for (int k = 0; k < 6; k++) c.put8(sig[k]);
}

__device__ inline void adx_write_footer(const AdxHeaderArgs &a, uint8_t *__restrict__ file)
{
    AdxCursor c{file, a.file_size, a.footer_pos};
    c.put16(0x8001);
    c.put16(a.footer_size - 4);
}

}  // namespace container
}  // namespace vga
