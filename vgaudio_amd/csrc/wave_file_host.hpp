// wave_file_host.hpp -- the host side of ONE WAVE file without HIP: WaveWriter's size and header math (vga_wave_file_size's,
// vga_wave_pcm8_file_size's and the _write_ calls' code) and what the readers check of a parsed vga_wave_info before they
// touch the data chunk (vga_wave_read_pcm16's and vga_wave_read_pcm8's code).  It exists once: capi_containers.hip calls it
// for the per-file calls, wave_files_host.hpp for every file of a set (include/vgaudio_hip_files/wave_files.h), which is why a
// set refuses a file with the per-file call's own code and message.  Header-only and free of <hip/hip_runtime.h>, so that a
// stand-alone host program can include it (tests/host/wave_files_host_driver.cpp); whoever includes it supplies
// vga::set_error.
#pragma once
#include "container_math.hpp"

#include <cstring>

namespace vga {
namespace container {

// KSDATAFORMAT_SUBTYPE_PCM (WaveFormatExtensible.cs)
constexpr uint8_t kWaveSubtypePcm[16] = {0x01, 0x00, 0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71};
constexpr int kWaveMaxHeader = 144;                         // 12 + 8 + 40 + 8 + 0x3c + 8 = 136, rounded up to 16

inline int wave_channel_mask(int n)                         // WaveWriter.cs:147-164
{
    switch (n) {
    case 4: return 0x0033;
    case 5: return 0x0133;
    case 6: return 0x0633;
    case 7: return 0x01f3;
    case 8: return 0x06f3;
    default: return (int)((1u << (n & 31)) - 1);
    }
}

inline int wave_header_size(const vga_wave_params *p, int nch) { return 12 + 8 + (nch > 2 ? 40 : 16) + (p->looping ? 8 + 0x3c : 0) + 8; }

// WaveWriter.FileSize (WaveWriter.cs:25-30) for samples of 2 bytes or 1 (DataChunkSize = nch * samples * bytes, odd sizes
// included); < 0 = error
inline int64_t wave_file_size(const vga_wave_params *p, int nch, int bytes_per_sample)
{
    if (!p || nch < 1 || nch > 0x7FFF || p->sample_count < 0) { set_error("bad WAVE parameters"); return VGA_ERR_ARGUMENT; }
    const int64_t size = wave_header_size(p, nch) + (int64_t)nch * p->sample_count * bytes_per_sample;
    if (size > 0x7FFFFFFF) { set_error("WAVE file would exceed 2 GiB (FileSize is an int)"); return VGA_ERR_OUT_OF_RANGE; }
    return size;
}

// WriteRiffHeader / WriteFmtChunk / WriteSmplChunk / the data chunk's header (WaveWriter.cs:56-129) into
// wave_header_size(p, nch) bytes; every chunk size here is even, so the reference's 2-byte alignment steps never move the
// position
inline void wave_header(const vga_wave_params *p, int nch, int64_t file_size, uint8_t *out, int bytes_per_sample = 2)
{
    const int bps = bytes_per_sample;
    uint8_t *at = out;
    auto put16 = [&](int v) { *at++ = (uint8_t)v; *at++ = (uint8_t)(v >> 8); };
    auto put32 = [&](int v) { put16(v); put16(v >> 16); };
    auto tag = [&](const char *t) { std::memcpy(at, t, 4); at += 4; };
    tag("RIFF");
    put32((int)(file_size - 8));
    tag("WAVE");
    tag("fmt ");
    put32(nch > 2 ? 40 : 16);
    put16(nch > 2 ? 0xFFFE : 1);
    put16(nch);
    put32(p->sample_rate);
    put32((int)((uint32_t)p->sample_rate * (uint32_t)(bps * nch)));
    put16(bps * nch);
    put16(8 * bps);
    if (nch > 2) {
        put16(22);
        put16(8 * bps);
        put32(wave_channel_mask(nch));
        std::memcpy(at, kWaveSubtypePcm, 16);
        at += 16;
    }
    if (p->looping) {
        tag("smpl");
        put32(0x3c);
        for (int i = 0; i < 7; i++) put32(0);
        put32(1);
        for (int i = 0; i < 3; i++) put32(0);
        put32(p->loop_start);
        put32(p->loop_end);
        put32(0);
        put32(0);
    }
    tag("data");
    put32((int)((uint32_t)nch * (uint32_t)p->sample_count * (uint32_t)bps));
}

// What vga_wave_read_pcm16 checks of a parsed info before it moves anything: `file_len` bytes of file lie behind it.
inline int wave_read16_check(const vga_wave_info *w, int64_t file_len)
{
    if (w->bits_per_sample != 16) { set_error("only 16-bit PCM is converted here (Pcm8 is outside this path)"); return VGA_ERR_ARGUMENT; }
    const int64_t bytes = (int64_t)w->sample_count * w->channel_count * 2;
    if (w->data_offset < 0 || w->data_offset + bytes > file_len) { set_error("info does not describe this file"); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

// ... and vga_wave_read_pcm8: the data bytes present must divide by the channel count (DeInterleave, Interleave.cs:83-85)
inline int wave_read8_check(const vga_wave_info *w, int64_t file_len)
{
    if (w->bits_per_sample != 8) { set_error("only 8-bit PCM is read here (vga_wave_read_pcm16 reads 16-bit files)"); return VGA_ERR_ARGUMENT; }
    if (w->channel_count < 1) { set_error("info does not describe this file"); return VGA_ERR_ARGUMENT; }
    if (w->data_size % w->channel_count != 0) {
        set_error("The input array length (%d) must be divisible by the number of outputs.", w->data_size);
        return VGA_ERR_INVALID_DATA;
    }
    const int64_t bytes = (int64_t)w->sample_count * w->channel_count;
    if (w->data_offset < 0 || w->data_offset + bytes > file_len) { set_error("info does not describe this file"); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

}  // namespace container
}  // namespace vga
