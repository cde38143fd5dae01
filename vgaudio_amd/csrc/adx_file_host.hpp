// adx_file_host.hpp -- the host side of ONE ADX file image without HIP: AdxWriter's size math (vga_adx_file_layout_for's code)
// and what vga_adx_write_device checks and hands its header and footer kernels.  It exists once: capi_containers.hip calls it
// for the per-file calls, adx_files_host.hpp for every file of a set (include/vgaudio_hip/adx_files.h), which is why a set
// refuses a file with the per-file call's own code and message.  Header-only and free of <hip/hip_runtime.h>, so that a
// stand-alone host program can include it (tests/host/adx_files_host_driver.cpp); whoever includes it supplies vga::set_error.
#pragma once
#include "adx_host.hpp"
#include "container_math.hpp"

#include <algorithm>
#include <cstring>

namespace vga {
namespace container {

// what the header and footer kernels take (AdxWriter.WriteHeader :81-117, the footer :133-138)
struct AdxHeaderArgs {
    int header_size, type, frame_size, nch, sample_rate, sample_count, highpass_frequency, version, encryption_type;
    int alignment_samples, looping, loop_start, loop_start_offset, loop_end, loop_end_offset;
    int footer_pos, footer_size, file_size;
};

// AdxWriter.cs:14-37,58-69
inline int adx_file_layout(const vga_adx_file_params *p, int nch, vga_adx_file_layout *L)
{
    if (!p || !L) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (nch < 1 || nch > 255) { set_error("ADX channel count %d does not fit the header byte", nch); return VGA_ERR_ARGUMENT; }
    if (p->frame_size < 3 || p->frame_size > 255) { set_error("ADX frame size %d out of range", p->frame_size); return VGA_ERR_ARGUMENT; }
    if (p->sample_count < 0 || p->loop_start < 0 || p->loop_end < 0) { set_error("negative sample count / loop point"); return VGA_ERR_OUT_OF_RANGE; }
    std::memset(L, 0, sizeof *L);
    const int spf = (p->frame_size - 2) * 2;                                                            // :27
    L->sample_count = (p->trim_file && p->looping) ? p->loop_end + spf * 3 : p->sample_count;           // :21
    L->frame_count = div_round_up(L->sample_count, spf);                                                // :28
    L->base_header_size = p->looping ? (p->version == 4 ? 60 : 52) : (p->version == 4 ? 36 : 32);        // :30
    if (p->looping) {                                                                                   // :58-69
        const int start = adx::sample_count_to_byte_count(p->loop_start, p->frame_size) * nch + L->base_header_size + 4;
        L->alignment_bytes = (int)next_multiple(start, 0x800) - start;
        if (p->version == 3) L->alignment_bytes += p->alignment_samples / spf * 0x800;
    }
    L->header_size = L->base_header_size + L->alignment_bytes;
    L->audio_offset = L->header_size + 4;
    const int64_t audio_size = (int64_t)p->frame_size * L->frame_count * nch;
    if (audio_size + L->audio_offset + 0x1000 > 0x7FFFFFFF) { set_error("ADX file would exceed 2 GiB (FileSize is an int)"); return VGA_ERR_OUT_OF_RANGE; }
    L->audio_size = (int)audio_size;
    L->footer_offset = L->audio_offset + L->audio_size;
    L->footer_size = p->looping ? (int)next_multiple(L->footer_offset + p->frame_size, 0x800) - L->footer_offset : p->frame_size;
    L->loop_start_offset = L->audio_offset + adx::sample_count_to_byte_count(p->loop_start, p->frame_size) * nch;
    L->loop_end_offset = L->audio_offset + (int)next_multiple(adx::sample_count_to_byte_count(p->loop_end, p->frame_size), p->frame_size) * nch;
    L->file_size = L->audio_offset + L->audio_size + L->footer_size;                                    // :18
    return VGA_OK;
}

// where the header fields end, written one after the other whatever HeaderSize is (WriteHeader :83-112)
inline int adx_header_fields_end(int version, int nch) { return 20 + (version == 4 ? 4 + 4 * nch + (nch == 1 ? 4 : 0) : 0) + 24; }

// the layout of a file whose channels hold audio_len bytes each, and the kernels' arguments
inline int adx_args(const vga_adx_file_params *p, int nch, int audio_len, vga_adx_file_layout *L, AdxHeaderArgs *a)
{
    if (int rc = adx_file_layout(p, nch, L)) return rc;
    a->header_size = L->header_size; a->type = p->type; a->frame_size = p->frame_size; a->nch = nch;
    a->sample_rate = p->sample_rate; a->sample_count = L->sample_count; a->highpass_frequency = p->highpass_frequency;
    a->version = p->version; a->encryption_type = p->encryption_type; a->alignment_samples = p->alignment_samples;
    a->looping = p->looping ? 1 : 0; a->loop_start = p->loop_start; a->loop_start_offset = L->loop_start_offset;
    a->loop_end = p->loop_end; a->loop_end_offset = L->loop_end_offset;
    a->footer_size = L->footer_size; a->file_size = L->file_size;
    // the footer goes where the interleaver leaves the stream (Interleave.cs:58-77): after the blocks it copied,
    // which is short of FooterOffset when the (trimmed) frame count exceeds the frames the channels hold
    const int in_blocks = div_round_up(audio_len, p->frame_size);
    a->footer_pos = L->audio_offset + std::min(in_blocks, L->frame_count) * p->frame_size * nch;
    // everything the header writes must fit the image (MemoryStream over byte[FileSize] is not expandable)
    const int header_end = adx_header_fields_end(p->version, nch);
    if (header_end > L->file_size || L->header_size + 4 > L->file_size || L->header_size < 2) {
        set_error("ADX header (%d bytes written) does not fit the %d-byte file", header_end, L->file_size);
        return VGA_ERR_INVALID_OP;                          // NotSupportedException
    }
    return VGA_OK;
}

}  // namespace container
}  // namespace vga
