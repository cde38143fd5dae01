// pcm_kernels.hpp -- launchers for the PCM gathers and scatters of the NintendoWare stream writers and readers, fused
// with the sample conversion (pcm_kernels.hip)
#pragma once
#include "common.hpp"

namespace vga {
namespace pcm {

// how a channel's bytes in the file relate to its int16 row
enum Conv : int {
    kSwap16 = 0,   // PCM16 in the other byte order than the row: the bytes of every sample swapped
    kPcm8 = 1,     // PCM8 signed: written as s >> 8 (Pcm8Codec.EncodeSigned), read as (sbyte)b << 8 (DecodeSigned)
};

// Interleave(channels, interleave, output_size) (Utilities/Interleave.cs:43-78) into the audio region of nfiles
// images from int16 rows (row f*nch+c at src + row * pitch samples), converting on the way; input_size is the
// bytes of one row AS STORED (the file's bytes per sample * samples).  Every byte of the region is written.
int launch_interleave_files(Conv conv, const int16_t *src, int64_t pitch, int nch, int nfiles, uint32_t input_size,
                            uint32_t interleave, uint32_t output_size, uint8_t *dst, int64_t file_pitch, hipStream_t s);
// DeInterleave (Interleave.cs:118-167) of `rows` channel rows (file = row / nch) into int16 rows of output_size / bps
// samples, converting on the way
int launch_deinterleave(Conv conv, const uint8_t *files, int64_t file_pitch, int audio_offset, int nch, int rows,
                        uint32_t input_size, uint32_t interleave, uint32_t output_size, int16_t *dst, int64_t dst_pitch,
                        hipStream_t s);

}  // namespace pcm
}  // namespace vga
