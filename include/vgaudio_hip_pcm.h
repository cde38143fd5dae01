/* vgaudio_hip_pcm.h -- uncompressed PCM in the NintendoWare stream and WAVE containers, and Pcm8Codec on the device.
 *
 * The GC-ADPCM-only calls of vgaudio_hip.h keep their results for every input, refusals included: these are separate
 * entry points with their own names.  All *_device calls run on the caller's stream and never synchronise it.
 */
#ifndef VGAUDIO_HIP_PCM_H
#define VGAUDIO_HIP_PCM_H

#include "vgaudio_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* NwCodec.cs */
#define VGA_NW_CODEC_PCM8 0
#define VGA_NW_CODEC_PCM16 1
#define VGA_NW_CODEC_GCADPCM 2

/* sample kind of pitched planar device rows (pitch counted in elements of the kind):
 *   VGA_SAMPLES_S16   int16 rows, what the encoders take and the decoders give;
 *   VGA_SAMPLES_8BIT  byte rows as the container stores them: signed in NW streams, unsigned in WAVE. */
#define VGA_SAMPLES_S16 0
#define VGA_SAMPLES_8BIT 1

/* ----------------------------------------------------------------------
 * Pcm8Codec (VGAudio/Codecs/Pcm8/Pcm8Codec.cs) over nrows pitched planar rows of n samples.
 * signed_ = 0: Encode (s + 0x8000) >> 8 / Decode (b - 0x80) << 8 (Pcm8Format, WAVE);
 * signed_ = 1: EncodeSigned s >> 8 / DecodeSigned (sbyte)b << 8 (Pcm8SignedFormat, NW streams).
 * Layout: byte rows at any byte, int16 rows at any short boundary, both pitches (in elements) anything >= n (less:
 * VGA_ERR_ARGUMENT); the elements behind a row are left alone.
 * -------------------------------------------------------------------- */
int vga_pcm8_encode_device(const int16_t *d_pcm, int64_t pcm_pitch, int n, int nrows, int signed_, uint8_t *d_out,
                           int64_t out_pitch, void *stream);
int vga_pcm8_decode_device(const uint8_t *d_in, int64_t in_pitch, int n, int nrows, int signed_, int16_t *d_pcm,
                           int64_t pcm_pitch, void *stream);

/* ----------------------------------------------------------------------
 * NintendoWare streams (BRSTM, BCSTM, BFSTM) with PCM8 or PCM16 audio: the Pcm16Bit / Pcm8Bit branches of
 * BrstmWriter.cs, BCFstmWriter.cs, BrstmReader.cs, BCFstmReader.cs and Common.cs.  vga_nwstm_params,
 * vga_nwstm_layout and vga_nwstm_info are reused; for PCM:
 *   - the defaults of samples_per_interleave, samples_per_seek_table_entry and loop_point_alignment are
 *     BytesToSamples(0x2000, codec): 4096 for PCM16, 8192 for PCM8; the interleave need not divide by 14;
 *   - there is no ADPC / SEEK block (seek_block_offset = seek_block_size = 0, seek_table_entry_count = 0), BRSTM
 *     carries 0 samples and 0 bytes per seek entry, BCSTM / BFSTM 4 bytes and the configured samples;
 *   - no loop alignment is done (alignment_needed = 0, layout.channel is zeroed) and the keep_* flags mean nothing;
 *   - a looping file stores SampleCount = LoopEnd: the audio is cut at the loop end;
 *   - BCSTM >= 2.3 and BFSTM >= 0.4 carry the GC-ADPCM unaligned loop points, which the reference reads from a
 *     GC-ADPCM format that a PCM stream lacks: VGA_ERR_INVALID_OP;
 *   - layout.channel_sample_count = params.sample_count (the samples of every input row) and
 *     layout.channel_adpcm_bytes = the bytes of one such row as stored.
 * PCM16 is stored in the file's byte order (BRSTM big-endian); PCM8 signed.  From VGA_SAMPLES_S16 rows a PCM8
 * write applies Pcm8Codec.EncodeSigned and a PCM8 read DecodeSigned; VGA_SAMPLES_8BIT rows are PCM8 bytes as
 * stored (a PCM16 stream takes and gives VGA_SAMPLES_S16 rows only).
 * -------------------------------------------------------------------- */
int vga_nwstm_pcm_layout_for(const vga_nwstm_params *p, int codec, int nch, vga_nwstm_layout *out);
/* nfiles equally shaped images; file f's channel c is row f*nch+c of d_samples (params.sample_count samples each,
 * pitch in elements of sample_kind); image f at d_files + f*file_pitch (file_pitch >= layout.file_size and a
 * multiple of 16 when nfiles > 1); every byte of each image is written.  Layout: d_files at any byte, d_samples at any
 * element boundary, pitch anything >= params.sample_count; a smaller pitch or a file_pitch off 16 is VGA_ERR_ARGUMENT
 * and writes nothing; no byte between two images is written */
int vga_nwstm_pcm_write_device(const vga_nwstm_params *p, int codec, int nch, int nfiles, const vga_nw_track *tracks,
                               const void *d_samples, int sample_kind, int64_t pitch, uint8_t *d_files,
                               int64_t file_pitch, void *stream);
/* one file from host rows: samples[c] params.sample_count elements of sample_kind; file_out layout.file_size bytes */
int vga_nwstm_pcm_write(const vga_nwstm_params *p, int codec, int nch, const vga_nw_track *tracks,
                        const void *const *samples, int sample_kind, uint8_t *file_out);
/* host only: vga_nwstm_parse for codec 0 / 1 streams.  info->codec tells which; info->adpcm_bytes is one channel's
 * bytes as stored (SamplesToBytes(sample_count, codec)), the coefficient and context tables stay zero.  A GC-ADPCM
 * stream (read it with vga_nwstm_parse) and any other codec give VGA_ERR_INVALID_OP. */
int vga_nwstm_pcm_parse(const uint8_t *file, size_t size, vga_nwstm_info *out);
/* nfiles images sharing one parsed geometry -> row f*channel_count+c of d_samples (info->sample_count elements of
 * sample_kind per row, pitch in elements).  Layout: images at any byte on any file_pitch that holds one (checked
 * when nfiles > 1), rows at any element boundary, pitch anything >= info->sample_count (less: VGA_ERR_ARGUMENT); the
 * elements behind a row are left alone */
int vga_nwstm_pcm_read_device(const vga_nwstm_info *info, const uint8_t *d_files, int64_t file_pitch, int nfiles,
                              void *d_samples, int sample_kind, int64_t pitch, void *stream);
/* host form: out[c] info->sample_count elements of sample_kind */
int vga_nwstm_pcm_read(const uint8_t *file, size_t size, const vga_nwstm_info *info, void *const *out, int sample_kind);

/* ----------------------------------------------------------------------
 * WAVE, 8-bit PCM: WaveWriter.cs with WaveCodec.Pcm8Bit and the 8-bit branch of WaveReader.cs.  The header is
 * the 16-bit one with 8-bit fields (block align nch, nch bytes per second per hertz, 8 valid bits in the extensible
 * fmt chunk above 2 channels); the data chunk holds nch * sample_count bytes, odd sizes included.  Samples are
 * unsigned: from VGA_SAMPLES_S16 rows the writer applies Pcm8Codec.Encode and the reader Pcm8Codec.Decode.
 * Layout of the _device calls: d_file / d_data at any byte, rows at any element boundary, pitch (in elements) anything
 * >= the sample count (less: VGA_ERR_ARGUMENT); the elements behind a row are left alone.
 * -------------------------------------------------------------------- */
int64_t vga_wave_pcm8_file_size(const vga_wave_params *p, int nch);        /* < 0 = error */
int vga_wave_write_pcm8(const void *const *samples, int sample_kind, int nch, const vga_wave_params *p, uint8_t *file_out);
int vga_wave_write_pcm8_device(const void *d_samples, int sample_kind, int64_t pitch, int nch, const vga_wave_params *p,
                               uint8_t *d_file, void *stream);
/* an 8-bit file parsed by vga_wave_parse: out[c] info->sample_count elements of sample_kind.  VGA_ERR_ARGUMENT for a
 * 16-bit file; VGA_ERR_INVALID_DATA when the data bytes present do not divide by the channel count (DeInterleave) */
int vga_wave_read_pcm8(const uint8_t *file, int64_t file_len, const vga_wave_info *info, void *const *out, int sample_kind);
/* the data chunk's bytes (any alignment) -> nch rows of sample_count elements of sample_kind */
int vga_wave_deinterleave_pcm8_device(const uint8_t *d_data, int sample_count, int nch, void *d_samples, int sample_kind,
                                      int64_t pitch, void *stream);

#ifdef __cplusplus
}
#endif
#endif
