/* vgaudio_hip_files/wave_files.h -- device-resident sets of WAVE FILES of different shapes: the data chunk of every file of a
 * set taken apart into planar int16 rows, and the image of every file written from such rows, in one set of launches per
 * call.  The first and the last step of every chain gc_files.h, nw_files.h, adx_files.h and hca_files.h describe ("WAV set
 * -> ..."): images -> vga_wave_read_device_v -> a ragged object's encode never leaves HBM and issues no launch per file
 * (WaveReader for a whole folder, VGAudio.Cli/Batch.cs), and neither does decoded rows -> vga_wave_write_device_v.  The
 * scaffolding is adx_files.h's.
 *
 * It lives in a directory of its own, outside the listings the older test files enumerate; the same disciplines are applied
 * to THIS header by tests/test_wave_files_host.py (exports, argument counts, the layout against a model, the work items'
 * tiling, the form every file takes, every refusal, and that the GPU file's table of cases names every function declared
 * here) and tests/test_gpu_wave_files.py (junk-filled buffers larger than needed, poison mode, a busy caller stream, two
 * streams at once, offsets past 4 GiB).  The hooks of this feature are declared here too, at the end.
 *
 * A SET is nfiles files (vga_wave_file: the channel count, 16 or 8 bits, and the file's own vga_wave_params, exactly what
 * vga_wave_write_pcm16_device / vga_wave_write_pcm8_device take), or, for reading, what vga_wave_parse returned for every
 * file.
 *
 * LAYOUT (vga_wave_files_layout_for computes it on the host, no GPU needed; an object carries the same numbers)
 *   rows    the channels of file f are rows first_channel[f] .. first_channel[f] + channels - 1 of ONE int16_t buffer d_pcm
 *           (VGA_SAMPLES_S16, for 8-bit files too: the reader applies Pcm8Codec.Decode, the writer Pcm8Codec.Encode).  A
 *           row is the file's sample_count samples (a set for reading: info->sample_count, from the bytes present).
 *           pcm_offsets == NULL: the rows lie in file order, each rounded up to 8 samples, a row of no samples takes no
 *           room, a guard of 128 samples behind the last (nothing writes it and the set's kernels never need it) -- offset
 *           for offset what vga_adx_ragged_layout_for, vga_hca_ragged_layout_for (stream-major is file-major) and
 *           vga_gcadpcm_ragged_offsets give for the same counts, so ONE set's output is a ragged object's d_pcm as it lies;
 *           the caller allocates the larger of the two totals.  pcm_offsets != NULL (one per row, in samples): the caller's
 *           offsets at any sample boundary, rows must not overlap; totals.pcm_samples is the end of the furthest row plus
 *           128.  That is for files that go to several ragged objects inside one allocation.
 *   images  Writing: file f's image is vga_wave_file_size / vga_wave_pcm8_file_size bytes at image_offsets[f] of one buffer
 *           of totals.image_bytes; image_offsets == NULL packs them, every offset rounded up to 16 bytes, a guard of 256
 *           bytes behind the last image (nothing writes it); image_offsets != NULL: the caller's offsets at ANY byte,
 *           images must not overlap.  Reading: image f runs to data_offset + data_size (only the data chunk is read) and
 *           starts at any byte offset the caller names (WAV files inside archives do not start aligned), or packed as above.
 *   d_pcm must be 2-byte aligned, d_images may start at any byte: the kernels look at the addresses they find.  A null or
 *   misaligned required buffer is VGA_ERR_ARGUMENT before anything is launched.  nfiles == 0 is an empty set: every call
 *   returns 0 and launches nothing.
 *
 * REFUSED AT CREATE AND LAYOUT, the message naming the file ("file <f>: " in front of the per-file message), with the
 * per-file call's own code, because the check IS that call's code (wave_file_host.hpp): what vga_wave_file_size and
 * vga_wave_pcm8_file_size refuse ("bad WAVE parameters" VGA_ERR_ARGUMENT: channels outside 1..32767, a negative count; a
 * file past 2 GiB VGA_ERR_OUT_OF_RANGE); of a parsed info what vga_wave_read_pcm16 refuses (anything but 8 bits is held
 * to that call: "only 16-bit PCM is converted here", an info whose samples do not fit its data bytes) and what
 * vga_wave_read_pcm8 refuses (data bytes present that do not divide by the channel count, VGA_ERR_INVALID_DATA).  Of the set
 * itself: bits other than 16 or 8, a negative offset, rows that overlap, images of a set for writing that overlap, a
 * null info, an info of negative counts or of more than 65535 channels, more than 2^31 rows (found before a row is placed)
 * VGA_ERR_ARGUMENT; more than 2^62 bytes (a row offset past 2^61 samples, an image offset past 2^62 bytes) and an info whose
 * data_offset lies past 2 GiB VGA_ERR_OUT_OF_RANGE.  Every file's own checks come before the offsets' checks.
 * A set made for writing refuses the read call and the other way round with VGA_ERR_INVALID_OP.
 *
 * READ   row c receives exactly what vga_wave_deinterleave_pcm16_device / vga_wave_deinterleave_pcm8_device deliver for
 * its file; nothing is written behind a row's end, into the rounding gaps or into the guard.  At most TWO launches whatever
 * nfiles is (the tile items, the general items; a launch without items is not made).
 * WRITE  image f is byte for byte what vga_wave_write_pcm16_device / vga_wave_write_pcm8_device write for that file alone:
 * the RIFF, fmt (extensible above two channels), smpl (looping files) and data headers, odd 8-bit data sizes included.  At
 * most THREE launches whatever nfiles is:
 *   1. headers   one workgroup per file copies the header the host laid out at create (at most 136 bytes);
 *   2. tile      (file, span of frames) items, below;
 *   3. general   (file, chunk) items, below.
 * There is no memset: every byte of every image is written by these kernels, and no byte between two images, behind the last
 * one or in a guard is.
 *
 * WHICH KERNELS.  The TILE form serves files whose frame (channels * bits / 8 bytes) is at most 2048 bytes, so that 8 frames
 * fit 16 KiB: a workgroup takes a span of F frames of one file (F a multiple of 8, at most 16 KiB of interleaved bytes),
 * moves the interleaved side with 16-byte vectors at ALIGNED addresses whatever the image's own alignment is (lead and tail
 * bytes go singly; no access falls outside the span's own bytes), puts the span through LDS, and moves the planar side as
 * 16-byte vectors of 8 samples where the row's address is on 16 bytes, as single samples otherwise.  A mono 16-bit file is
 * the degenerate case, a realigning copy through the same kernel.  Every other file takes the GENERAL form, for any channel
 * count: one thread per granule of the output (read: 8 samples of a row; write: 16 bytes of the data chunk), gathered
 * sample by sample, in chunks of 2048 granules.  The forms are chosen on the host at create; vga_wave_files_stats says how
 * many files and items take which.
 *
 * All calls run on the caller's stream and never synchronise it; they need no workspace; the library allocates nothing per
 * call.  The object keeps its tables in the memory of the device that was current at create, is immutable and serves any
 * number of calls, concurrent calls on different streams included.
 *
 * LEFT OUT: byte rows (VGA_SAMPLES_8BIT) in sets -- rows are int16 for every file; host-pointer forms of the _v calls;
 * moving the per-file WAVE calls onto the tile kernel (that changes an existing call's launches and belongs to a change of
 * its own); WAVE files of other sample formats (float, 24-bit, ADPCM), which the reference refuses too. */
#ifndef VGAUDIO_HIP_FILES_WAVE_FILES_H
#define VGAUDIO_HIP_FILES_WAVE_FILES_H

#include "../vgaudio_hip_pcm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { int channels; int bits; vga_wave_params params; } vga_wave_file;   /* bits: 16 or 8; params: as the _write_ calls take them */
typedef struct { int files, channels; int64_t pcm_samples, image_bytes; } vga_wave_files_totals;   /* guards included */
typedef struct vga_wave_files vga_wave_files;

/* host only, needs no GPU.  pcm_offsets: one per row (samples), or NULL for packed rows; image_offsets: one per file
 * (bytes), or NULL for packed images.  first_channel_out / image_offsets_out: nfiles entries; pcm_offsets_out: one per row;
 * any output may be NULL, but not all of them. */
int  vga_wave_files_layout_for(const vga_wave_file *files, int nfiles, const int64_t *pcm_offsets, const int64_t *image_offsets,
                               int *first_channel_out, int64_t *pcm_offsets_out, int64_t *image_offsets_out,
                               vga_wave_files_totals *totals_out);
/* a set for WRITING: the same checks, then the tables in the current device's memory */
int  vga_wave_files_create(const vga_wave_file *files, int nfiles, const int64_t *pcm_offsets, const int64_t *image_offsets,
                           vga_wave_files **out);
/* a set for READING, from what vga_wave_parse returned for every file */
int  vga_wave_files_create_from_infos(const vga_wave_info *const *infos, int nfiles, const int64_t *pcm_offsets,
                                      const int64_t *image_offsets, vga_wave_files **out);
void vga_wave_files_destroy(vga_wave_files *s);
int  vga_wave_files_totals_of(const vga_wave_files *s, vga_wave_files_totals *out);
int  vga_wave_files_offsets(const vga_wave_files *s, int *first_channel_out, int64_t *pcm_offsets_out, int64_t *image_offsets_out);

int  vga_wave_read_device_v(const vga_wave_files *s, const uint8_t *d_images, int16_t *d_pcm, void *stream);
int  vga_wave_write_device_v(const vga_wave_files *s, const int16_t *d_pcm, uint8_t *d_images, void *stream);

/* ---- hooks of this feature (tests and tools)
 * The work items of a set, host only: what the kernels of a call are launched over, in launch order.  begin / end: the bytes
 * the item writes, counted from the start of the file's image (write) or of the row, in bytes of int16 samples (read); a
 * TILE item of a set for reading writes [begin, end) of EVERY row of its file.  HEADER items exist in a set for writing
 * only, one per file.  x, y: the item as the kernel reads it -- TILE: file, first frame; GENERAL: file (write) or row (read),
 * index of a chunk of 2048 granules.  span: frames of a TILE item's file per span (F), 0 otherwise.  general != 0: the items
 * of a call under vga_wave_files_force_general_this_thread(1).  items_out may be NULL (the count alone); more than `capacity`
 * items is VGA_ERR_ARGUMENT with the count in *count_out. */
#define VGA_WAVE_FILES_HEADER 0
#define VGA_WAVE_FILES_TILE 1
#define VGA_WAVE_FILES_GENERAL 2
#define VGA_WAVE_FILES_MAX_TILE_FRAME 2048 /* bytes of a frame: at most this in the TILE form */
typedef struct { int form, file, x; uint32_t y; int span; int64_t begin, end; } vga_wave_files_item;
int  vga_wave_files_write_items_for(const vga_wave_file *files, int nfiles, const int64_t *pcm_offsets, const int64_t *image_offsets,
                                    int general, vga_wave_files_item *items_out, int64_t capacity, int64_t *count_out);
int  vga_wave_files_read_items_for(const vga_wave_info *const *infos, int nfiles, const int64_t *pcm_offsets,
                                   const int64_t *image_offsets, int general, vga_wave_files_item *items_out, int64_t capacity,
                                   int64_t *count_out);
/* out[0..3]: files in the tile form, files in the general form (files that move no samples count in neither), tile items,
 * general items -- of a call made by this thread now (the force hook applies) */
int  vga_wave_files_stats(const vga_wave_files *s, int64_t *out /*[4]*/);
/* per thread: the _v calls of this thread take the general form for every file.  Returns the previous value. */
int  vga_wave_files_force_general_this_thread(int on);

#ifdef __cplusplus
}
#endif
#endif
