/* vgaudio_hip_files/nw_pcm_files.h -- device-resident sets of NintendoWare stream FILES with PCM16 or PCM8 audio, of different
 * shapes: the BRSTM, BCSTM or BFSTM image of every file of a set written from planar int16 rows, and every image taken
 * apart into such rows, in one set of launches per call.  The PCM branch of the chain nw_files.h describes for GC-ADPCM:
 * WAV set -> vga_wave_read_device_v -> vga_nwstm_pcm_write_device_v never leaves HBM and issues no launch per file
 * (VGAudio.Cli/Batch.cs with --out-format pcm16 or pcm8), and neither does images -> vga_nwstm_pcm_read_device_v -> rows.
 * The scaffolding is wave_files.h's; the per-file calls are those of vgaudio_hip_pcm.h.
 *
 * It lives next to wave_files.h, outside the listings the older test files enumerate; the same disciplines are applied to
 * THIS header by tests/test_nw_pcm_files_host.py (exports, argument counts, the layout against a model, the work items'
 * tiling, the form and conversion every file takes, every refusal, and that the GPU file's table of cases names every
 * function declared here) and tests/test_gpu_nw_pcm_files.py (junk-filled buffers larger than needed, poison mode, a busy
 * caller stream, two streams at once, offsets past 4 GiB).  The hooks of this feature are declared here too, at the end.
 *
 * A SET for writing is nfiles files (vga_nw_file of nw_files.h: channel count, sample rate, sample count and the format's
 * loop), ONE vga_nw_file_config and ONE codec (VGA_NW_CODEC_PCM16 or VGA_NW_CODEC_PCM8) for all of them, as
 * VGAudio.Cli/Batch.cs applies one BxstmConfiguration to every file of a folder.  File f's vga_nwstm_params is the
 * configuration plus the file's numbers, and everything about file f is what vga_nwstm_pcm_layout_for says for those
 * params, the codec and the file's channels: the defaults are 4096 (PCM16) / 8192 (PCM8) samples per interleave, there is
 * no seek block, a looping file stores loop_end samples.  The tracks of every file are the default list,
 * AudioTrack.GetDefaultTrackList(channels); a caller's own list stays with the per-file call vga_nwstm_pcm_write_device.
 * A SET for reading is made from what vga_nwstm_pcm_parse returned for every file; its files may differ in target, codec,
 * endianness and version.
 *
 * LAYOUT (vga_nw_pcm_files_layout_for computes it on the host, no GPU needed; an object carries the same numbers)
 *   rows    exactly as wave_files.h lays them: the channels of file f are rows first_channel[f] .. first_channel[f] +
 *           channels - 1 of ONE int16_t buffer d_pcm (VGA_SAMPLES_S16 for every file: a PCM8 file goes through
 *           Pcm8Codec.EncodeSigned when written and DecodeSigned when read, as in the per-file calls).  Writing: a row is
 *           the file's sample_count samples, of which a looping file stores the first loop_end (rounded up as the
 *           reference's Interleave rounds: see WRITE).  Reading: a row is info->sample_count samples.  pcm_offsets == NULL:
 *           the rows lie in file order, each rounded up to 8 samples, a row of no samples takes no room, a guard of 128
 *           samples behind the last -- offset for offset what vga_wave_files_layout_for gives for the same counts, so one
 *           vga_wave_read_device_v output, or a decoder's packed PCM, is this set's input as it lies.  pcm_offsets != NULL
 *           (one per row, in samples): the caller's offsets at any sample boundary, rows must not overlap;
 *           totals.pcm_samples is the end of the furthest row plus 128.
 *   images  Writing: file f's image is layout.file_size bytes at image_offsets[f] of one buffer of totals.image_bytes;
 *           image_offsets == NULL packs them, every offset rounded up to 16 bytes, a guard of 256 bytes behind the last
 *           image (nothing writes it); image_offsets != NULL: the caller's offsets, multiples of 16 (anything else is
 *           VGA_ERR_ARGUMENT), images must not overlap.  Reading: image f runs to audio_data_offset + audio_data_length and
 *           starts at any byte offset the caller names (files inside archives do not start aligned), or packed as above.
 *   d_pcm must be 2-byte aligned, d_images may start at any byte (a set for writing: 16-byte aligned, as its offsets are).
 *   A null or misaligned required buffer is VGA_ERR_ARGUMENT before anything is launched.  nfiles == 0 is an empty set: every
 *   call returns 0 and launches nothing.
 *
 * REFUSED AT CREATE AND LAYOUT, the message naming the file ("file <f>: " in front of the per-file message), with the
 * per-file call's own code, because the check IS that call's code (nw_host.hpp).  Writing: whatever vga_nwstm_pcm_layout_for
 * refuses for the file's params (an unknown target, channels outside 1..255 VGA_ERR_ARGUMENT; loop points WithLoop rejects, a
 * version the writer does not produce, a file past 2 GiB VGA_ERR_OUT_OF_RANGE; BCSTM >= 2.3 and BFSTM >= 0.4
 * VGA_ERR_INVALID_OP).  Reading: what vga_nwstm_pcm_read_device refuses of an info (a GC-ADPCM info, an info that does not
 * describe a stream, VGA_ERR_ARGUMENT).  Of the set itself: an unknown codec, a null configuration, a negative offset, an
 * image offset of a set for writing off 16, rows that overlap, images of a set for writing that overlap, a null info, an
 * info of negative offsets or more than 255 channels, more than 2^31 rows VGA_ERR_ARGUMENT; more than 2^62 bytes and an
 * image of a set for reading past 2 GiB VGA_ERR_OUT_OF_RANGE; a PCM16 info whose interleave or bytes per channel are odd
 * VGA_ERR_INVALID_OP (no writer makes one; vga_nwstm_pcm_read_device reads it).  Every file's own checks come before the
 * offsets' checks.  A file of 0 samples is a good file: headers and an empty DATA block.
 * A set made for writing refuses the read call and the other way round with VGA_ERR_INVALID_OP.
 *
 * WRITE  image f is byte for byte what vga_nwstm_pcm_write_device writes for that file alone with tracks = NULL: the file
 * header, HEAD / INFO, the DATA header and Interleave(rows, interleave_size, audio_data_size) of the stored samples -- PCM16
 * in the file's byte order, PCM8 the high byte of every short; the bytes no row supplies (the last block's padding to 0x20,
 * what lies behind a looping file's rows) are zero.  As the reference's Interleave does, a looping file whose loop_end
 * falls inside a block stores the row's samples to the end of that block's 0x20 rounding, not zeros.  At most THREE launches
 * whatever nfiles is:
 *   1. headers   one workgroup per file: the body the per-file call's header kernel runs (nw_header_body.hpp);
 *   2. vector    (file, chunk) items, below;
 *   3. general   (file, chunk) items, below.
 * There is no memset: every byte of every image is written by these kernels, and no byte between two images, behind the last
 * one, in a rounding gap or in a guard is.  Nothing outside a row's own samples is read.
 * READ   row c receives exactly what vga_nwstm_pcm_read_device delivers into an int16 row: samples no block supplies are
 * zero, nothing is written behind a row's end, and nothing outside an image's own bytes is read.  At most TWO launches (the
 * vector items, the general items); a launch without items is not made.
 *
 * WHICH KERNELS.  Block b of the audio holds interleave_size bytes of each channel in turn, so every (file, block, channel)
 * segment is a contiguous run of one row and the work is a converting copy: COPY (PCM16, little-endian file), SWAP16 (PCM16,
 * big-endian file: every BRSTM) or PCM8.  The VECTOR form moves one 16-byte granule of the FILE side per thread as aligned
 * 16-byte vector accesses on both sides (a PCM8 write loads 32 bytes of row per 16 stored, a PCM8 read stores 32 bytes of
 * row per 16 loaded), converts whole dwords with v_perm_b32, and writes the zero fill with the same threads; a granule a
 * row supplies only in part, or that would cross a row's end, goes sample by sample.  Items are chunks of 1024 granules of
 * one file's audio (write) or of one row as stored (read), 256 threads.  A file takes the VECTOR form when its
 * interleave_size and its last block's size are multiples of 16 bytes, image offset + audio offset is on 16 bytes and every
 * row offset of the file is on 8 samples: every packed set at the default configuration.  Every other file (an interleave of
 * 1001 PCM8 or 5 PCM16 samples, caller's row offsets off 8 samples, read images at odd byte offsets) takes the GENERAL form,
 * the same addressing one sample per thread.  The form is chosen per file on the host at create; a call whose d_pcm or
 * d_images is not 16-byte aligned takes the general form for every file.  vga_nw_pcm_files_stats says how many files and
 * items take which.  All offsets inside an image fit 32 bits (FileSize is an int); image and row bases are int64_t.
 *
 * All calls run on the caller's stream and never synchronise it; they need no workspace; the library allocates nothing per
 * call.  The object keeps its tables in the memory of the device that was current at create, is immutable and serves any
 * number of calls, concurrent calls on different streams included.
 *
 * LEFT OUT: byte rows (VGA_SAMPLES_8BIT) in sets -- rows are int16 for every file; custom track lists in sets; host-pointer
 * forms of the _v calls; moving the per-file PCM calls (vga_nwstm_pcm_write_device / _read_device) onto these kernels (that
 * changes an existing call's launches and belongs to a change of its own). */
#ifndef VGAUDIO_HIP_FILES_NW_PCM_FILES_H
#define VGAUDIO_HIP_FILES_NW_PCM_FILES_H

#include "../vgaudio_hip/nw_files.h"
#include "../vgaudio_hip_pcm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { int files, channels; int64_t pcm_samples, image_bytes; } vga_nw_pcm_files_totals;   /* guards included */
typedef struct vga_nw_pcm_files vga_nw_pcm_files;

/* host only, needs no GPU.  codec: VGA_NW_CODEC_PCM8 / PCM16.  pcm_offsets: one per row (samples), or NULL for packed rows;
 * image_offsets: one per file (bytes, multiples of 16), or NULL for packed images.  first_channel_out / image_offsets_out:
 * nfiles entries; pcm_offsets_out: one per row; any output may be NULL, but not all of them. */
int  vga_nw_pcm_files_layout_for(const vga_nw_file *files, int nfiles, const vga_nw_file_config *config, int codec,
                                 const int64_t *pcm_offsets, const int64_t *image_offsets, int *first_channel_out,
                                 int64_t *pcm_offsets_out, int64_t *image_offsets_out, vga_nw_pcm_files_totals *totals_out);
/* a set for WRITING: the same checks, then the tables in the current device's memory */
int  vga_nw_pcm_files_create(const vga_nw_file *files, int nfiles, const vga_nw_file_config *config, int codec,
                             const int64_t *pcm_offsets, const int64_t *image_offsets, vga_nw_pcm_files **out);
/* a set for READING, from what vga_nwstm_pcm_parse returned for every file; image_offsets: any byte offsets, or NULL */
int  vga_nw_pcm_files_create_from_infos(const vga_nwstm_info *const *infos, int nfiles, const int64_t *pcm_offsets,
                                        const int64_t *image_offsets, vga_nw_pcm_files **out);
void vga_nw_pcm_files_destroy(vga_nw_pcm_files *s);
int  vga_nw_pcm_files_totals_of(const vga_nw_pcm_files *s, vga_nw_pcm_files_totals *out);
int  vga_nw_pcm_files_offsets(const vga_nw_pcm_files *s, int *first_channel_out, int64_t *pcm_offsets_out, int64_t *image_offsets_out);

int  vga_nwstm_pcm_write_device_v(const vga_nw_pcm_files *s, const int16_t *d_pcm, uint8_t *d_images, void *stream);
int  vga_nwstm_pcm_read_device_v(const vga_nw_pcm_files *s, const uint8_t *d_images, int16_t *d_pcm, void *stream);

/* ---- hooks of this feature (tests and tools)
 * The work items of a set, host only: what the kernels of a call are launched over, in launch order.  begin / end: the bytes
 * the item writes, counted from the start of the file's image (write) or of the row, in bytes of int16 samples (read).
 * HEADER items exist in a set for writing only, one per file, and cover everything in front of the audio.  x, y: the item
 * as the kernel reads it -- file (write) or row (read), index of a chunk of 1024 granules of 16 stored bytes.  conv: the
 * file's conversion.  general != 0: the items of a call under vga_nw_pcm_files_force_general_this_thread(1).  items_out may
 * be NULL (the count alone); more than `capacity` items is VGA_ERR_ARGUMENT with the count in *count_out. */
#define VGA_NW_PCM_FILES_HEADER 0
#define VGA_NW_PCM_FILES_VECTOR 1
#define VGA_NW_PCM_FILES_GENERAL 2
#define VGA_NW_PCM_FILES_COPY 0
#define VGA_NW_PCM_FILES_SWAP16 1
#define VGA_NW_PCM_FILES_PCM8 2
typedef struct { int form, file, x; uint32_t y; int conv; int64_t begin, end; } vga_nw_pcm_files_item;
int  vga_nw_pcm_files_write_items_for(const vga_nw_file *files, int nfiles, const vga_nw_file_config *config, int codec,
                                      const int64_t *pcm_offsets, const int64_t *image_offsets, int general,
                                      vga_nw_pcm_files_item *items_out, int64_t capacity, int64_t *count_out);
int  vga_nw_pcm_files_read_items_for(const vga_nwstm_info *const *infos, int nfiles, const int64_t *pcm_offsets,
                                     const int64_t *image_offsets, int general, vga_nw_pcm_files_item *items_out,
                                     int64_t capacity, int64_t *count_out);
/* out[0..3]: files in the vector form, files in the general form (files that move no samples count in neither), vector
 * items, general items -- of a call made by this thread now on 16-byte aligned buffers (the force hook applies) */
int  vga_nw_pcm_files_stats(const vga_nw_pcm_files *s, int64_t *out /*[4]*/);
/* per thread: the _v calls of this thread take the general form for every file.  Returns the previous value. */
int  vga_nw_pcm_files_force_general_this_thread(int on);

#ifdef __cplusplus
}
#endif
#endif
