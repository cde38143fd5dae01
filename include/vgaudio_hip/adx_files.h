/* vgaudio_hip/adx_files.h -- device-resident sets of CRI ADX FILES of different shapes: the image of every file of a set,
 * written and read, in one set of launches per call.  The consumer of the rows adx_ragged.h leaves: WAV set ->
 * vga_adx_encode_device_v -> vga_adx_write_device_v never leaves HBM and issues no launch per file (AdxWriter for a whole
 * folder, VGAudio.Cli/Batch.cs), and neither does images -> vga_adx_read_device_v.  The first codec outside GC-ADPCM with
 * file sets; the scaffolding is nw_files.h's.
 *
 * It lives next to nw_files.h and outside the directory listing the older test files enumerate; the same disciplines are
 * applied to THIS header by tests/test_adx_files_host.py (exports, argument counts, the layout against a model, the work
 * items' tiling, the form every file takes, every refusal, and that the GPU file's table of cases names every function
 * declared here) and tests/test_gpu_adx_files.py (junk-filled buffers larger than needed, poison mode, a busy caller
 * stream, two streams at once).  The hooks of this feature are declared here too, at the end.
 *
 * A SET is nfiles files (vga_adx_file: the channel count and the file's own vga_adx_file_params, exactly what
 * vga_adx_write_device takes: rate, loop, alignment samples, frame size, version, type, trim).  Everything about file f is
 * what vga_adx_file_layout_for says for its params.
 *
 * LAYOUT (vga_adx_files_layout_for computes it on the host, no GPU needed; an object carries the same numbers)
 *   rows    the channels of file f are rows first_channel[f] .. first_channel[f] + channels - 1 of d_audio.  A row is
 *           ceil(params.sample_count / spf) * frame_size bytes (spf = (frame_size - 2) * 2): vga_adx_encoded_byte_count of
 *           the unaligned sample count with padding = alignment_samples.  audio_offsets == NULL: the rows lie as
 *           vga_adx_ragged_layout_for packs rows of those byte counts -- the caller's order, each rounded up to 16 bytes, a
 *           row of no bytes takes no room, a guard of 256 bytes behind the last -- so ONE vga_adx_ragged object's output is a
 *           set's input as it lies.  audio_offsets != NULL (one per row): the caller's offsets, multiples of 4, rows must
 *           not overlap; totals.audio_bytes is the end of the furthest row plus 256.  That is for files that differ in
 *           sample rate or loop padding (a ragged object takes ONE vga_adx_params): each object's buffer at a base inside
 *           one allocation, the files ordered by group.  d_history is indexed by row; it is required if any file is
 *           version 4 and read for those files only.
 *   images  File f's image is layout.file_size bytes at image_offsets[f] of one buffer of totals.image_bytes; offsets are
 *           rounded up to 16 bytes and a guard of 256 bytes follows the last image (nothing writes it).  For a set made
 *           from parsed headers image f runs to audio_offset + audio_bytes * channel_count and starts at ANY byte offset the
 *           caller names (ADX files inside archives do not start aligned), or packed as above.
 *   d_audio and d_images must be 16-byte aligned.  Anything less, or a null required buffer, is VGA_ERR_ARGUMENT before
 *   anything is launched.  nfiles == 0 is an empty set: every call returns 0 and launches nothing.
 *
 * REFUSED AT CREATE AND LAYOUT, the message naming the file ("file <f>: " in front of the per-file message), with the
 * per-file call's own code, because the check IS that call's code (adx_file_host.hpp): whatever vga_adx_file_layout_for
 * refuses (channels outside 1..255, a frame size outside 3..255 VGA_ERR_ARGUMENT; negative counts, a file past 2 GiB
 * VGA_ERR_OUT_OF_RANGE) and what vga_adx_write_device adds ("ADX header (.. bytes written) does not fit the ..-byte file",
 * VGA_ERR_INVALID_OP).  One refusal is the set's own: a file whose image has no room for the footer's four bytes (3-byte
 * frames without a loop) is VGA_ERR_INVALID_OP, as the reference throws; the per-file call drops the fourth byte instead and
 * keeps doing so.  Of the set itself: an audio offset that is negative or no multiple of 4, rows that overlap, more
 * than 2^31 rows VGA_ERR_ARGUMENT; more than 2^62 bytes VGA_ERR_OUT_OF_RANGE.  A set from parsed headers refuses the info
 * vga_adx_read_device refuses ("info does not describe an ADX file", VGA_ERR_ARGUMENT; here also for an info of no audio
 * bytes, which that call returns from before it looks), a null info and a negative image offset.
 *
 * A set made for writing refuses the read call and the other way round with VGA_ERR_INVALID_OP.
 *
 * WRITE  image f is byte for byte what vga_adx_write_device writes for that file alone (AdxWriter.cs:81-138,
 * Interleave.cs:43-78), the reference's quirks included: the header fields are written one after the other whatever
 * HeaderSize is (a 255-channel version-4 header runs 1068 bytes), "(c)CRI" and the audio overwrite what ran past it, the
 * footer sits where the interleaver left the stream when a trimmed looping file asks for more frames than the rows hold,
 * and rows are truncated when it asks for fewer.  A fixed number of launches whatever nfiles is, applied in this order
 * where they overlap:
 *   1. headers    one workgroup per file: zeros up to the audio offset (or the end of the header fields, if that is
 *                 later), the fields, "(c)CRI";
 *   2. audio      min(frames the rows hold, frames asked) frames of every channel, over (file, span of frames) work items
 *                 in a 1-D grid, in at most two forms (below);
 *   3. footers    one workgroup per file: 0x8001 and the padding size where the audio ended, zeros from there to the end of
 *                 the image -- except over header fields that ran past that point, which stay, as in the reference.
 * There is no memset: every byte of every image is written by these kernels, and no byte between two images, behind the
 * last one or in a guard is.
 * READ   row c receives what vga_adx_read_device delivers for its file: the frames of one channel back to back; nothing is
 * written behind a row's end or into the guards.  d_history_out (one short per row, or NULL) gets history[c][0] of the
 * infos, uploaded at create: what vga_adx_decode_device takes as its start history.
 *
 * WHICH KERNELS.  The SPAN form serves files of 18-byte frames, at most 113 channels and rows at multiples of 16 bytes: a
 * workgroup takes a span of frames of one file (a multiple of 8 frames per channel, at most 16 KiB), moves it through LDS
 * with aligned 16-byte vectors on both sides, whatever the image's own alignment is; lead and tail bytes go singly.  The
 * read side's body is vga_adx_read_device's fast kernel's (one device function for both), the write side is its mirror
 * image.  Every other file takes the GENERAL form, for any frame size and channel count: one thread per granule of the
 * output, the granule as wide (16 .. 1 bytes) as the frame size, the row offsets and the image's audio offset allow; a
 * mono file is a plain copy and the frame size does not enter.  vga_adx_files_stats says how many files and items take
 * which.
 *
 * All calls run on the caller's stream and never synchronise it; they need no workspace; the library allocates nothing per
 * call.  The object keeps its tables in the memory of the device that was current at create, is immutable and serves any
 * number of calls, concurrent calls on different streams included.
 *
 * Keyed encryption of sets is vgaudio_hip_files/adx_keyed_files.h's, on the objects made here; in the calls of THIS header
 * encryption_type is the header byte only, as in vga_adx_write_device.
 *
 * LEFT OUT: host-pointer
 * forms of the _v calls; HCA file sets (header plus copy: they can follow on this scaffolding); a ragged ADX decode with a
 * start history per channel (vga_adx_params.history is one value per object, so the read side ends at the rows and the
 * histories); moving the per-file vga_adx_write_device onto the span kernel (that changes an existing call's launches and
 * belongs to a change of its own). */
#ifndef VGAUDIO_HIP_ADX_FILES_H
#define VGAUDIO_HIP_ADX_FILES_H

#include "adx_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { int channels; vga_adx_file_params params; } vga_adx_file;   /* params: as vga_adx_write_device takes them */
typedef struct { int files, channels; int64_t audio_bytes, image_bytes; } vga_adx_files_totals;   /* guards included */
typedef struct vga_adx_files vga_adx_files;

/* host only, needs no GPU.  audio_offsets: one per row, or NULL for packed rows.  first_channel_out / image_offsets_out:
 * nfiles entries; audio_offsets_out: one per row; any output may be NULL, but not all of them. */
int  vga_adx_files_layout_for(const vga_adx_file *files, int nfiles, const int64_t *audio_offsets,
                              int *first_channel_out, int64_t *audio_offsets_out, int64_t *image_offsets_out,
                              vga_adx_files_totals *totals_out);
/* the same checks, then the tables in the current device's memory */
int  vga_adx_files_create(const vga_adx_file *files, int nfiles, const int64_t *audio_offsets, vga_adx_files **out);
/* a set for READING, from what vga_adx_parse returned for every file.  The rows are info->audio_bytes bytes each, packed;
 * image f is at image_offsets[f] (any byte), or packed as the writer packs. */
int  vga_adx_files_create_from_infos(const vga_adx_file_info *const *infos, int nfiles,
                                     const int64_t *image_offsets /* NULL: packed */, vga_adx_files **out);
void vga_adx_files_destroy(vga_adx_files *s);
int  vga_adx_files_totals_of(const vga_adx_files *s, vga_adx_files_totals *out);
int  vga_adx_files_offsets(const vga_adx_files *s, int *first_channel_out, int64_t *audio_offsets_out, int64_t *image_offsets_out);

int  vga_adx_write_device_v(const vga_adx_files *s, const uint8_t *d_audio, const int16_t *d_history, uint8_t *d_images,
                            void *stream);
int  vga_adx_read_device_v(const vga_adx_files *s, const uint8_t *d_images, uint8_t *d_audio, int16_t *d_history_out,
                           void *stream);

/* ---- hooks of this feature (tests and tools)
 * The work items of a set, host only: what the kernels of a call are launched over, in launch order.  begin / end: the bytes
 * the item writes, counted from the start of the file's image (write) or of the row (read).  HEADER and FOOTER items exist
 * in a set for writing only, one each per file; a footer item leaves the bytes below `keep_end` alone that lie behind its
 * four footer bytes (header fields that ran past the audio).  x, y: the item as the kernel reads it -- SPAN: file, first
 * frame; GENERAL: file (write) or row (read), index of a chunk of 2048 granules.  granule: bytes per vector of a GENERAL
 * item.  general != 0: the items of a call under vga_adx_files_force_general_this_thread(1).  items_out may be NULL (the
 * count alone); more than `capacity` items is VGA_ERR_ARGUMENT with the count in *count_out. */
#define VGA_ADX_FILES_HEADER 0
#define VGA_ADX_FILES_SPAN 1
#define VGA_ADX_FILES_GENERAL 2
#define VGA_ADX_FILES_FOOTER 3
typedef struct { int form, file, x; uint32_t y; int granule; int64_t begin, end, keep_end; } vga_adx_files_item;
int  vga_adx_files_write_items_for(const vga_adx_file *files, int nfiles, const int64_t *audio_offsets, int general,
                                   vga_adx_files_item *items_out, int64_t capacity, int64_t *count_out);
int  vga_adx_files_read_items_for(const vga_adx_file_info *const *infos, int nfiles, const int64_t *image_offsets, int general,
                                  vga_adx_files_item *items_out, int64_t capacity, int64_t *count_out);
/* out[0..3]: files in the span form, files in the general form (files that move no audio count in neither), span items,
 * general items -- of a call made by this thread now (the force hook applies) */
int  vga_adx_files_stats(const vga_adx_files *s, int64_t *out /*[4]*/);
/* per thread: the _v calls of this thread take the general form for every file.  Returns the previous value. */
int  vga_adx_files_force_general_this_thread(int on);

#ifdef __cplusplus
}
#endif
#endif
