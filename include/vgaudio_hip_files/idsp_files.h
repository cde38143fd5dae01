/* vgaudio_hip_files/idsp_files.h -- device-resident sets of IDSP FILES of different shapes: the IDSP image of every file of a
 * set, written and read, in one set of launches per call.  A consumer of the rows gc_files_aligned.h leaves: WAV set ->
 * vga_gcadpcm_coefs_device_v -> vga_gcadpcm_encode_device_v -> vga_gcadpcm_align_channels_device_v -> vga_idsp_write_device_v
 * never leaves HBM and issues no launch per file, and neither does images -> vga_idsp_read_device_v ->
 * vga_gcadpcm_decode_device_v.  The scaffolding is nw_files.h's.
 *
 * It lives in the directory of wave_files.h, outside the listings the older test files enumerate; the same disciplines are
 * applied to THIS header by tests/test_idsp_files_host.py (exports, argument counts, the layout against a model, the regions
 * the kernels write, every refusal, and that the GPU file's table of cases names every function declared here) and
 * tests/test_gpu_idsp_files.py (junk-filled buffers larger than needed, poison mode, a busy caller stream, two streams at
 * once).  The hooks of this feature are declared here too, at the end.
 *
 * A SET is nfiles files (vga_idsp_file: channel count, sample rate, sample count and the format's loop, before the writer
 * aligns it) and ONE vga_idsp_file_config for all of them, as VGAudio.Cli/Batch.cs applies one configuration to every file of
 * a folder; its fields mean what the fields of vga_idsp_params of the same names mean (block_size 0x10 is the reference's
 * default, 0 = not interleaved).  File f's vga_idsp_params is the configuration plus the file's numbers, and everything about
 * file f is what vga_idsp_layout_for says for those params.
 *
 * LAYOUT (vga_idsp_files_layout_for computes it on the host, no GPU needed; an object carries the same numbers)
 *   inputs  lie exactly as gc_files_aligned.h leaves its OUTPUT: the channels of file f are rows first_channel[f] ..
 *           first_channel[f] + channels - 1 of a GC ragged batch over the files' layout.channel_sample_count
 *           (vga_idsp_files_ragged; rows rounded to 16 bytes, a guard of 256 bytes behind the last); a row's ADPCM is
 *           layout.channel_adpcm_bytes bytes.  totals.adpcm_bytes / pcm_samples are the batch's sizes, guards included.
 *           Per-channel arrays (d_coefs: 16 shorts, d_gain: 1, the contexts: 3 each) are indexed by row.
 *           vga_idsp_files_gc_files fills the vga_gc_file array (channel = layout.channel: the loop alignment multiple is
 *           ByteCountToSampleCount(block_size)) that vga_gc_aligned_create takes: that object's output rows are this one's
 *           inputs.  The set does not own or need the aligned object.
 *   images  File f's image is layout.file_size bytes at image_offsets[f] of one buffer of totals.image_bytes; offsets are
 *           rounded up to 16 bytes (an IDSP header is 0x40 + 0x60 * channels bytes and the audio a multiple of 8, so sizes
 *           are multiples of 8 only) and a guard of 256 bytes follows the last image (nothing writes it).
 *   d_adpcm and d_images must be 16-byte aligned.  Anything less, or a null required buffer, is VGA_ERR_ARGUMENT before
 *   anything is launched.  nfiles == 0 is an empty set: every call returns 0 and launches nothing.
 *
 * REFUSED AT CREATE AND LAYOUT, the message naming the file ("file <f>: " in front of the per-file message), with the
 * per-file call's own code, because the check IS vga_idsp_layout_for's code (gc_stream_host.hpp): whatever that call refuses
 * for the file's params (no channel VGA_ERR_ARGUMENT; more than 255 channels VGA_ERR_INVALID_OP; a block size that is negative
 * or not divisible by 8, loop points WithLoop rejects, a file past 2 GiB VGA_ERR_OUT_OF_RANGE; block size 0 with no audio
 * VGA_ERR_INVALID_OP); more than 2^31 rows VGA_ERR_ARGUMENT; images of more than 2^62 bytes VGA_ERR_OUT_OF_RANGE.  A file of 0
 * samples with a block size is a good file (a header and no audio).
 *
 * A set made for writing refuses the read call and the other way round with VGA_ERR_INVALID_OP.
 *
 * LAUNCHES.  A write is at most TWO launches whatever nfiles is: the headers (one workgroup per file, every byte of the
 * 0x40 + 0x60 * channels header), then Interleave(rows, interleave_size, audio_data_size) of every file over (file, chunk)
 * work items cut on the host, none outside its image, the zero padding of short rows and of the last block written by the
 * item that owns it.  A read is at most TWO as well: the parsed per-channel arrays (only if one is asked for), then
 * DeInterleave over (row, chunk) items.  A launch without items is not made.  There is no memset: every byte of every image
 * is written exactly once by these kernels, and no byte between two images, behind the last image or in the guard is.
 * GRANULES.  The audio of an image starts on 16 bytes (the header is a multiple of 0x20 and the image offset one of 16), so
 * a written file moves as 16-byte vectors where its interleave -- and the rows of its last block -- are multiples of 16
 * (every block size that is one, the default 0x10 included), and as 8-byte vectors otherwise (block size 8, or block size
 * 0 with an odd number of frames).  A file read moves 16-byte vectors where its audio's address, its interleave and its
 * bytes per channel are multiples of 16, 8-byte vectors where they are multiples of 8, and single bytes otherwise (the
 * GENERAL form: foreign files are not refused, whatever vga_idsp_read_device reads the set reads).
 *
 * All calls run on the caller's stream and never synchronise it; they need no workspace; the library allocates nothing per
 * call and writes nothing outside an image (write) or a row and a per-channel array (read): not the rounding gaps, not
 * the guards.  The object keeps its tables in the memory of the device that was current at create, is immutable and
 * serves any number of calls, concurrent calls on different streams included.
 *
 * LEFT OUT: host-pointer forms of the _v calls.  (Sets of HPS files are hps_files.h, next to this header.) */
#ifndef VGAUDIO_HIP_FILES_IDSP_FILES_H
#define VGAUDIO_HIP_FILES_IDSP_FILES_H

#include "../vgaudio_hip/gc_files_aligned.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int channels;                          /* 1 .. VGA_GC_CONTAINER_MAX_CHANNELS */
    int sample_rate;
    int sample_count;                      /* the format's UnalignedSampleCount */
    int looping, loop_start, loop_end;     /* the format's loop, before the writer aligns it */
} vga_idsp_file;
typedef struct {                           /* IdspConfiguration: one per set */
    int block_size;                        /* BlockSize: 0 = not interleaved, else a multiple of 8; the reference's default is 0x10 */
    int trim_file;                         /* Configuration.TrimFile */
} vga_idsp_file_config;
typedef struct {
    int files, channels;
    int64_t pcm_samples, adpcm_bytes;      /* = the GC ragged object's over channel_sample_count, guards included */
    int64_t image_bytes;                   /* packed images, guard included */
} vga_idsp_files_totals;
typedef struct vga_idsp_files vga_idsp_files;

/* host only, needs no GPU.  first_channel_out / image_offsets_out: nfiles entries; any output may be NULL, but not all of
 * them. */
int  vga_idsp_files_layout_for(const vga_idsp_file *files, int nfiles, const vga_idsp_file_config *config,
                               int *first_channel_out, int64_t *image_offsets_out /* per file */,
                               vga_idsp_files_totals *totals_out);
/* the same checks, then the tables in the current device's memory */
int  vga_idsp_files_create(const vga_idsp_file *files, int nfiles, const vga_idsp_file_config *config, vga_idsp_files **out);
/* a set for READING, from what vga_idsp_parse returned for every file.  The rows are over each header's sample_count
 * (info->adpcm_bytes bytes); image f is audio_data_offset + channel_count * audio_data_length bytes at image_offsets[f] --
 * ANY byte offset that is not negative (IDSP files inside archives do not start aligned; images that overlap are the
 * caller's business, they are only read) --, or packed as the writer packs.  The object uploads the parsed coefficients,
 * gains and contexts once.  An info vga_idsp_read_device refuses is refused by that call's own check (gc_stream_host.hpp), with
 * its code and its message behind "file <f>: "; one whose adpcm_bytes is not its sample count's, or whose audio offset is
 * negative, is VGA_ERR_ARGUMENT, naming the file. */
int  vga_idsp_files_create_from_infos(const vga_idsp_info *const *infos, int nfiles,
                                      const int64_t *image_offsets /* NULL: packed as the writer packs */, vga_idsp_files **out);
void vga_idsp_files_destroy(vga_idsp_files *s);
int  vga_idsp_files_totals_of(const vga_idsp_files *s, vga_idsp_files_totals *out);
int  vga_idsp_files_offsets(const vga_idsp_files *s, int *first_channel_out, int64_t *image_offsets_out);
/* out: totals.files entries, {channels, sample_rate, layout.channel} of every file: what vga_gc_aligned_create takes.  A
 * set for reading has no writer configuration: VGA_ERR_INVALID_OP. */
int  vga_idsp_files_gc_files(const vga_idsp_files *s, vga_gc_file *out);
/* borrowed; lives as long as s.  NULL for an empty set made where there is no device. */
const vga_gcadpcm_ragged *vga_idsp_files_ragged(const vga_idsp_files *s);

/* IdspWriter.cs for every file: image f is byte for byte what vga_idsp_write_device writes for that file alone from rows of
 * layout.channel_adpcm_bytes bytes, the NULL-pointer defaults of that call included (d_gain NULL: 0; d_start_context NULL:
 * (the row's first byte -- 0 for a row of no bytes --, 0, 0); d_loop_context NULL: zeros). */
int  vga_idsp_write_device_v(const vga_idsp_files *s, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *d_gain,
                             const int16_t *d_start_context, const int16_t *d_loop_context, uint8_t *d_images, void *stream);
/* The bytes vga_idsp_read_device delivers for every file, into the rows of the ragged layout (row bytes no block supplies
 * are zero, nothing is written behind a row's end); the per-channel outputs that are not NULL get what the infos hold, so
 * vga_gcadpcm_decode_device_v on vga_idsp_files_ragged(s) can follow without a host round trip.  The set is one from
 * vga_idsp_files_create_from_infos. */
int  vga_idsp_read_device_v(const vga_idsp_files *s, const uint8_t *d_images, uint8_t *d_adpcm, int16_t *d_coefs,
                            int16_t *d_gain, int16_t *d_start_context, int16_t *d_loop_context, void *stream);

/* ---- hooks of this feature (tests and tools)
 * The regions a call's kernels write, host only (no GPU), computed from the work tables a set of these arguments holds, in
 * launch order.  kernel: VGA_IDSP_FILES_HEADER (write: one per file) or VGA_IDSP_FILES_AUDIO (one per work item).  index:
 * the file (write) or the row (read).  begin / end: the bytes written, counted from the start of the file's image (write) or
 * of the row (read).  granule: 16, 8 or 1, the vector the item moves (0: the header).  regions_out may be NULL (the count
 * alone); more than `capacity` regions is VGA_ERR_ARGUMENT with the count in *count_out. */
#define VGA_IDSP_FILES_HEADER 0
#define VGA_IDSP_FILES_AUDIO 1
typedef struct { int kernel, index, granule; int64_t begin, end; } vga_idsp_files_region;
int  vga_idsp_files_write_regions_for(const vga_idsp_file *files, int nfiles, const vga_idsp_file_config *config,
                                      vga_idsp_files_region *regions_out, int64_t capacity, int64_t *count_out);
int  vga_idsp_files_read_regions_for(const vga_idsp_info *const *infos, int nfiles, const int64_t *image_offsets,
                                     vga_idsp_files_region *regions_out, int64_t capacity, int64_t *count_out);
/* out[0..3]: the audio work items, those of 16-byte granules, the bytes of the object's device tables, the kernels the last
 * _v call of THIS thread on any vga_idsp_files launched (0 after a refused call or one on an empty set) */
int  vga_idsp_files_stats(const vga_idsp_files *s, int64_t *out /*[4]*/);

#ifdef __cplusplus
}
#endif
#endif
