/* vgaudio_hip/nw_files.h -- device-resident sets of NintendoWare stream FILES of different shapes: the BRSTM, BCSTM or BFSTM
 * image of every file of a set, written and read, in one set of launches per call.  The consumer of the rows
 * gc_files_aligned.h leaves: WAV set -> vga_gcadpcm_coefs_device_v -> vga_gcadpcm_encode_device_v ->
 * vga_gcadpcm_align_channels_device_v -> vga_nwstm_write_device_v never leaves HBM and issues no launch per file (with
 * BRSTM and the default configuration: the whole of VGAudio.Cli/Batch.cs), and neither does images ->
 * vga_nwstm_read_device_v -> vga_gcadpcm_decode_device_v.
 *
 * It lives next to gc_files.h / gc_files_aligned.h and outside the directory listing the older test files enumerate; the
 * same disciplines are applied to THIS header by tests/test_nw_files_host.py (exports, argument counts, the layout against a
 * model, the work tables, every refusal, and that the GPU file's table of cases names every function declared here) and
 * tests/test_gpu_nw_files.py (junk-filled buffers larger than needed, poison mode, a busy caller stream).
 *
 * A SET is nfiles files (vga_nw_file: channel count, sample rate, sample count and the format's loop, before the writer
 * aligns it) and ONE vga_nw_file_config for all of them, as VGAudio.Cli/Batch.cs applies one configuration to every file of
 * a folder; its fields mean what the fields of vga_nwstm_params of the same names mean, "0 = default" included.  File f's
 * vga_nwstm_params is the configuration plus the file's numbers, and everything about file f is what vga_nwstm_layout_for
 * says for those params.  The tracks of every file are the default list, AudioTrack.GetDefaultTrackList(channels); a
 * caller's own track list stays with the per-file call vga_nwstm_write_device.  The keep_* flags do not exist here.
 *
 * LAYOUT (vga_nw_files_layout_for computes it on the host, no GPU needed; an object carries the same numbers)
 *   inputs  lie exactly as gc_files_aligned.h leaves its OUTPUT: the channels of file f are rows first_channel[f] ..
 *           first_channel[f] + channels - 1 of a GC ragged batch over the files' layout.channel_sample_count
 *           (vga_nw_files_ragged; rows rounded to 16 bytes, a guard of 256 bytes behind the last); a row's ADPCM is
 *           layout.channel_adpcm_bytes bytes.  totals.adpcm_bytes / pcm_samples are the batch's sizes, guards included.
 *           Channel c's seek table is 2 * layout.channel_seek_entries shorts at seek_offsets[c] of one buffer of
 *           totals.seek_shorts; offsets are rounded up to 8 shorts.  Per-channel arrays (d_coefs: 16 shorts, d_gain: 1, the
 *           contexts: 3 each) are indexed by row.  vga_nw_files_gc_files fills the vga_gc_file array (channel =
 *           layout.channel) that vga_gc_aligned_create takes: that object's output rows and seek offsets are this one's
 *           inputs.  The set does not own or need the aligned object.
 *   images  File f's image is layout.file_size bytes at image_offsets[f] of one buffer of totals.image_bytes; offsets are
 *           rounded up to 16 bytes (every NW image size is a multiple of 0x20) and a guard of 256 bytes follows the last
 *           image (nothing writes it).
 *   d_adpcm, d_seek and d_images must be 16-byte aligned.  Anything less, or a null required buffer, is VGA_ERR_ARGUMENT
 *   before anything is launched.  nfiles == 0 is an empty set: every call returns 0 and launches nothing.
 *
 * REFUSED AT CREATE AND LAYOUT, the message naming the file ("file <f>: " in front of the per-file message), with the
 * per-file call's own code, because the check IS vga_nwstm_layout_for's code: whatever that call refuses for the file's
 * params (an unknown target, channels outside 1..255 VGA_ERR_ARGUMENT; an interleave not divisible by 14, a seek-table entry
 * below 2, loop points WithLoop rejects, a version the writer does not produce, a file past 2 GiB VGA_ERR_OUT_OF_RANGE);
 * more than 2^31 channels VGA_ERR_ARGUMENT; images of more than 2^62 bytes VGA_ERR_OUT_OF_RANGE.  A file of 0 samples is a
 * good file (vga_nwstm_write_device writes it: headers and an empty DATA block).
 *
 * A set made for writing refuses the read call and the other way round with VGA_ERR_INVALID_OP.
 *
 * All calls run on the caller's stream and never synchronise it; they need no workspace; the library allocates nothing per
 * call and writes nothing outside an image (write) or a row and a per-channel array (read): not the rounding gaps, not
 * the guards.  The object keeps its tables in the memory of the device that was current at create, is immutable and
 * serves any number of calls, concurrent calls on different streams included.
 *
 * LEFT OUT: sets of HPS and IDSP files, host-pointer forms of the _v calls, custom track lists in sets, the seek tables on the
 * read side (vga_nwstm_read delivers them per file).  PCM8 / PCM16 NintendoWare streams in sets are
 * ../vgaudio_hip_files/nw_pcm_files.h's. */
#ifndef VGAUDIO_HIP_NW_FILES_H
#define VGAUDIO_HIP_NW_FILES_H

#include "gc_files_aligned.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int channels;                          /* 1 .. VGA_NW_MAX_CHANNELS */
    int sample_rate;
    int sample_count;                      /* GcAdpcmFormat.SampleCount of the encoded channels */
    int looping, loop_start, loop_end;     /* the format's loop, before the writer aligns it */
} vga_nw_file;
typedef struct {                           /* BxstmConfiguration and the target: one per set */
    int target;                            /* VGA_NW_RSTM / CSTM / FSTM */
    int samples_per_interleave;            /* 0 = 14336; must be divisible by 14 */
    int samples_per_seek_table_entry;      /* 0 = 14336; at least 2 */
    int loop_point_alignment;              /* 0 = 14336 */
    int track_type, seek_table_type;       /* BRSTM only: VGA_NW_TRACK_*, VGA_NW_SEEK_* */
    uint32_t version;                      /* packed NwVersion; 0 = 2.1 (CSTM) / 0.3 (FSTM) */
    int endianness;                        /* -1 = the target's default; BRSTM is always big */
} vga_nw_file_config;
typedef struct {
    int files, channels;
    int64_t pcm_samples, adpcm_bytes;      /* = the GC ragged object's over channel_sample_count, guards included */
    int64_t seek_shorts;                   /* packed seek tables (a set for reading: 0) */
    int64_t image_bytes;                   /* packed images, guard included */
} vga_nw_files_totals;
typedef struct vga_nw_files vga_nw_files;

/* host only, needs no GPU.  first_channel_out / image_offsets_out: nfiles entries; seek_offsets_out: one per channel; any
 * output may be NULL, but not all of them. */
int  vga_nw_files_layout_for(const vga_nw_file *files, int nfiles, const vga_nw_file_config *config,
                             int *first_channel_out, int64_t *seek_offsets_out /* per channel */,
                             int64_t *image_offsets_out /* per file */, vga_nw_files_totals *totals_out);
/* the same checks, then the tables in the current device's memory */
int  vga_nw_files_create(const vga_nw_file *files, int nfiles, const vga_nw_file_config *config, vga_nw_files **out);
/* a set for READING, from what vga_nwstm_parse returned for every file.  The rows are over each header's sample_count
 * (info->adpcm_bytes bytes); image f is audio_data_offset + audio_data_length bytes at image_offsets[f] (any multiples of
 * 8), or packed as the writer packs.  The object uploads the parsed coefficients, gains and contexts once.  An info
 * vga_nwstm_read_device refuses (or whose adpcm_bytes is not its sample count's) is VGA_ERR_ARGUMENT, naming the file; a
 * file whose audio offset, interleave or bytes per channel is no multiple of 8 is VGA_ERR_INVALID_OP (no writer makes
 * one; vga_nwstm_read_device reads it). */
int  vga_nw_files_create_from_infos(const vga_nwstm_info *const *infos, int nfiles,
                                    const int64_t *image_offsets /* NULL: packed as the writer packs */, vga_nw_files **out);
void vga_nw_files_destroy(vga_nw_files *s);
int  vga_nw_files_totals_of(const vga_nw_files *s, vga_nw_files_totals *out);
int  vga_nw_files_offsets(const vga_nw_files *s, int *first_channel_out, int64_t *seek_offsets_out, int64_t *image_offsets_out);
/* out: totals.files entries, {channels, sample_rate, layout.channel} of every file: what vga_gc_aligned_create takes.  A
 * set for reading has no writer configuration: VGA_ERR_INVALID_OP. */
int  vga_nw_files_gc_files(const vga_nw_files *s, vga_gc_file *out);
/* borrowed; lives as long as s.  NULL for an empty set made where there is no device. */
const vga_gcadpcm_ragged *vga_nw_files_ragged(const vga_nw_files *s);

/* BrstmWriter.cs / BCFstmWriter.cs for every file: image f is byte for byte what vga_nwstm_write_device writes for that file
 * alone with tracks = NULL, the NULL-pointer defaults of that call included (d_gain NULL: 0; d_start_context NULL: (the
 * row's first byte -- 0 for a row of no bytes --, 0, 0); d_loop_context NULL: zeros; a file that does not loop carries its
 * start context as loop context).  d_seek: the packed tables, NULL only if no file has entries.  Every byte of every image
 * is written by the three kernels (headers, seek tables, audio); there is no memset, and no byte between two images,
 * behind the last image or in the guard is written. */
int  vga_nwstm_write_device_v(const vga_nw_files *s, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *d_gain,
                              const int16_t *d_start_context, const int16_t *d_loop_context, const int16_t *d_seek,
                              uint8_t *d_images, void *stream);
/* The bytes vga_nwstm_read_device delivers for every file, into the rows of the ragged layout (row bytes no block supplies
 * are zero, nothing is written behind a row's end); the per-channel outputs that are not NULL get what the infos hold
 * (d_gain of a BCSTM / BFSTM: 0), so vga_gcadpcm_decode_device_v on vga_nw_files_ragged(s) can follow without a host round
 * trip.  The set is one from vga_nw_files_create_from_infos. */
int  vga_nwstm_read_device_v(const vga_nw_files *s, const uint8_t *d_images, uint8_t *d_adpcm, int16_t *d_coefs,
                             int16_t *d_gain, int16_t *d_start_context, int16_t *d_loop_context, void *stream);

#ifdef __cplusplus
}
#endif
#endif
