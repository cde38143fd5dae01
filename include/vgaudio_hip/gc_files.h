/* vgaudio_hip/gc_files.h -- device-resident sets of GC-ADPCM FILES of different shapes: the GcAdpcmChannel metadata (loop
 * context, seek table) of every file and every file's DSP image, written and read, in one set of launches per call.  The
 * last stage of the ragged GC-ADPCM route of ../vgaudio_hip.h: WAV set -> vga_gcadpcm_encode_device_v ->
 * vga_gcadpcm_build_channels_device_v -> vga_dsp_write_device_v never leaves HBM and issues no launch per file, and neither
 * does DSP images -> vga_dsp_read_device_v -> vga_gcadpcm_decode_device_v.
 *
 * This header lives one directory below the drop-in header for the reason adx_ragged.h gives: the test files that hold
 * every function of include/ itself to the export, dirty-memory, busy-stream and loosest-layout checks enumerate the
 * top-level headers and carry their own tables of cases.  The same disciplines are applied to THIS header by
 * tests/test_gc_files_host.py (exports, argument counts, the layout against a model, the work tables, every refusal, and that
 * the GPU file's table of cases names every function declared here) and tests/test_gpu_gc_files.py (junk-filled buffers
 * larger than needed, poison mode, a busy caller stream).
 *
 * A SET is nfiles files; file f has its own channel count, sample rate, sample count, loop and seek spacing
 * (vga_gc_file), and ONE vga_dsp_file_config applies to all of them, as VGAudio.Cli/Batch.cs applies one configuration to
 * every file of a folder.  Without a config (NULL) the set has no images and serves vga_gcadpcm_build_channels_device_v only.
 *
 * LAYOUT (vga_gc_files_layout_for computes it on the host, no GPU needed; an object carries the same numbers)
 *   rows    The channels of file f are rows first_channel[f] .. first_channel[f] + channels - 1 of a GC ragged batch
 *           (vga_gcadpcm_ragged_create over the files' sample counts, each repeated per channel): every row of a file has
 *           that file's sample count.  vga_gc_files_ragged returns that batch, so the _device_v codec calls take the same
 *           packed d_pcm and d_adpcm unchanged; totals.pcm_samples / adpcm_bytes are its sizes, guards included.  A row's
 *           ADPCM is SampleCountToByteCount(sample_count) bytes.
 *   seek    Channel c's table is 2 * seek_table_entries shorts at seek_offsets[c] of one buffer of totals.seek_shorts;
 *           offsets are rounded up to 8 shorts, a channel without entries takes no room.
 *   images  File f's image is vga_dsp_layout_for(...).file_size bytes at image_offsets[f] of one buffer of
 *           totals.image_bytes; offsets are rounded up to 16 bytes and a guard of 256 bytes follows the last image (loads
 *           may touch it, nothing writes it).
 *   d_adpcm, d_pcm, d_images, d_seek_out and the workspace must be 16-byte aligned.  Anything less, a null required buffer or
 *   a short workspace is VGA_ERR_ARGUMENT before anything is launched.  nfiles == 0 is an empty set: every call returns 0
 *   and launches nothing.  Per-channel arrays (d_coefs: 16 shorts, d_gain: 1, the contexts: 3 each) are indexed by row.
 *
 * REFUSED AT CREATE, the message naming the file ("file <f>: ..."), with the per-file call's own code:
 *   channels < 1 VGA_ERR_ARGUMENT, channels > VGA_DSP_MAX_CHANNELS VGA_ERR_INVALID_OP; what
 *   vga_gcadpcm_channel_layout_for refuses (VGA_ERR_OUT_OF_RANGE); what vga_dsp_layout_for refuses (VGA_ERR_OUT_OF_RANGE:
 *   an interleave not divisible by 14); a mono file whose header sample count needs more bytes than its row has
 *   (VGA_ERR_ARGUMENT, as vga_dsp_write_device).
 *   A file whose vga_gcadpcm_channel_layout_for says alignment_needed is VGA_ERR_INVALID_OP: the GcAdpcmAlignment.cs
 *   re-encode is not done in ragged form; that file goes through vga_gcadpcm_build_channels_device.  DSP never needs it:
 *   DspWriter's LoopPointAlignment only shifts header numbers (DspWriter.cs:29-31).
 *
 * All calls run on the caller's stream and never synchronise it; all scratch is the caller's workspace; the library
 * allocates nothing per call and writes nothing outside a row, a table or an image (not the rounding gaps, not the guards).
 * The object keeps its tables in the memory of the device that was current at create, is immutable and serves any number
 * of calls, concurrent calls on different streams (each with a workspace of its own) included. */
#ifndef VGAUDIO_HIP_GC_FILES_H
#define VGAUDIO_HIP_GC_FILES_H

#include "../vgaudio_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int channels;                          /* 1 .. VGA_DSP_MAX_CHANNELS */
    int sample_rate;
    vga_gcadpcm_channel_params channel;    /* this FILE's sample count, loop, alignment multiple, seek spacing */
} vga_gc_file;
typedef struct {                           /* DspConfiguration: one per set, as Batch.cs applies one to all files */
    int samples_per_interleave, loop_point_alignment, trim_file;
} vga_dsp_file_config;
typedef struct {
    int files, channels;
    int64_t pcm_samples, adpcm_bytes;      /* = the GC ragged object's, guards included */
    int64_t seek_shorts;                   /* packed seek tables */
    int64_t image_bytes;                   /* packed DSP images, guard included; 0 without a config */
    size_t  build_workspace_bytes;         /* the decoded PCM when the caller does not take it: pcm_samples * 2 */
} vga_gc_files_totals;
typedef struct vga_gc_files vga_gc_files;

/* host only, needs no GPU.  first_channel_out / image_offsets_out: nfiles entries; seek_offsets_out: one per channel; any
 * output may be NULL, but not all of them.  image_offsets_out is left alone without a config. */
int  vga_gc_files_layout_for(const vga_gc_file *files, int nfiles, const vga_dsp_file_config *dsp /* or NULL */,
                             int *first_channel_out, int64_t *seek_offsets_out /* per channel */,
                             int64_t *image_offsets_out /* per file */, vga_gc_files_totals *totals_out);
/* the same checks, then the work tables in the current device's memory */
int  vga_gc_files_create(const vga_gc_file *files, int nfiles, const vga_dsp_file_config *dsp, vga_gc_files **out);
/* a set for READING, from what vga_dsp_parse returned for every file: each file with its own channel count, sample count
 * (the header's: the rows' length) and frames per interleave.  Image f is audio_offset + data_length bytes at
 * image_offsets[f] (any multiple of 8), or packed as the writer packs.  Such a set carries no loop, no seek table and no
 * writer configuration (vga_dsp_write_device_v on it is VGA_ERR_INVALID_OP); the contexts come out of the headers.  An info
 * vga_dsp_read_device refuses is VGA_ERR_ARGUMENT. */
int  vga_gc_files_create_from_dsp(const vga_dsp_info *const *infos, int nfiles,
                                  const int64_t *image_offsets /* NULL: packed as the writer packs */, vga_gc_files **out);
void vga_gc_files_destroy(vga_gc_files *s);
int  vga_gc_files_totals_of(const vga_gc_files *s, vga_gc_files_totals *out);
int  vga_gc_files_offsets(const vga_gc_files *s, int *first_channel_out, int64_t *seek_offsets_out, int64_t *image_offsets_out);
/* borrowed; lives as long as s.  NULL for an empty set made where there is no device. */
const vga_gcadpcm_ragged *vga_gc_files_ragged(const vga_gc_files *s);

/* GcAdpcmChannel(GcAdpcmChannelBuilder) for every channel of every file: what one vga_gcadpcm_build_channels_device call on
 * that file alone writes -- the decoded PCM (into d_pcm_out, or into the workspace: totals.build_workspace_bytes), the seek
 * table, the three shorts of the loop context (loop start 0: zeros).  The PCM is vga_gcadpcm_decode_device_v's on the set's
 * ragged batch, d_status handed to it as is; when no seek table is wanted and no loop start is non-zero the decode is
 * skipped, as the per-file call skips it, and the workspace may be NULL.  VGA_ERR_OUT_OF_RANGE, naming the file, when a
 * loop context is asked for and a file's loop start lies past its data (as the per-file call). */
int  vga_gcadpcm_build_channels_device_v(const vga_gc_files *s, const uint8_t *d_adpcm, const int16_t *d_coefs,
                                         int16_t *d_pcm_out /* or NULL */, int16_t *d_seek_out /* or NULL */,
                                         int16_t *d_loop_context_out /* channels*3, or NULL */, int *d_status,
                                         void *d_workspace, size_t workspace_bytes, void *stream);
/* DspWriter.cs:17-103 for every file: image f is byte for byte what vga_dsp_write_device writes for that file.  d_gain NULL:
 * 0; d_start_context NULL: (the row's first byte -- 0 for a row of no bytes --, 0, 0); d_loop_context NULL or a file that
 * does not loop: zeros.  Every byte of every image is written by the two kernels (headers, audio); there is no memset. */
int  vga_dsp_write_device_v(const vga_gc_files *s, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *d_gain,
                            const int16_t *d_start_context, const int16_t *d_loop_context, uint8_t *d_images, void *stream);
/* DspReader.cs:103-115 for every image: the bytes vga_dsp_read_device delivers, into the rows of the ragged layout (row
 * bytes no block supplies are zero); the per-channel outputs that are not NULL are read big-endian from the headers on the
 * device, as vga_dsp_info holds them.  The set is one from vga_gc_files_create_from_dsp (a header's sample count, which
 * sizes the rows read into, need not be the one its file was written from); any other is VGA_ERR_INVALID_OP. */
int  vga_dsp_read_device_v(const vga_gc_files *s, const uint8_t *d_images, uint8_t *d_adpcm, int16_t *d_coefs,
                           int16_t *d_gain, int16_t *d_start_context, int16_t *d_loop_context, void *stream);

#ifdef __cplusplus
}
#endif
#endif
