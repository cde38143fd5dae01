/* vgaudio_hip/gc_files_aligned.h -- device-resident sets of GC-ADPCM FILES whose loop starts need the GcAdpcmAlignment.cs
 * re-encode: the aligned ADPCM, the aligned PCM, the seek table and the loop context of every channel of every file, in one
 * set of launches per call.  gc_files.h refuses such a file at create (its DSP images never need the re-encode); the
 * NintendoWare writers do (BxstmConfiguration.LoopPointAlignment defaults to 14 336), and this header is the ragged form of
 * what vga_gcadpcm_build_channels_device does for one file: WAV set -> vga_gcadpcm_coefs_device_v ->
 * vga_gcadpcm_encode_device_v -> vga_gcadpcm_align_channels_device_v never leaves HBM and issues no launch per file.
 *
 * It lives next to gc_files.h and outside the directory listing the older test files enumerate; the same disciplines are
 * applied to THIS header by tests/test_gc_aligned_host.py (exports, argument counts, the layout against a model, the
 * per-channel numbers against GcAdpcmAlignment.cs:29-39, every refusal, and that the GPU file's table of cases names every
 * function declared here) and tests/test_gpu_gc_aligned.py (junk-filled buffers larger than needed, poison mode, a busy
 * caller stream).
 *
 * A SET is nfiles files (vga_gc_file of gc_files.h, used here without a DSP configuration); file f has its own channel
 * count, sample count, loop, alignment multiple and seek spacing.  A caller who writes NW streams fills `channel` from
 * vga_nwstm_layout_for(...).channel per file.
 *
 * LAYOUT (vga_gc_aligned_layout_for computes it on the host, no GPU needed; an object carries the same numbers)
 *   input   The channels of file f are rows first_channel[f] .. first_channel[f] + channels - 1 of a GC ragged batch over
 *           the files' sample_count (vga_gc_aligned_ragged_in; exactly gc_files.h's rows): what the _device_v codec calls
 *           read and wrote.  totals.pcm_samples / adpcm_bytes are its sizes, guards included.
 *   output  The same rows of a second GC ragged batch over the files' sample_count_aligned
 *           (vga_gcadpcm_channel_layout_for; vga_gc_aligned_ragged_out): totals.out_pcm_samples / out_adpcm_bytes.  A row's
 *           ADPCM is SampleCountToByteCount(sample_count_aligned) bytes.  When no file needs alignment the two batches are
 *           the same layout.  A file's rows are one pitch apart (every row of a file has the same length), so they go to
 *           the per-file container writers as (base, pitch) unchanged.
 *   seek    Channel c's table is 2 * seek_table_entries shorts (entries from sample_count_aligned) at seek_offsets[c] of one
 *           buffer of totals.seek_shorts; offsets are rounded up to 8 shorts, a channel without entries takes no room.
 *   d_adpcm, d_adpcm_out, d_pcm_out, d_seek_out and the workspace must be 16-byte aligned.  Anything less, a null required
 *   buffer (d_adpcm, d_coefs, d_adpcm_out) or a short workspace is VGA_ERR_ARGUMENT before anything is launched.
 *   nfiles == 0 is an empty set: every call returns 0 and launches nothing.  Per-channel arrays (d_coefs: 16 shorts, the
 *   contexts: 3 each) are indexed by row.
 *   workspace   totals.workspace_bytes is everything a call can need: the plain decode of the input batch, the tails to
 *           encode (PCM, ADPCM, their coefficients and histories) and the encoder's time-piece states.  A set in which no
 *           file needs alignment needs the plain decode only, and not even that when d_pcm_out is given or nothing reads
 *           the PCM; then the workspace may be NULL.
 *
 * REFUSED AT CREATE AND LAYOUT, the message naming the file ("file <f>: ..."), with the per-file call's own code:
 *   what gc_files.h refuses without a configuration (channels < 1 VGA_ERR_ARGUMENT, channels > VGA_DSP_MAX_CHANNELS
 *   VGA_ERR_INVALID_OP, what vga_gcadpcm_channel_layout_for refuses VGA_ERR_OUT_OF_RANGE); a zero-length loop that needs
 *   alignment VGA_ERR_INVALID_OP (the reference's fill loop never ends); a file that needs alignment whose loop_end lies
 *   past sample_count VGA_ERR_OUT_OF_RANGE (the row does not hold the loop: the reference's decode of loopEnd samples runs
 *   past Adpcm, GcAdpcmAlignment.cs:41-42).
 * REFUSED AT THE CALL: with d_loop_context_out, a file whose ALIGNED loop start lies past its ORIGINAL data is
 *   VGA_ERR_OUT_OF_RANGE, naming the file, before anything is launched (the context's pred/scale byte is read from the
 *   original stream, GcAdpcmChannelBuilder.cs:179); with a NULL context the same set runs.
 *
 * All calls run on the caller's stream and never synchronise it; all scratch is the caller's workspace; the library
 * allocates nothing per call and writes nothing outside a row of the output batch, a seek table, a context or the
 * workspace (not the rounding gaps, not the guards).  The object keeps its tables in the memory of the device that was
 * current at create, is immutable and serves any number of calls, concurrent calls on different streams (each with a
 * workspace of its own) included. */
#ifndef VGAUDIO_HIP_GC_FILES_ALIGNED_H
#define VGAUDIO_HIP_GC_FILES_ALIGNED_H

#include "gc_files.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int files, channels, aligned_channels;        /* channels of files whose alignment_needed is set */
    int64_t pcm_samples, adpcm_bytes;             /* INPUT rows: the ragged batch over sample_count (as gc_files.h) */
    int64_t out_pcm_samples, out_adpcm_bytes;     /* OUTPUT rows: the ragged batch over sample_count_aligned, guards included */
    int64_t seek_shorts;                          /* packed seek tables, entries from sample_count_aligned */
    size_t  workspace_bytes;                      /* everything the call needs, the encoder's scratch included */
} vga_gc_aligned_totals;
typedef struct vga_gc_aligned vga_gc_aligned;

/* host only, needs no GPU.  first_channel_out: nfiles entries; seek_offsets_out: one per channel; any output may be NULL,
 * but not all of them. */
int  vga_gc_aligned_layout_for(const vga_gc_file *files, int nfiles, int *first_channel_out,
                               int64_t *seek_offsets_out /* per channel */, vga_gc_aligned_totals *totals_out);
/* the same checks, then the work tables in the current device's memory */
int  vga_gc_aligned_create(const vga_gc_file *files, int nfiles, vga_gc_aligned **out);
void vga_gc_aligned_destroy(vga_gc_aligned *s);
int  vga_gc_aligned_totals_of(const vga_gc_aligned *s, vga_gc_aligned_totals *out);
int  vga_gc_aligned_offsets(const vga_gc_aligned *s, int *first_channel_out, int64_t *seek_offsets_out);
/* borrowed; live as long as s.  NULL for an empty set made where there is no device. */
const vga_gcadpcm_ragged *vga_gc_aligned_ragged_in(const vga_gc_aligned *s);    /* rows of sample_count: what the _device_v codec calls wrote */
const vga_gcadpcm_ragged *vga_gc_aligned_ragged_out(const vga_gc_aligned *s);   /* rows of sample_count_aligned */

/* GcAdpcmChannel(GcAdpcmChannelBuilder) for every channel of every file, byte for byte what one
 * vga_gcadpcm_build_channels_device call on that file alone writes: d_adpcm_out gets SampleCountToByteCount(
 * sample_count_aligned) bytes per row of the OUTPUT batch, d_pcm_out sample_count_aligned shorts, d_seek_out the seek
 * tables, d_loop_context_out three shorts per channel (aligned loop start 0: zeros).  A file that needs no alignment gets its
 * input row copied; one that needs it goes through GcAdpcmAlignment.cs:33-62 (keep loop_end / 14 frames, gather the tail --
 * the rest of the last kept-from frame, then the loop wrapped --, encode it with the history of the last two kept samples,
 * decode it again from samples_to_keep on).  d_status is handed to the decode of the input batch as is. */
int  vga_gcadpcm_align_channels_device_v(const vga_gc_aligned *s, const uint8_t *d_adpcm, const int16_t *d_coefs,
                                         uint8_t *d_adpcm_out, int16_t *d_pcm_out /* or NULL */,
                                         int16_t *d_seek_out /* or NULL */, int16_t *d_loop_context_out /* channels*3, or NULL */,
                                         int *d_status, void *d_workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
