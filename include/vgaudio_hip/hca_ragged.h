/* vgaudio_hip/hca_ragged.h -- device-resident CRI HCA batches of streams of DIFFERENT lengths: packed frames, packed
 * PCM, one set of launches per call (the HCA counterpart of vga_gcadpcm_ragged_create and the *_device_v calls of
 * ../vgaudio_hip.h).
 *
 * This header lives one directory below the drop-in header on purpose.  The test files that hold every function of
 * include/ itself to the export check, the dirty-memory check, the busy-stream check and the loosest-layout check enumerate the
 * top-level headers and carry their own tables of cases; a function declared here is outside those lists.  The same four
 * disciplines are applied to THIS header by tests/test_hca_ragged_device_host.py (exports, argument counts, and that the
 * GPU file's table of cases names every function declared here) and tests/test_gpu_hca_ragged_device.py (junk-filled
 * buffers larger than needed, poison mode, a busy caller stream, refused layouts).  Test hooks stay in
 * ../vgaudio_hip_testing.h (vga_testing_hca_ragged_stats).
 *
 * LAYOUT (vga_hca_ragged_layout_for computes it on the host, no GPU needed; an object carries the same numbers)
 *   frames  stream s's frames lie back to back at d_frames + frame_offsets[s] (bytes).  Offsets ascend in stream order;
 *           each is frame_count * frame_size past the one before, rounded up to 4.  totals.frame_bytes is the end of the
 *           last stream rounded up to 4 plus 8 bytes of slack whose content does not matter (the decoder's loads may
 *           touch them; nothing writes them).  d_frames must be 4-byte aligned.
 *   PCM     rows are stream-major: stream 0 channel 0, stream 0 channel 1, ..., stream 1 channel 0, ...  Row i starts at
 *           d_pcm + pcm_row_offsets[i] (samples) and is its stream's sample_count long; rows follow each other rounded up
 *           to 8 samples, totals.pcm_samples is the end of the last.  d_pcm must be 16-byte aligned, and so must the
 *           decoder's d_workspace.
 *   A stream with frame_count == 0 takes no room among the frames and one with sample_count == 0 none among the rows (its
 *   offsets equal the next stream's); the decoder's second kernel launches nothing for either, and the encoder writes the
 *   frames a stream of no samples still has (CriHcaEncoder.Initialize gives it one).
 *   Anything less than the alignments above, or a workspace smaller than totals.decode_workspace_bytes, is
 *   VGA_ERR_ARGUMENT before anything is launched.
 *
 * ONE SHAPE CLASS PER OBJECT.  All streams must agree in what the kernels are compiled data for: channel count, frame
 * size, band counts, channel types, ATH curve -- the rule vga_hca_decode_batch_v sorts by (vga_testing_hca_decode_classes
 * reports it): frame_count, sample_count and inserted_samples are free, and so are the loop fields, header_size and
 * comment_length, so looping streams decode beside plain ones.  A stream of a second class -> VGA_ERR_ARGUMENT, the
 * message names the first such stream; callers with several classes make one object per class.  An HcaInfo that
 * vga_hca_decode_device refuses is refused here with the same code.
 *
 * DECODE  bit for bit what one vga_hca_decode_device call per stream writes.  d_status has one int PER STREAM: stream s's
 * own flag bits are OR-ed into d_status[s] (the bits of vga_hca_decode_device: 1 invalid sync word, 2 scale-factor delta
 * out of range, 32 intensity 15; the caller zeroes the array and reads it after its stream), so a bad frame marks its own
 * stream only and the call still returns 0.  Nothing is written outside a stream's own rows: not the rounding gaps, not
 * the slack, not d_frames.
 * ENCODE  streams that do not loop: the bytes of one vga_hca_encode_device call per stream with that stream's sample_count
 * as pcm_length; d_status[s] as there (4 bitrate too low, 8, 16).  An object that holds a looping stream gives
 * VGA_ERR_INVALID_OP from THIS encode call and is still good for decoding; vga_hca_encode_loops_device_v of
 * ../vgaudio_hip_files/hca_ragged_loops.h encodes such an object, looping streams beside plain ones, in the same launches.
 *
 * Both calls run on the caller's stream and never synchronise it; d_workspace is the caller's, the library allocates
 * nothing per call.  The object keeps its tables in the memory of the device that was current at create, is immutable and
 * may serve any number of calls, concurrent calls on different streams (each with a workspace of its own) included. */
#ifndef VGAUDIO_HIP_HCA_RAGGED_H
#define VGAUDIO_HIP_HCA_RAGGED_H

#include "../vgaudio_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vga_hca_ragged vga_hca_ragged;
typedef struct {
    int64_t frame_bytes, pcm_samples; /* sizes of the two packed buffers (bytes with the slack; samples) */
    int rows, total_frames;           /* sum of channel_count; sum of frame_count */
    size_t decode_workspace_bytes;
} vga_hca_ragged_totals;

/* host only, needs no GPU: the packed layout for nstreams streams of ONE shape class.  frame_offsets_out: nstreams entries,
 * pcm_row_offsets_out: sum of channel_count entries; either may be NULL, totals_out too, but not all three.  nstreams == 0
 * is an empty batch (8 bytes of frames, no PCM). */
int vga_hca_ragged_layout_for(const vga_hca_info *infos, int nstreams, int64_t *frame_offsets_out,
                              int64_t *pcm_row_offsets_out, vga_hca_ragged_totals *totals_out);
/* the same checks, then the kernels' tables in the current device's memory */
int vga_hca_ragged_create(const vga_hca_info *infos, int nstreams, vga_hca_ragged **out);
void vga_hca_ragged_destroy(vga_hca_ragged *r);
int vga_hca_ragged_streams(const vga_hca_ragged *r);
int vga_hca_ragged_totals_of(const vga_hca_ragged *r, vga_hca_ragged_totals *out);
int vga_hca_ragged_offsets(const vga_hca_ragged *r, int64_t *frame_offsets_out, int64_t *pcm_row_offsets_out);

int vga_hca_decode_device_v(const vga_hca_ragged *r, const uint8_t *d_frames, int16_t *d_pcm, void *d_workspace,
                            size_t workspace_bytes, int *d_status, void *stream);
int vga_hca_encode_device_v(const vga_hca_ragged *r, const int16_t *d_pcm, uint8_t *d_frames, int *d_status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
