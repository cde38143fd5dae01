/* vgaudio_hip/adx_ragged.h -- device-resident CRI ADX batches of channels of DIFFERENT lengths: packed PCM rows, packed ADX
 * rows, one set of launches per call (the ADX counterpart of vga_gcadpcm_ragged_create and of hca_ragged.h; the fourth way
 * to hand in a batch next to vga_adx_encode_batch, vga_adx_encode_device and vga_adx_encode_batch_v of ../vgaudio_hip.h).
 *
 * This header lives one directory below the drop-in header for the reason hca_ragged.h gives: the test files that hold every
 * function of include/ itself to the export check, the dirty-memory check, the busy-stream check and the loosest-layout check
 * enumerate the top-level headers and carry their own tables of cases; a function declared here is outside those lists.  The
 * same disciplines are applied to THIS header by tests/test_adx_ragged_device_host.py (exports, argument counts, and that the
 * GPU file's table of cases names every function declared here) and tests/test_gpu_adx_ragged_device.py (junk-filled buffers
 * larger than needed, poison mode, a busy caller stream, refused layouts).  Test hooks stay in ../vgaudio_hip_testing.h
 * (vga_testing_adx_ragged_stats).
 *
 * ONE PARAMETER SET PER OBJECT.  All channels share one vga_adx_params, validated exactly as vga_adx_encode_device validates
 * it (the same codes).  Coefficients, version, type and padding are kernel arguments; a caller with several sample rates or
 * loop paddings makes one object per set (the grouping vga_adx_encode_batch_v does on its own).  sample_counts[c] >= 0 are
 * free; a negative one is VGA_ERR_ARGUMENT and the message names the channel.
 *
 * LAYOUT (vga_adx_ragged_layout_for computes it on the host, no GPU needed; an object carries the same numbers)
 *   PCM   channel c's row starts pcm_offsets[c] samples into d_pcm and is sample_counts[c] long.
 *   ADX   its row starts adx_offsets[c] bytes into d_adx and is vga_adx_encoded_byte_count(sample_counts[c], p) long, which
 *         covers what the decoder reads too: floor(padding / spf) + ceil(n / spf) <= ceil((n + padding) / spf) frames.
 *   Rows follow each other in the caller's channel order, PCM rows rounded up to 8 samples, ADX rows to 16 bytes.  A channel
 *   of no bytes or no samples takes no room: its offset is the next channel's.  Each total (totals.pcm_samples,
 *   totals.adx_bytes) is the end of the last row plus a guard of 256 bytes (128 samples): loads may touch the guard, nothing
 *   writes it.  d_pcm, d_adx and d_workspace must be 16-byte aligned.  Anything less than these alignments, a null buffer,
 *   or a workspace smaller than the total says, is VGA_ERR_ARGUMENT before anything is launched.  nch == 0 is an empty
 *   batch: guards only, both calls return 0 and launch nothing.
 *
 * ENCODE  channel c's row receives bit for bit what one vga_adx_encode_device call on that channel alone writes
 * (CriAdxCodec.Encode of it), the zero bytes of frames that lie wholly inside the padding included; d_history_out[c]
 * (nch shorts, or NULL) as that call fills it.  An object that holds a channel of 0 samples while version == 4 and
 * padding == 0 gives VGA_ERR_ARGUMENT from the encode call (the reference reads pcm[0]); the message names the first such
 * channel, and the object is still good for decoding.
 * DECODE  channel c's row receives what one vga_adx_decode_device call on it writes, the zero tail of a padded stream whose
 * first frame yields fewer samples than asked included (CriAdxCodec.cs:18-34).  d_status has one int PER CHANNEL: the value
 * vga_adx_decode_device ORs into its single word for a frame naming a filter the table lacks (1) is OR-ed into d_status[c]
 * for channel c's own frames only; the caller zeroes the array, and the call returns 0.
 * Nothing is written outside a channel's own rows: not the rounding gaps, not the guards, not the input buffer.
 *
 * WHICH KERNELS.  Objects with frame_size == 18 and padding == 0 (and coefficients of the size the reference can produce:
 * |c| <= 16384) take the time-piece kernels of the equal-length calls in their ragged form: work slots are the channels
 * longest first (a stable sort), 64 slots form a group = one wave, the longest channel is cut into at most 64 time pieces,
 * and a wave is launched for every (group, piece) whose first frame lies inside the group's longest channel.  Padded
 * (looping) streams and other frame sizes take the general lane-per-channel kernel reading the same tables; their
 * workspace is 0 bytes and d_workspace may be NULL.  vga_testing_adx_ragged_stats reports which.
 *
 * Both calls run on the caller's stream and never synchronise it; all scratch is the caller's workspace (d_workspace, at
 * least totals.encode_workspace_bytes / decode_workspace_bytes; its content before and after a call means nothing), the
 * library allocates nothing per call.  The workspace is proportional to the batch's own frames -- 8 bytes per frame of every
 * group's longest channel and lane for the encoder, a few bytes per channel and piece besides -- never longest x channels.
 * The object keeps its tables in the memory of the device that was current at create, is immutable and serves any number of
 * calls, concurrent calls on different streams (each with a workspace of its own) included.  The piece plan is made at
 * create, on the creating thread (vga_testing_gc_encoder_segments_this_thread applies if it is set there) and never exceeds
 * 64 pieces; the workspace sizes hold for any plan, so vga_adx_ragged_layout_for and the object report the same numbers.
 * vga_testing_force_open_seams_this_thread is read at call time. */
#ifndef VGAUDIO_HIP_ADX_RAGGED_H
#define VGAUDIO_HIP_ADX_RAGGED_H

#include "../vgaudio_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vga_adx_ragged vga_adx_ragged;
typedef struct {
    int64_t pcm_samples, adx_bytes;   /* sizes of the two packed buffers, guards included */
    int     channels;
    int64_t total_frames;             /* sum over channels of the frames of the encoded stream */
    size_t  encode_workspace_bytes, decode_workspace_bytes;
} vga_adx_ragged_totals;

/* host only, needs no GPU.  pcm_offsets_out / adx_offsets_out: nch entries each; any of the three outputs may be NULL, but
 * not all of them. */
int  vga_adx_ragged_layout_for(const vga_adx_params *p, const int *sample_counts, int nch,
                               int64_t *pcm_offsets_out, int64_t *adx_offsets_out, vga_adx_ragged_totals *totals_out);
/* the same checks, then the plan and the kernels' tables in the current device's memory */
int  vga_adx_ragged_create(const vga_adx_params *p, const int *sample_counts, int nch, vga_adx_ragged **out);
void vga_adx_ragged_destroy(vga_adx_ragged *r);
int  vga_adx_ragged_channels(const vga_adx_ragged *r);
int  vga_adx_ragged_totals_of(const vga_adx_ragged *r, vga_adx_ragged_totals *out);
int  vga_adx_ragged_offsets(const vga_adx_ragged *r, int64_t *pcm_offsets_out, int64_t *adx_offsets_out);

int  vga_adx_encode_device_v(const vga_adx_ragged *r, const int16_t *d_pcm, uint8_t *d_adx, int16_t *d_history_out,
                             void *d_workspace, size_t workspace_bytes, void *stream);
int  vga_adx_decode_device_v(const vga_adx_ragged *r, const uint8_t *d_adx, int16_t *d_pcm,
                             void *d_workspace, size_t workspace_bytes, int *d_status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
