/* vgaudio_hip_files/hca_ragged_loops.h -- LOOPING streams in the packed CRI HCA encode: one set of launches for the streams
 * of a vga_hca_ragged object (../vgaudio_hip/hca_ragged.h), looping or not.  The older call, vga_hca_encode_device_v, keeps
 * refusing an object that holds a looping stream; this one takes the same object, the same buffers and the same layout and is
 * a superset of it: an object without loops may use either and gets the same bytes.
 *
 * LAYOUT  hca_ragged.h's, unchanged: stream s's frames at d_frames + frame_offsets[s], rows stream-major at
 * d_pcm + pcm_row_offsets[i], each row its stream's HcaInfo.sample_count long; d_frames 4-byte aligned, d_pcm 16; one status
 * word per stream (4 bitrate too low, 8, 16), OR-ed into, zeroed by the caller.  The call runs on the caller's stream, never
 * synchronises it and allocates nothing in the steady state: the encoder's tables of an object that holds a looping stream
 * are made on the first call (and once per value of the frames-per-run test hook), under the object's own lock.
 *
 * CONTRACT  stream s gets the bytes of one vga_hca_encode_device call with pcm_length = infos[s].sample_count and that
 * stream's HcaInfo.  The encoder's input behind the main audio of a looping stream is the loop audio replayed from the loop
 * start (CriHcaEncoder.cs:209-232, SaveLoopAudio :244-254), then zeros; every frame is encoded independently, so only a
 * stream's first and last few frames read that map at all.  Nothing is written outside a stream's own frames.
 *
 * REFUSALS  those of vga_hca_encode_device_v without the one for loops, same codes and messages: a null object, an object of
 * another device, "Bitrate is set too low.", an HcaInfo that does not describe its PCM, null or misaligned buffers --
 * VGA_ERR_ARGUMENT / VGA_ERR_INVALID_DATA before anything is launched.
 *
 * ROWS END AT SampleCount.  For a looping stream HcaInfo.sample_count is the loop end rounded as CriHcaEncoder.Initialize
 * rounds it, and a FILE may hold audio behind it.  The reference's encode of such a file reads that audio in one case only:
 * when the loop is SHORTER than the post audio (256 to 383 samples), SaveLoopAudio runs on behind the loop end.  A packed row
 * cannot supply those samples.  vga_hca_loop_may_read_tail tells: with
 *     post     = frame_count * 1024 - inserted_samples - appended_samples - sample_count
 *     loop_len = sample_count - (loop_start_frame * 1024 + pre_loop_samples - inserted_samples)
 * it returns looping && loop_len < post.  0: the packed encode equals the reference's encode of the whole file whatever
 * lies behind sample_count.  1: it equals it only for a file that ENDS at sample_count; a caller whose file is longer encodes
 * that file by a vga_hca_encode_device call of its own with the file's length (hca.write_files does). */
#ifndef VGAUDIO_HIP_FILES_HCA_RAGGED_LOOPS_H
#define VGAUDIO_HIP_FILES_HCA_RAGGED_LOOPS_H

#include "../vgaudio_hip/hca_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

/* host only, no GPU: 1 if the packed encode of this stream can differ from the reference's encode of a FILE that has audio
 * behind HcaInfo.SampleCount (see above), 0 if not, < 0 on a bad info */
int vga_hca_loop_may_read_tail(const vga_hca_info *info);
int vga_hca_encode_loops_device_v(const vga_hca_ragged *r, const int16_t *d_pcm, uint8_t *d_frames, int *d_status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
