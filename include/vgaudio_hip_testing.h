/*
 * vgaudio_hip_testing.h -- test-only exports of libvgaudio_hip.so.  NOT part of the drop-in surface
 * (include/vgaudio_hip.h); nothing a managed shim binds lives here.
 */
#ifndef VGAUDIO_HIP_TESTING_H
#define VGAUDIO_HIP_TESTING_H

#ifdef __cplusplus
extern "C" {
#endif

/* GC-ADPCM encode/decode and ADX encode/decode cut long channels into time segments that run side by side and
 * close the seams afterwards (LABNOTES.md 4.3).  mode = 1: calls made FROM THE CALLING THREAD never accept a seam
 * as closed; 2: only the even seams of every third channel are kept open (a mix of open and closed seams inside
 * one workgroup); 3: every seam, and the decoders count them as seams that would not close, so that their REPAIR launch
 * (one piece per wave from the first open seam on; round 5) produces the output instead of the chained tail kernel;
 * 0: normal operation.  The serial fall-backs then produce the output, which must not change.
 * The setting is thread-local (no other thread's calls see it) and is passed to the kernels as a launch argument.
 * Returns the calling thread's previous mode. */
int vga_testing_force_open_seams_this_thread(int mode);

/* GC-ADPCM encoder wave layout for calls made FROM THE CALLING THREAD: 0 = the launcher's choice (the product: 4 for
 * batches below ~512 channels, 8 from there on and for ragged batches); 8 = lane per (channel, predictor); 4 = lane per
 * (channel, predictor, scale candidate).  8 also names the workgroup shape: two encoder waves and a helper wave, sixteen
 * channel slots.  1 = the (channel, predictor) lanes in the self-served shape -- one-wave workgroups of eight channel slots
 * that take (group of eight, piece) items from a queue, each wave helper and encoder of its own channels -- which the
 * launcher picks by itself from 2048 channels on and for ragged batches; it runs as persistent workgroups whatever
 * vga_testing_gc_encoder_persistent_this_thread says.  All produce the same bytes.  Returns the previous value; other
 * arguments leave it unchanged. */
int vga_testing_gc_encoder_layout_this_thread(int channels_per_wave);
/* GC-ADPCM coefficient-search kernel for calls made from the calling thread: 0 = the launcher's choice by channel count
 * (the product), 1 = one wave per channel, 2 = workgroups of four channels and a summing wave, 3 = the same five waves on
 * one channel (the choice for small batches).  Same coefficients.
 * Returns the previous value; other arguments leave it unchanged. */
int vga_testing_gc_coefs_variant_this_thread(int variant);
/* Forces the number of time pieces a channel is cut into by the kernels that speculate over time -- the GC-ADPCM and ADX
 * encoders (pieces of 64 frames or more) and decoders (8 frames or more) -- for calls made from the calling thread (0 = the
 * launcher's own choice).  Results must not depend on it.  Returns the previous value. */
int vga_testing_gc_encoder_segments_this_thread(int segments);
/* How the GC-ADPCM encoder hands its (channel group, time piece) items to workgroups, for calls made from the calling
 * thread: 0 = the launcher's choice, 1 = one workgroup per item (a plain grid), 2 = persistent workgroups taking items from
 * a queue.  Results must not depend on it.  Returns the previous value. */
int vga_testing_gc_encoder_persistent_this_thread(int mode);

/* The GC-ADPCM encoder's piece schedule (gc::plan_encode_pieces, vgaudio_amd/csrc/gc_encode_kernel.hip) for a device of
 * `cus` compute units: `groups` channel groups of sixteen whose longest channel has `frames` frames and whose longest
 * channels hold `group_frames` frames in all.  Host arithmetic, needs no GPU.  out5 = {pieces, big, nb, small, persistent}:
 * piece k begins at frame min(k, nb) * big + max(k - nb, 0) * small.  The pieces must cover `frames`.  With
 * vga_testing_gc_encoder_layout_this_thread(1) in force: the schedule of the self-served shape (always persistent; the rounds
 * of the two-size schedule counted in groups of eight on twelve workgroups per compute unit; on uniform batches whose tail
 * descends this is the schedule of the groups that keep the coarse tail, see vga_testing_gc_plan_pieces_n).  Returns 0. */
int vga_testing_gc_plan_pieces(int cus, int groups, int frames, long long group_frames, int ragged, int *out5);
/* ... the same with the whole schedule: out10 = {pieces, big, nb, small, n1, s2, n2, s3, persistent, 0} -- behind the nb big
 * pieces come n1 pieces of `small` frames, then n2 of s2, then pieces of s3 (n1 or n2 = 1 << 30: that level has no end and the
 * later ones are unused).  coarse != 0: the schedule of the groups of eight whose seams are likely to close slowly (the
 * self-served shape on uniform batches: one tail level, of pieces no shorter than 4096 frames). */
int vga_testing_gc_plan_pieces_n(int cus, int groups, int frames, long long group_frames, int ragged, int coarse, int *out10);

/* Diagnostics of the GC-ADPCM encoder's data-dependent parts, summed over every launch of the process on the current
 * device since the last reset (the call synchronises the device first): out8 = {seams closed inside their piece, seams left
 * open for the chain kernel, frames re-encoded by seam runs, wave-frames encoded, wave-frames that took the cold block
 * (third trips of the retry loop, GcAdpcmEncoder.cs:127-170; counted by -DVGA_GC_STATS builds only), channels the chain kernel
 * walked, pieces encoded, 1 if this build counts the cold blocks}.
 * reset != 0 clears the counters afterwards.  Returns 0, or -1 when the device cannot be read. */
int vga_testing_gc_encode_stats(unsigned long long *out8, int reset);
/* ... the same with n <= 9 fields: [8] = channels with an open seam whose chain the self-served encoder walked inside its own
 * launch (the hand-over below) -- the channels the chain kernel counts in [5] when the hand-over is switched off. */
int vga_testing_gc_encode_stats_n(unsigned long long *out, int n, int reset);

/* The self-served GC-ADPCM encoder (layout 1) on uniform batches continues an open seam into the next piece inside its own
 * launch, as soon as that piece and its own seam run are finished, and leaves the chain kernel a record per channel; the chain
 * kernel then walks nothing but the partial last frame of a run that never met.  on = 0: calls made from the calling thread
 * leave every open seam to the chain kernel, as ragged batches and the other shapes do; on != 0 (the default): normal
 * operation.  Same bytes.  Returns the previous setting. */
int vga_testing_gc_seam_handover_this_thread(int on);
/* The schedule of the self-served GC-ADPCM encoder on uniform batches, for calls made from the calling thread, at any batch
 * size: the workgroups' share of the frames in big_rounds rounds of big items, then tail_counts[i] pieces per channel of
 * tail_frames[i] frames, i = 0, 1, 2 (descending; a count of 0 skips the level), none shorter than min_tail_frames (at least
 * 64).  The groups flagged as slow-closing take tail_counts[0] pieces of max(tail_frames[0], min(4096, 4 * min_tail_frames))
 * frames instead.  big_rounds = 0 (or null arrays) restores the default.  Same bytes.  Returns the previous big_rounds. */
int vga_testing_gc_schedule_this_thread(int big_rounds, const int *tail_counts, const int *tail_frames, int min_tail_frames);
/* With the hand-over in force the same launch takes the groups of eight channels whose seams are likely to close slowly --
 * a predictor with complex poles next to the unit circle, vgaudio_amd/csrc/gc_plan8.hpp -- from its queue first.  The order
 * of the groups for nch channels' coefficients (16 per channel): order[(nch + 7) / 8] = the flagged groups, ascending, then
 * the others, ascending; returns the number of flagged groups, or -1.  _host: coefs in host memory, host code, needs no GPU;
 * _device: d_coefs in device memory, the table built by the kernel the encoder launches (null stream; the call waits). */
int vga_testing_gc_slow_order_host(const short *coefs, int nch, int *order);
int vga_testing_gc_slow_order_device(const void *d_coefs, int nch, int *order);
/* The one launch in front of the self-served encoder on uniform batches (gc_self_served_prologue_kernel): it builds that table
 * with a flag per group behind it and fills the scratch the encoder's queue starts from -- zero_ints words of zeros (the queue's
 * head, the seams' counters and words), a zero per channel (the channels' records) and "no open seam" per channel.  Runs it
 * (null stream; the call waits) on buffers of its own whose every byte was 0xFF: order_flags[2 * ((nch + 7) / 8) + 1] = the
 * order, the number of flagged groups, the flags; *bad_words = the words of the fills, and of a guard behind them, that do
 * not hold what they should.  Returns the number of flagged groups, or -1. */
int vga_testing_gc_prologue_device(const void *d_coefs, int nch, int zero_ints, int *order_flags, int *bad_words);

/* The host-pointer entry points (vga_*_batch) move data through a pipeline of feeder threads, pinned rings, per-chunk
 * kernel launches and drainer threads (vgaudio_amd/csrc/host_pipeline.hpp); its shape normally follows the volume of
 * the call.  Non-zero arguments override it for calls made FROM THE CALLING THREAD (0 = automatic): feeder / drainer
 * thread counts (a NEGATIVE feeder count: that many feeders with an upload stream each instead of one shared stream, and a
 * download stream per drainer), units (channels, streams) per chunk, bytes per ring slot.  Results must not depend on any of
 * them. */
void vga_testing_host_pipeline_this_thread(int feeders, int drainers, int chunk_units, int slot_bytes);

/* ... and the size of the call's LAST chunk (the last regular chunk is split once into (rest, tail); 0 = automatic: 3/8 of a
 * chunk). */
void vga_testing_host_pipeline_tail_this_thread(int tail_units);

/* The ragged ADX / HCA entry points (vga_adx_*_batch_v, vga_hca_encode_batch_v) sort their units into chunks of one parameter
 * group and similar length (vgaudio_amd/csrc/host_batch.hpp, plan_buckets) and run the chunks shortest first (ADX) or longest
 * first (HCA).  vga_testing_plan_buckets() returns that plan for n units -- order_out[n]: position -> unit;
 * chunk_begin_out[chunks + 1]: positions; chunk_length_out / chunk_group_out[chunks]: a chunk's largest length and its group --
 * and the number of chunks (-1: bad arguments or more than max_chunks).  Host code, no GPU.
 * vga_testing_buckets_order_this_thread(1 | 2) forces shortest / longest first for calls made from the calling thread
 * (0: the entry point's own order; timing comparisons -- results must not depend on it). */
int vga_testing_plan_buckets(const int *group, const int *length, int n, int max_units, long long max_volume, int longest_first,
                             int *order_out, int *chunk_begin_out, int *chunk_length_out, int *chunk_group_out, int max_chunks);
void vga_testing_buckets_order_this_thread(int order);
/* Page-locked rows of the host-pointer entry points, for calls made from the calling thread: 0 (default) = moved by transfer
 * kernels on compute units reserved for them (calls of 256 MB and more whose rows average under 4 MB), 1 = one hipMemcpyAsync
 * per row as until round 5, 2 = transfer kernels whatever the call's size: the gather of direct uploads (one feeder), the
 * scatter of direct downloads and of staged ring slots, on masked streams.  Other values: 0.
 * vga_testing_host_transfer_piece_bytes_this_thread() sets the largest piece one workgroup of those kernels copies
 * (0 = the pipeline's 256 KB; at least 4096), so that rows of a few KB travel in several pieces.  Results must not depend on
 * either. */
void vga_testing_host_transfer_this_thread(int mode);
void vga_testing_host_transfer_piece_bytes_this_thread(int bytes);
/* Compute streams of the host-pointer entry points' pipeline (chunk k's kernels on stream k % lanes, at most 4): 0 = the
 * entry point's own choice -- for calls made from the calling thread.  The GC-ADPCM encoders size their per-lane buffers for
 * the count before they allocate; the entry points that share one buffer between chunks (vga_gcadpcm_calculate_coefficients_batch,
 * vga_gcadpcm_encode_with_coefs_batch) always run one lane.  Results must not depend on it. */
void vga_testing_host_compute_lanes_this_thread(int lanes);

/* Failure injection for calls made from the calling thread: the nth step (counting from 1, from this call of the hook on) of
 * the given kind is refused -- the entry point returns VGA_ERR_DEVICE and vga_last_error() reads
 * "step refused by vga_testing_fail_step_this_thread".  A refused step is a host-side error return: nothing of it is handed
 * to HIP.  The steps the calling thread's pipelines run on their feeder and drainer threads (transfer launches) count
 * towards the calling thread's setting.  A call spread over several GPUs (vga_set_devices) gives every other share's thread
 * a copy of the setting, which counts that share's steps on its own.  kind 0 (or nth <= 0) switches the injection off. */
enum {
    VGA_TESTING_STEP_CHUNK_COMPUTE = 1,      /* a pipeline chunk's kernel launches (pipe::Job::compute) */
    VGA_TESTING_STEP_TRANSFER = 2,           /* a transfer-kernel launch of the pipeline (gather, scatter, staged scatter) */
    VGA_TESTING_STEP_HCA_STREAM_FRAMES = 3   /* the frame launch of vga_hca_stream_encode (calls that complete frames) */
};
void vga_testing_fail_step_this_thread(int kind, int nth);

/* Where the wall time of the calling thread's last pipelined call went, in seconds (diagnostics for bench.py's e2e
 * block): [0] total [1] set-up [2] feeders' memcpy (sum over threads) [3] feeders waiting for a ring slot [4] feeders
 * inside hipMemcpyAsync/hipEventRecord [5] slowest feeder [6] caller waiting for uploads [7] caller launching kernels
 * [8] caller's final stream sync [9] drainers waiting for compute [10] drainers waiting for downloads [11] drainers'
 * memcpy [12] slowest drainer [13] feeders [14] drainers [15] chunks [16] units per chunk [17] device allocation
 * before the pipeline [18] the whole entry point up to its return value [19] feeders at chunk boundaries [20] feeders' final
 * stream synchronisation [21] drainers page-locking the output rows.  Returns the number of fields. */
int vga_testing_last_pipeline_stats(double *out, int n);

/* The HCA decoder's second kernel gives a workgroup a run of consecutive frames of one stream and carries the IMDCT overlap
 * inside the run (1..16 frames, by the size of the batch).  > 0 forces the run length for calls made from the calling
 * thread (0 = the launcher's choice).  PCM must not depend on it.  Returns the previous value. */
int vga_testing_hca_frames_per_group_this_thread(int frames);

/* The HCA kernels' view of a stream (vgaudio_amd/csrc/hca_info.hpp: DeviceInfo -- channel types, coded band counts, the
 * scaled ATH curve), as the library derives it from an HcaInfo; `out` receives sizeof(DeviceInfo) = 240 bytes.  Host code,
 * needs no GPU: the CPU suite feeds it to the lane emulator of the HCA decoder (tests/host/hca_decode_emulator.cpp). */
int vga_testing_hca_device_info(const void *hca_info, void *out, int out_bytes);

/* vga_hca_decode_batch_v sorts its streams into shape classes -- equality of the DeviceInfo above with frame_count,
 * sample_count and inserted_samples ignored; the loop fields, comment_length and header_size of the HcaInfo are not part of
 * it -- and the streams of one class and one length bucket share their launches.  infos: nstreams vga_hca_info;
 * class_out[s]: the class of stream s, dense ids in order of first appearance.  Returns the number of classes, negative on
 * bad arguments or an HcaInfo the decoder refuses.  Host code, needs no GPU. */
int vga_testing_hca_decode_classes(const void *infos, int nstreams, int *class_out);
/* The calling thread's last vga_hca_decode_batch_v call: [0] pipeline jobs run (one per channel count present and device
 * share) [1] chunks = launch sets [2] shape classes [3] own frames (the sum of the streams' frame_count) [4] frame slots
 * launched (the sum over the chunks of streams x the chunk's longest frame_count; a slot behind a stream's own frames does
 * no work).  Writes min(n, 5) fields and returns 5. */
int vga_testing_hca_decode_v_stats(long long *out, int n);
/* The calling thread's last vga_hca_encode_batch_v call: [0] streams [1] groups (streams of one group may share launches:
 * plain streams by quality, bitrate, channels and rate; looping streams by the same and NOT by their loops) [2] chunks
 * [3] encode launches (one per chunk that has frames).  Writes min(n, 4) fields and returns 4. */
int vga_testing_hca_encode_v_stats(long long *out, int n);
/* A packed batch (vgaudio_hip/hca_ragged.h; ragged: a vga_hca_ragged): [0] own frames (the sum of the streams' frame_count)
 * [1] scan slots launched (own frames rounded up to the 64 lanes of a wave: no slot lies behind a stream's frames) [2]
 * workgroups of the decoder's second kernel [3] runs in its table (one workgroup each; streams without samples have none).
 * Host state of the object at the launcher's own frames per run: the call launches nothing.  Writes min(n, 4) fields and
 * returns 4. */
int vga_testing_hca_ragged_stats(const void *ragged, long long *out, int n);

/* The ADX file reader (vga_adx_read_device) moves 18-byte frames with a kernel of 16-byte vectors when the rows are 16-byte
 * aligned.  on != 0 sends calls made from the calling thread to the general de-interleave instead; the bytes must not
 * change.  Returns the previous setting. */
int vga_testing_adx_read_general_this_thread(int on);

/* Which kernel form the ADX launchers took for the last vga_adx_encode_device / vga_adx_decode_device call (or
 * host-pointer chunk) made FROM THE CALLING THREAD: 0 = none yet, 1 = the time-piece kernels (18-byte frames on the
 * layout include/vgaudio_hip.h names next to those calls), 2 = the general lane-per-channel kernel.  Either pointer
 * may be null.  Host state only: the call allocates and launches nothing.  Returns 0. */
int vga_testing_adx_last_path_this_thread(int *encode, int *decode);
/* A packed ADX batch (vgaudio_hip/adx_ragged.h; ragged: a vga_adx_ragged): [0] own frames (the sum of the channels' encoded
 * frames) [1] groups of 64 work slots [2] the encoder's time pieces [3] their length in frames [4] the (group, piece) items
 * its first kernel is launched over -- one wave each, none wholly behind its group's longest channel -- [5] [6] [7] the same
 * for the decoder [8] the encoder's path [9] the decoder's (1 = the time-piece kernels, 2 = the general lane-per-channel
 * kernel, as vga_testing_adx_last_path_this_thread, which the *_device_v calls record in as well; 0 = an empty batch).
 * Host state of the object: the call launches nothing.  Writes min(n, 10) fields and returns 10. */
int vga_testing_adx_ragged_stats(const void *ragged, long long *out, int n);

/* Poison mode for every allocation the library makes.  The device pool of the host-pointer entry points hands a parked block
 * of 1 MiB or more to any later request of half its size or more with the last call's bytes in it, the page-locked pool any
 * idle block that is large enough, and the stream-ordered scratch of the device entry points is recycled by the runtime's
 * pool: in production no buffer starts out as zeros.  byte = 0..255: every block -- pooled or fresh device blocks, the
 * stream-ordered scratch, page-locked blocks, and the tables of ragged batches, sound banks and the CRC -- is filled with
 * that byte before it is handed out; results must not depend on it.  -1 (the default) switches the mode off; other values
 * leave the setting unchanged.  PROCESS-WIDE (the pools are), host state only: the call itself touches no device and needs
 * none.  Stream-ordered scratch is filled on the caller's stream, which is never waited for; a block without a stream is
 * filled on the null stream and the fill has completed when the block is handed out.  Returns the previous setting. */
int vga_testing_poison_allocations(int byte);

#ifdef __cplusplus
}
#endif
#endif
