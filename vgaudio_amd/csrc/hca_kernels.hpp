// hca_kernels.hpp -- launchers for the CRI HCA kernels (device pointers).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "hca_device.hpp"

namespace vga {
namespace hca {

// bytes of decoder workspace per (stream, frame): the scan's hand-over record (hca_decode_core.hpp)
size_t decode_record_bytes(const DeviceInfo &info);

// frames: stream s at d_frames + s*frames_pitch (frame_count*frame_size bytes + >= 8 bytes slack);
// pcm: stream s channel c at d_pcm + s*stream_pitch + c*ch_pitch (samples)
// d_dims (device, one int4 per stream: {frame_count, sample_count, inserted_samples, 0}) or nullptr.  nullptr: every stream
// has info's three values.  With a table info.frame_count is the LONGEST stream's (it sizes the grid and the workspace,
// decode_record_bytes() * nstreams * info.frame_count as ever) and every stream decodes to its own values; the rows must be
// zero-padded or at least readable up to frames_pitch.
int launch_decode(const uint8_t *d_frames, int64_t frames_pitch, int nstreams, const DeviceInfo &info, int16_t *d_pcm,
                  int64_t stream_pitch, int64_t ch_pitch, void *d_workspace, int *d_status, hipStream_t stream,
                  const int4 *d_dims = nullptr);

// d_crc_pow: uint16[4096], x^(8k) mod 0x18005 (built by the host)
int launch_encode(const int16_t *d_pcm, int64_t stream_pitch, int64_t ch_pitch, int nstreams, const PcmMap &map,
                  const DeviceInfo &info, uint8_t *d_frames, int64_t frames_pitch, const uint16_t *d_crc_pow,
                  int *d_status, hipStream_t stream, int first_frame = 0, int frame_limit = -1);

// ---- packed streams (include/vgaudio_hip/hca_ragged.h): every stream's frames and PCM rows at offsets of their own, no
// pitch and no slot behind a stream's last frame.  The tables are made by the host once (capi_hca_ragged.hip) and read by
// the PACKED instantiations of the kernels; a stream without frames is in none of them.
struct PackedRun {                     // one workgroup (a wave of the one-wave encoder): frames [f0, f0 + len) of one stream
    int64_t frames_at;                 // the stream's first frame, bytes from d_frames (a multiple of 4)
    int64_t pcm_at;                    // the stream's first row, samples from d_pcm (a multiple of 8)
    int64_t frames_room;               // bytes from frames_at to the end of the frames buffer, slack included
    int ch_pitch;                      // samples from one row of the stream to the next
    int first_record;                  // the stream's frame 0 among all frames of the batch (the decoder's records)
    int f0, len;
    int frame_count, sample_count, inserted_samples;
    int zero_pre;                      // PcmMap::zero_pre of the stream (encoder)
    int stream;                        // the caller's index of the stream: its word of d_status
    int loop_map;                      // encoder: 0 = the stream does not loop, else 1 + its entry of the launch's PackedLoopMap table
};
static_assert(sizeof(PackedRun) == 64, "PackedRun is read as four 16-byte pieces");
// What the PcmMap of a looping stream has beyond a PackedRun (hca_device.hpp; made by make_pcm_map like every map): one entry
// per looping stream of a launch, read only where a run's cold fields are read.  The runs of plain streams carry loop_map 0
// and are byte for byte what they were before looping streams shared the packed launches.
struct PackedLoopMap {
    int post_end, loop_start, last_chunk;
    int raw_len;                       // samples the stream's rows hold: >= sample_count (the host batch's rows hold the whole file)
};
static_assert(sizeof(PackedLoopMap) == 16, "PackedLoopMap is read as one 16-byte piece");
struct PackedScanStream {              // the scan's view of a stream that has frames, in the caller's order
    int64_t frames_at, frames_room;
    int first_record, frame_count;
    int stream, reserved;
};
static_assert(sizeof(PackedScanStream) == 32, "PackedScanStream is read as two 16-byte pieces");
// device block of the scan: int4 {streams, total frames, 0, 0} | PackedScanStream[streams] | int first_stream[waves], where
// first_stream[w] is the stream that holds frame 64 w: a lane walks on from there over the streams that begin in its wave
inline size_t packed_scan_table_bytes(int streams, int total_frames)
{
    return 16 + (size_t)streams * sizeof(PackedScanStream) + (size_t)((total_frames + 63) / 64) * sizeof(int);
}

// info: the class (frame_count, sample_count, inserted_samples are not read); d_status: one word per stream of the caller
int launch_decode_packed(const uint8_t *d_frames, const DeviceInfo &info, int total_frames, const void *d_scan_table,
                         const PackedRun *d_runs, int nruns, int16_t *d_pcm, void *d_workspace, int *d_status, hipStream_t stream);
// wave_runs: d_runs was cut for the one-wave kernel (encode_wave_kernel_takes); d_loops: the table the runs' loop_map indexes
// (nullptr when no run has one)
int launch_encode_packed(const int16_t *d_pcm, const DeviceInfo &info, const PackedRun *d_runs, int nruns, bool wave_runs,
                         uint8_t *d_frames, const uint16_t *d_crc_pow, int *d_status, hipStream_t stream,
                         const PackedLoopMap *d_loops = nullptr);
// frames per run the launchers would choose for total_frames frames (0 < override: the test hook's value)
int decode_frames_per_group(int64_t total_frames, int override_value);
int encode_frames_per_run(const DeviceInfo &info, int64_t total_frames, int override_value, bool *wave_kernel);

// hca_encode_wave_kernel.hip: one wave per run of frames, one or two channels (launch_encode hands such streams over)
bool encode_wave_kernel_takes(const DeviceInfo &info);
int encode_wave_frames_per_run(int64_t total_frames, int override_value);
int launch_encode_wave_packed(const int16_t *d_pcm, const DeviceInfo &info, const PackedRun *d_runs, int nruns, uint8_t *d_frames,
                              const uint16_t *d_crc_pow, int *d_status, hipStream_t stream, const PackedLoopMap *d_loops);
int launch_encode_wave(const int16_t *d_pcm, int64_t stream_pitch, int64_t ch_pitch, int nstreams, const PcmMap &map,
                       const DeviceInfo &info, uint8_t *d_frames, int64_t frames_pitch, const uint16_t *d_crc_pow,
                       int *d_status, hipStream_t stream, int first_frame, int end_frame, int frames_per_run_override);

}  // namespace hca
}  // namespace vga
