// adx_kernels.hpp -- launchers for the CRI ADX kernels (device pointers).
#pragma once
#include <hip/hip_runtime.h>

#include "adx_host.hpp"                    // AdxDeviceParams and make_device_params, the pieces' figures

namespace vga {
namespace adx {

// d_own_frames / d_own_samples (device, one int per channel; nullptr: every channel is pcm_length / sample_count long): the
// channels are shorter streams zero-padded to the launch's length (the ragged entry points' length buckets) -- what lies past
// a channel's own ceil(length / 32) frames / own samples is not output, and the seams there are left alone.
int launch_encode(const int16_t *d_pcm, int64_t pcm_pitch, int nch, int pcm_length, const AdxDeviceParams &p,
                  uint8_t *d_out, int64_t out_pitch, int16_t *d_history_out, hipStream_t stream, const int *d_own_frames = nullptr);
int launch_decode(const uint8_t *d_adpcm, int64_t in_pitch, int nch, int sample_count, const AdxDeviceParams &p,
                  int16_t *d_pcm, int64_t pcm_pitch, int *d_status, hipStream_t stream, const int *d_own_samples = nullptr);

// ---- ragged device-resident batches (adx_ragged_kernels.hip; include/vgaudio_hip/adx_ragged.h, adx_host.hpp)
// The tables of a packed batch, in device memory.  A work slot is a lane: slot = group * 64 + lane, the channels longest
// first; the slots behind the last channel have length 0, offsets 0 and channel -1.
struct AdxRaggedTables {
    const int64_t *pcm_off, *adx_off;      // [slots] samples / bytes from the packed buffers' bases
    const int *length;                     // [slots] samples
    const int *channel;                    // [slots] the caller's index: where the history and the status word go
    const int64_t *crumb_base;             // [groups] the group's [group_frames][64] block among the encoder's crumbs
    int slots, nch;
};
// one direction's plan: (group, piece) pairs in device memory
struct AdxRaggedItems {
    const int2 *items;
    int count, segments, seg_frames;
};
// time_pieces: the object's frames are 18 bytes and unpadded (else: the general lane-per-channel kernels, no workspace).
// `workspace` is cut as adx_host.hpp says; nothing is allocated and the stream is not waited for.
int launch_encode_ragged(const int16_t *d_pcm, const AdxRaggedTables &t, const AdxRaggedItems &plan, bool time_pieces, int cus,
                         const AdxDeviceParams &p, uint8_t *d_adx, int16_t *d_history_out, void *workspace, hipStream_t stream);
int launch_decode_ragged(const uint8_t *d_adx, const AdxRaggedTables &t, const AdxRaggedItems &plan, bool time_pieces,
                         const AdxDeviceParams &p, int16_t *d_pcm, int *d_status, void *workspace, hipStream_t stream);

}  // namespace adx
}  // namespace vga
