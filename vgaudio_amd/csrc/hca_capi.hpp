// hca_capi.hpp -- what the HCA C-ABI files share and that needs HIP types (capi_hca.hip, capi_hca_stream.hip, capi_hca_v.hip,
// capi_hca_ragged.hip; capi_crypt.hip and container_readers.hip for the CRC table).  The derivations without HIP are in
// hca_host.hpp.
#pragma once
#include "common.hpp"
#include "host_batch.hpp"
#include "hca_kernels.hpp"
#include "hca_host.hpp"
#include "../../include/vgaudio_hip/hca_ragged.h"

#include <vector>

namespace vga {
namespace hca {

// x^(8k) mod (x^16 + x^15 + x^2 + 1), k = 0..65535, uploaded once per device (capi_hca.hip); shared with the encryption
// pass (capi_crypt.hip) and the file reader (container_readers.hip)
int crc_pow_table(const uint16_t **out);

// streams per chunk of the host pipeline (host_pipeline.hpp): 256 stereo streams x 2813 frames = 720 k workgroups
constexpr int HCA_CHUNK_STREAMS = 256;
constexpr int HCA_MIN_SHARE_STREAMS = 32;       // streams per share of a call spread over several GPUs (vga_set_devices)
constexpr int64_t HCA_BUCKET_VOLUME = (int64_t)HCA_CHUNK_STREAMS * 2880000;      // padded samples per chunk and channel
// A decode downloads several times what it uploads and its first download waits for the first chunk's kernels: chunks a
// quarter of the encoder's, as planned_chunk_units() cuts the equal-length decode's.  The volume is in bytes of frames.
constexpr int HCA_DECODE_CHUNK_STREAMS = HCA_CHUNK_STREAMS / 4;
constexpr int64_t HCA_DECODE_BUCKET_VOLUME = (int64_t)HCA_DECODE_CHUNK_STREAMS << 20;

// the encoder's input stream (hca_device.hpp PcmMap), from the fields CriHcaEncoder.Initialize derived
inline int make_pcm_map(const vga_hca_info &h, int pcm_length, PcmMap &m)
{
    const int input_samples = h.frame_count * SPF - h.inserted_samples - h.appended_samples;
    const int pre = h.inserted_samples - SPSF;
    if (pre < 0 || h.sample_count < 0 || h.sample_count > pcm_length || input_samples < h.sample_count) {
        set_error("HcaInfo does not describe this PCM (sample count %d of %d, inserted %d, appended %d)", h.sample_count,
                  pcm_length, h.inserted_samples, h.appended_samples);
        return VGA_ERR_ARGUMENT;
    }
    m.zero_pre = pre > SPF ? (divide_by_round_up(pre, SPF) - 1) * SPF : 0;
    m.pre_end = pre;
    m.main_end = pre + h.sample_count;
    m.post_end = m.main_end + (h.looping ? input_samples - h.sample_count : 0);   // not looping: _postAudio is all zero
    m.loop_start = h.loop_start_frame * SPF + h.pre_loop_samples - h.inserted_samples;
    m.last_chunk = h.sample_count > 0 ? (h.sample_count - 1) / SPF : 0;
    m.raw_len = pcm_length;
    return VGA_OK;
}

// the encoder's part of a PackedRun (hca_kernels.hpp) from the stream's map: zero_pre, and for a looping stream its entry of the
// launch's PackedLoopMap table (loops == nullptr: the caller encodes plain streams only).  raw_len: samples in the stream's rows.
inline int set_encoder_map(PackedRun &r, const vga_hca_info &h, int raw_len, std::vector<PackedLoopMap> *loops)
{
    PcmMap m;
    if (int rc = make_pcm_map(h, raw_len, m)) return rc;
    r.zero_pre = m.zero_pre;
    if (h.looping && loops) {
        loops->push_back(PackedLoopMap{m.post_end, m.loop_start, m.last_chunk, m.raw_len});
        r.loop_map = (int)loops->size();
    }
    return VGA_OK;
}

// the status word of a host batch job, zeroed: its kernels OR their flag bits into it
inline int alloc_status_word(DevBuf &d_status)
{
    VGA_HIP_TRY(d_status.alloc(sizeof(int)));
    VGA_HIP_TRY(hipMemset(d_status.p, 0, sizeof(int)));
    return VGA_OK;
}

// the tail of every host batch job: the pipeline, then the status word as the call's error
inline int run_status_job(pipe::Job &job, int chunk_units, DevBuf &d_status)
{
    if (int rc = run_batch_pipeline(job, chunk_units)) return rc;
    int status = 0;
    VGA_HIP_TRY(hipMemcpy(&status, d_status.p, sizeof(int), hipMemcpyDeviceToHost));
    return status_to_error(status);
}

// A pipeline job has one row count per unit: run(units, nch) once per channel count present among the streams
// [first, first + count), units = those streams' indices in the caller's order
template <class ChannelsOf, class Run>
inline int for_each_channel_count(int first, int count, ChannelsOf channels_of, Run run)
{
    for (int nch = 1; nch <= 8; nch++) {
        std::vector<int> units;
        for (int s = first; s < first + count; s++)
            if (channels_of(s) == nch) units.push_back(s);
        if (units.empty()) continue;
        if (int rc = run(units, nch)) return rc;
    }
    return VGA_OK;
}

// ---- the packed layout of a device-resident ragged batch (capi_hca_ragged.hip)
struct RaggedLayout {
    std::vector<vga_hca_info> infos;
    DeviceInfo cls;                        // the class: the first stream's DeviceInfo
    std::vector<int64_t> frame_at, row_at; // [nstreams], [rows]
    std::vector<size_t> first_row;         // stream -> its first row
    std::vector<int> first_record;         // stream -> its frame 0 among all frames
    vga_hca_ragged_totals totals;
    int first_looping = -1;
};
// the one place the layout is made: vga_hca_ragged_layout_for and vga_hca_ragged_create
int make_layout(const vga_hca_info *infos, int nstreams, RaggedLayout &L);
// the runs {stream, first frame, length} of one launch: every stream's frames cut at per_run, never across a stream's end.
// The decoder's second kernel has nothing to do for a stream without samples; the encoder writes such a stream's frames.
// loops (encoder): receives the PackedLoopMap of every looping stream, whose runs then name it; nullptr: plain maps only.
std::vector<PackedRun> cut_runs(const RaggedLayout &L, int per_run, bool encoder, std::vector<PackedLoopMap> *loops = nullptr);

}  // namespace hca
}  // namespace vga
