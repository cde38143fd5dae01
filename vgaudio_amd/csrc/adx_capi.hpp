// adx_capi.hpp -- what the CRI ADX C-ABI files of host rows share and that needs HIP types (capi_adx.hip, capi_adx_v.hip).
// The arithmetic and the argument checks, without HIP, are in adx_host.hpp.
#pragma once
#include "common.hpp"
#include "host_batch.hpp"
#include "adx_kernels.hpp"

#include <cstring>

namespace vga {
namespace adx {

constexpr int ADX_CHUNK_CHANNELS = 1024;        // channels per chunk of the host pipeline (host_pipeline.hpp): the piece-wise kernels fill the chip from 1024 on
constexpr int ADX_MIN_SHARE_CHANNELS = 128;     // channels per share of a call spread over several GPUs (vga_set_devices)
constexpr int64_t ADX_BUCKET_VOLUME = (int64_t)1024 * 2880000;   // padded samples per chunk of a ragged call: what ADX_CHUNK_CHANNELS x 60 s hold

// A host-pointer call as one(first_channel, channel_count) per share of vga_set_devices()'s GPUs.  A call without channels
// or without one of its arrays is `one`'s whole, which refuses it or has nothing to do.
template <class One>
inline int for_each_share(int nch, bool arrays, One one)
{
    if (nch <= 0 || !arrays) return one(0, nch);
    return for_each_device_share(nch, ADX_MIN_SHARE_CHANNELS, one);
}

// parameter groups of a ragged call: channels whose device parameters are the same bytes
inline int group_of(std::vector<AdxDeviceParams> &seen, const AdxDeviceParams &d)
{
    for (size_t i = 0; i < seen.size(); i++)
        if (memcmp(&seen[i], &d, sizeof d) == 0) return (int)i;
    seen.push_back(d);
    return (int)seen.size() - 1;
}

// the tail of a decode job: the pipeline, then the decoders' status word as the call's error
inline int run_decode_job(pipe::Job &job, DevBuf &d_status)
{
    return run_status_job(job, ADX_CHUNK_CHANNELS, d_status, "a frame names a filter the coefficient table lacks (IndexOutOfRangeException in the reference)");
}

}  // namespace adx
}  // namespace vga
