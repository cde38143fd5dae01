// capi_hca_stream.hip -- the C ABI of CriHcaEncoder's streaming shell (vga_hca_stream_*, include/vgaudio_hip.h).
#include "hca_capi.hpp"

#include <cstring>
#include <deque>
#include <memory>
#include <vector>

using namespace vga;
using namespace vga::hca;

// ---------------------------------------------------------------- CriHcaEncoder's streaming shell (CriHcaEncoder.cs:126-269)
// The reference's encoder is a stateful object fed [channels][1024] blocks; Encode() returns how many frames the block
// completed -- none while the 1024-sample buffer fills, several when the pre-audio of a looping stream or the post-audio at
// the end flush whole frames -- the first into the caller's buffer, the rest into a queue (GetPendingFrame).  Here a frame is
// a function of the stream's PCM alone (hca_device.hpp PcmMap; every frame independent), so the shell keeps what the caller
// has fed in HBM (whole blocks: SaveLoopAudio :244-254 reads a block beyond the stream's last sample), walks the reference's
// counters to know which frames this call completes, and runs hca_encode_kernel on exactly those.
struct vga_hca_stream {
    vga_hca_info info;
    hca::DeviceInfo dev;
    hca::PcmMap map;
    int device = 0;
    int nch = 0, chunks = 0, chunks_fed = 0;
    hca::StreamCounters counters;          // the reference's (hca_host.hpp)
    std::deque<std::vector<uint8_t>> pending;
    DevBuf d_pcm, d_frames, d_status;
    std::vector<uint8_t> host_frames;
    hipStream_t s = nullptr;
};

extern "C" {

int vga_hca_stream_create(const vga_hca_params *c, vga_hca_info *info_out, vga_hca_stream **out)
{
    if (!out) { set_error("null output"); return VGA_ERR_ARGUMENT; }
    *out = nullptr;
    vga_hca_info h;
    if (int rc = vga_hca_encoder_initialize(c, &h)) return rc;
    if (info_out) *info_out = h;
    if (bitrate_too_low(h)) { set_error("Bitrate is set too low."); return VGA_ERR_INVALID_DATA; }   // (vga_hca_encode_device)
    if (int rc = require_device()) return rc;
    std::unique_ptr<vga_hca_stream> st(new vga_hca_stream);
    st->info = h;
    if (int rc = make_device_info(h, st->dev)) return rc;
    st->nch = h.channel_count;
    // the blocks the reference consumes: one per started 1024 samples of the (loop-trimmed) stream, at least one
    st->chunks = std::max(1, divide_by_round_up(h.sample_count, hca::SPF));
    if (int rc = make_pcm_map(h, st->chunks * hca::SPF, st->map)) return rc;
    st->map.last_chunk = st->chunks - 1;
    st->counters = stream_counters_for(h);
    (void)hipGetDevice(&st->device);
    const size_t pcm_bytes = (size_t)st->nch * st->chunks * hca::SPF * 2;
    VGA_HIP_TRY(st->d_pcm.alloc(pcm_bytes));
    VGA_HIP_TRY(hipMemset(st->d_pcm.p, 0, pcm_bytes));
    VGA_HIP_TRY(st->d_frames.alloc((size_t)frames_pitch_for(h)));
    if (int rc = alloc_status_word(st->d_status)) return rc;
    VGA_HIP_TRY(hipStreamCreateWithFlags(&st->s, hipStreamNonBlocking));
    *out = st.release();
    return VGA_OK;
}

void vga_hca_stream_destroy(vga_hca_stream *st)
{
    if (!st) return;
    if (st->s) (void)hipStreamDestroy(st->s);
    delete st;
}

int vga_hca_stream_frame_size(const vga_hca_stream *st) { return st ? st->info.frame_size : 0; }
int vga_hca_stream_frames_processed(const vga_hca_stream *st) { return st ? st->counters.frames_processed : 0; }
int vga_hca_stream_pending_frame_count(const vga_hca_stream *st) { return st ? (int)st->pending.size() : 0; }

int vga_hca_stream_get_pending_frame(vga_hca_stream *st, uint8_t *frame_out)
{
    if (!st || !frame_out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (st->pending.empty()) { set_error("There are no pending frames"); return VGA_ERR_INVALID_OP; }    // :158
    std::memcpy(frame_out, st->pending.front().data(), st->pending.front().size());
    st->pending.pop_front();
    return VGA_OK;
}

int vga_hca_stream_encode(vga_hca_stream *st, const int16_t *const *pcm, uint8_t *hca_out, int *frames_output)
{
    if (!st || !pcm || !hca_out || !frames_output) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    *frames_output = 0;
    const vga_hca_info &h = st->info;
    if (stream_finished(st->counters, h)) {                                                 // :128-131
        set_error("All audio frames have already been output by the encoder");
        return VGA_ERR_INVALID_OP;
    }
    for (int c = 0; c < st->nch; c++)
        if (!pcm[c]) { set_error("pcm[%d] is null", c); return VGA_ERR_ARGUMENT; }
    int device = -1;
    (void)hipGetDevice(&device);
    if (device != st->device) { set_error("the stream was created on device %d, the current one is %d", st->device, device); return VGA_ERR_ARGUMENT; }
    // the block joins the stream's PCM in HBM (blocks past the stream's end carry nothing the reference reads).  A call that
    // fails is rolled back to before its block, chunks_fed included: the retry writes the same block to the same slot.
    const int saved_fed = st->chunks_fed;
    if (st->chunks_fed < st->chunks) {
        const int64_t ch_pitch = (int64_t)st->chunks * hca::SPF;
        for (int c = 0; c < st->nch; c++)
            VGA_HIP_TRY(hipMemcpyAsync(st->d_pcm.as<int16_t>() + c * ch_pitch + (int64_t)st->chunks_fed * hca::SPF, pcm[c],
                                       hca::SPF * sizeof(int16_t), hipMemcpyHostToDevice, st->s));
        // the caller reuses its block buffer for the next call (CriHcaFormat.cs:50-56 does): the block is on the device before
        // this call returns, whether or not it completes a frame
        VGA_HIP_TRY(hipStreamSynchronize(st->s));
        st->chunks_fed++;
    }
    // ---- the reference's counters through this call (Encode :126-156 and what it calls): how many frames does it complete?
    // They are walked on the object and put back if the frames they promise cannot be delivered (launch, copy or status
    // failure): a caller that retries then gets the same frames instead of skipping them.
    const hca::StreamCounters saved = st->counters;
    auto roll_back = [&](int rc) {
        st->chunks_fed = saved_fed;
        st->counters = saved;
        *frames_output = 0;
        return rc;
    };
    const int first = saved.frames_processed;
    const int count = st->counters.advance_one_block(h);
    *frames_output = count;
    if (count == 0) return VGA_OK;
    const uint16_t *pow = nullptr;
    if (int rc = crc_pow_table(&pow)) return roll_back(rc);
    const int64_t ch_pitch = (int64_t)st->chunks * hca::SPF;
    const int64_t frames_pitch = frames_pitch_for(h);
    auto hip_ok = [&](hipError_t e, const char *what) {
        if (e == hipSuccess) return true;
        set_error("%s failed: %s", what, hipGetErrorString(e));
        return false;
    };
    // the status word is this call's: an error of an earlier call was reported by that call
    if (!hip_ok(hipMemsetAsync(st->d_status.p, 0, sizeof(int), st->s), "hipMemsetAsync")) return roll_back(VGA_ERR_DEVICE);
    if (refuse_step(VGA_TESTING_STEP_HCA_STREAM_FRAMES)) {
        set_error("%s", kRefusedStep);
        return roll_back(VGA_ERR_DEVICE);
    }
    if (int rc = hca::launch_encode(st->d_pcm.as<int16_t>(), ch_pitch * st->nch, ch_pitch, 1, st->map, st->dev, st->d_frames.as<uint8_t>(),
                                    frames_pitch, pow, st->d_status.as<int>(), st->s, first, count))
        return roll_back(rc);
    st->host_frames.resize((size_t)count * h.frame_size);
    int status = 0;
    if (!hip_ok(hipMemcpyAsync(st->host_frames.data(), st->d_frames.as<uint8_t>() + (size_t)first * h.frame_size, st->host_frames.size(),
                               hipMemcpyDeviceToHost, st->s), "hipMemcpyAsync") ||
        !hip_ok(hipMemcpyAsync(&status, st->d_status.p, sizeof(int), hipMemcpyDeviceToHost, st->s), "hipMemcpyAsync") ||
        !hip_ok(hipStreamSynchronize(st->s), "hipStreamSynchronize"))
        return roll_back(VGA_ERR_DEVICE);
    if (int rc = status_to_error(status)) return roll_back(rc);
    std::memcpy(hca_out, st->host_frames.data(), (size_t)h.frame_size);
    for (int k = 1; k < count; k++)
        st->pending.emplace_back(st->host_frames.begin() + (size_t)k * h.frame_size, st->host_frames.begin() + (size_t)(k + 1) * h.frame_size);
    return VGA_OK;
}

}  // extern "C"
