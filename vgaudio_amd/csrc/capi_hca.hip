// capi_hca.hip -- C-ABI entry points for CRI HCA (see include/vgaudio_hip.h): the stream parameters, the device-resident
// calls and the host batches of equally shaped streams.  The host-side derivations (CriHcaEncoder.Initialize, channel
// typing, ATH curve) are in hca_host.hpp, the streaming shell in capi_hca_stream.hip, the ragged host batches in
// capi_hca_v.hip, the packed device-resident ones in capi_hca_ragged.hip; the per-frame work is entirely in
// hca_encode_kernel.hip / hca_decode_kernels.hip.
#include "hca_capi.hpp"
#include "hca_frame_crc.hpp"

#include <mutex>

using namespace vga;
using namespace vga::hca;

namespace {

// x^(8k) mod (x^16 + x^15 + x^2 + 1), k = 0..65535 (hca_crc::kPowEntries: any frame a file can declare), uploaded once per device
struct CrcPow {
    std::mutex mu;
    uint16_t *dev[64] = {};
} g_crc_pow;

}  // namespace

extern "C" int vga_testing_hca_device_info(const void *hca_info, void *out, int out_bytes)
{
    if (!hca_info || !out || out_bytes < (int)sizeof(hca::DeviceInfo)) { set_error("bad arguments"); return VGA_ERR_ARGUMENT; }
    hca::DeviceInfo d;
    if (int rc = make_device_info(*static_cast<const vga_hca_info *>(hca_info), d)) return rc;
    memcpy(out, &d, sizeof d);
    return VGA_OK;
}

int vga::hca::crc_pow_table(const uint16_t **out)
{
    int device = 0;
    VGA_HIP_TRY(hipGetDevice(&device));
    if (device < 0 || device >= 64) { set_error("device index out of range"); return VGA_ERR_DEVICE; }
    std::lock_guard<std::mutex> lock(g_crc_pow.mu);
    if (!g_crc_pow.dev[device]) {
        static uint16_t host[hca_crc::kPowEntries];
        unsigned v = 1;                      // x^0
        for (int k = 0; k < hca_crc::kPowEntries; k++) {
            host[k] = (uint16_t)v;
            for (int j = 0; j < 8; j++) v = ((v << 1) ^ ((v & 0x8000u) ? 0x8005u : 0u)) & 0xFFFFu;
        }
        uint16_t *d = nullptr;
        VGA_HIP_TRY(device_malloc(reinterpret_cast<void **>(&d), sizeof host));
        VGA_HIP_TRY(hipMemcpy(d, host, sizeof host, hipMemcpyHostToDevice));
        g_crc_pow.dev[device] = d;
    }
    *out = g_crc_pow.dev[device];
    return VGA_OK;
}

extern "C" {

// CriHcaEncoder.Initialize (CriHcaEncoder.cs:61-114)
int vga_hca_encoder_initialize(const vga_hca_params *c, vga_hca_info *h) { return encoder_initialize(c, h); }

size_t vga_hca_decode_workspace_bytes(const vga_hca_info *h, int nstreams)
{
    if (!h || nstreams <= 0 || h->frame_count <= 0 || h->channel_count < 1 || h->channel_count > 8) return 0;
    hca::DeviceInfo d;
    if (make_device_info(*h, d) != VGA_OK) return 0;
    return hca::decode_record_bytes(d) * (size_t)h->frame_count * (size_t)nstreams;
}

int vga_hca_encode_device(const int16_t *d_pcm, int64_t stream_pitch, int64_t ch_pitch, int nstreams, int pcm_length,
                          const vga_hca_info *h, uint8_t *d_frames, int64_t frames_pitch, int *d_status, void *stream)
{
    if (!h) { set_error("null HcaInfo"); return VGA_ERR_ARGUMENT; }
    if (bitrate_too_low(*h)) { set_error("Bitrate is set too low."); return VGA_ERR_INVALID_DATA; }
    hca::DeviceInfo d;
    if (int rc = make_device_info(*h, d)) return rc;
    if (nstreams < 0 || pcm_length < 0 || (frames_pitch & 1) || frames_pitch < (int64_t)h->frame_count * h->frame_size ||
        ch_pitch < pcm_length || stream_pitch < ch_pitch * h->channel_count) {
        set_error("bad sizes / pitches for vga_hca_encode_device");
        return VGA_ERR_ARGUMENT;
    }
    hca::PcmMap m;
    if (int rc = make_pcm_map(*h, pcm_length, m)) return rc;
    const uint16_t *pow = nullptr;
    if (int rc = crc_pow_table(&pow)) return rc;
    return hca::launch_encode(d_pcm, stream_pitch, ch_pitch, nstreams, m, d, d_frames, frames_pitch, pow,
                              d_status, (hipStream_t)stream);
}

int vga_hca_decode_device(const vga_hca_info *h, const uint8_t *d_frames, int64_t frames_pitch, int nstreams,
                          int16_t *d_pcm, int64_t stream_pitch, int64_t ch_pitch, void *d_workspace,
                          size_t workspace_bytes, int *d_status, void *stream)
{
    if (!h) { set_error("null HcaInfo"); return VGA_ERR_ARGUMENT; }
    hca::DeviceInfo d;
    if (int rc = make_device_info(*h, d)) return rc;
    if (nstreams < 0 || (frames_pitch & 3) || ((uintptr_t)d_frames & 3) ||
        frames_pitch < (int64_t)h->frame_count * h->frame_size + 8 || ch_pitch < h->sample_count ||
        stream_pitch < ch_pitch * h->channel_count || workspace_bytes < vga_hca_decode_workspace_bytes(h, nstreams)) {
        set_error("bad sizes / pitches / workspace for vga_hca_decode_device (frames need 4-byte alignment and 8 bytes of slack)");
        return VGA_ERR_ARGUMENT;
    }
    return hca::launch_decode(d_frames, frames_pitch, nstreams, d, d_pcm, stream_pitch, ch_pitch, d_workspace, d_status,
                              (hipStream_t)stream);
}

// CriHcaFormat.EncodeFromPcm16 (Formats/CriHca/CriHcaFormat.cs:34-84) for a batch of equally shaped streams.
// pcm: nstreams*channel_count planar pointers (stream-major); frames_out[s]: frame_count*frame_size bytes.
static int hca_encode_batch_one(const int16_t *const *pcm, int nstreams, const vga_hca_params *p, vga_hca_info *info_out,
                                uint8_t *const *frames_out);
int vga_hca_encode_batch(const int16_t *const *pcm, int nstreams, const vga_hca_params *p, vga_hca_info *info_out,
                         uint8_t *const *frames_out)
{
    if (nstreams <= 0 || !pcm || !frames_out || !p || p->channel_count < 1 || p->channel_count > 8)
        return hca_encode_batch_one(pcm, nstreams, p, info_out, frames_out);
    const int nch = p->channel_count;
    return for_each_device_share(nstreams, HCA_MIN_SHARE_STREAMS, [&](int first, int count) {
        return hca_encode_batch_one(pcm + (size_t)first * nch, count, p, first == 0 ? info_out : nullptr, frames_out + first);
    });
}
static int hca_encode_batch_one(const int16_t *const *pcm, int nstreams, const vga_hca_params *p, vga_hca_info *info_out,
                                uint8_t *const *frames_out)
{
    vga_hca_info h;
    if (int rc = vga_hca_encoder_initialize(p, &h)) return rc;
    if (info_out) *info_out = h;
    if (nstreams < 0) { set_error("negative stream count"); return VGA_ERR_ARGUMENT; }
    if (nstreams == 0) return VGA_OK;
    if (!pcm || !frames_out) { set_error("null array"); return VGA_ERR_ARGUMENT; }
    const int nch = h.channel_count, n = p->sample_count;
    for (int i = 0; i < nstreams * nch; i++)
        if (!pcm[i] && n > 0) { set_error("pcm[%d] is null", i); return VGA_ERR_ARGUMENT; }
    for (int i = 0; i < nstreams; i++)
        if (!frames_out[i]) { set_error("frames_out[%d] is null", i); return VGA_ERR_ARGUMENT; }
    if (int rc = require_device()) return rc;
    DevBuf d_pcm, d_frames, d_status;
    const int64_t ch_pitch = round_up(n > 0 ? n : 1, 8);
    const int64_t stream_pitch = ch_pitch * nch;
    const int64_t fbytes = (int64_t)h.frame_count * h.frame_size;
    const int64_t frames_pitch = frames_pitch_for(h);
    VGA_HIP_TRY(d_pcm.alloc((size_t)nstreams * stream_pitch * 2));
    VGA_HIP_TRY(d_frames.alloc((size_t)nstreams * frames_pitch));
    if (int rc = alloc_status_word(d_status)) return rc;
    // a unit of the pipeline is a stream: channel_count input rows, one row of frames out (the reference encodes one
    // stream per task, CriHcaFormat.cs:53-81 under Cli/Batch.cs:24-25)
    pipe::Job job;
    job.units = nstreams;
    if (n > 0) {
        job.in_rows_per_unit = nch;
        bind_in(job, (const void *const *)pcm, (size_t)n * 2, d_pcm.as<char>(), (size_t)ch_pitch * 2);
    }
    if (fbytes > 0) bind_out(job, (void *const *)frames_out, (size_t)fbytes, d_frames.as<char>(), (size_t)frames_pitch);
    job.compute_lanes = planned_compute_lanes(1);                       // (nothing per lane)
    job.compute = chunk_compute([&](int first, int count, hipStream_t s) {
        return vga_hca_encode_device(d_pcm.as<int16_t>() + (int64_t)first * stream_pitch, stream_pitch, ch_pitch, count, n, &h,
                                     d_frames.as<uint8_t>() + (int64_t)first * frames_pitch, frames_pitch, d_status.as<int>(), s);
    });
    return run_status_job(job, HCA_CHUNK_STREAMS, d_status);
}

// CriHcaFormat.ToPcm16 (CriHcaFormat.cs:26-32 -> CriHcaDecoder.Decode, CriHcaDecoder.cs:11-29), batched.
static int hca_decode_batch_one(const vga_hca_info *h, const uint8_t *const *frames, int nstreams, int16_t *const *pcm_out);
int vga_hca_decode_batch(const vga_hca_info *h, const uint8_t *const *frames, int nstreams, int16_t *const *pcm_out)
{
    if (nstreams <= 0 || !h || !frames || !pcm_out || h->channel_count < 1 || h->channel_count > 8)
        return hca_decode_batch_one(h, frames, nstreams, pcm_out);
    const int nch = h->channel_count;
    return for_each_device_share(nstreams, HCA_MIN_SHARE_STREAMS, [&](int first, int count) {
        return hca_decode_batch_one(h, frames + first, count, pcm_out + (size_t)first * nch);
    });
}
static int hca_decode_batch_one(const vga_hca_info *h, const uint8_t *const *frames, int nstreams, int16_t *const *pcm_out)
{
    if (!h) { set_error("null HcaInfo"); return VGA_ERR_ARGUMENT; }
    hca::DeviceInfo d;
    if (int rc = make_device_info(*h, d)) return rc;
    if (nstreams < 0 || h->sample_count < 0) { set_error("negative size"); return VGA_ERR_ARGUMENT; }
    if (nstreams == 0) return VGA_OK;
    if (!frames || !pcm_out) { set_error("null array"); return VGA_ERR_ARGUMENT; }
    const int nch = h->channel_count;
    for (int i = 0; i < nstreams; i++)
        if (!frames[i] && h->frame_count > 0) { set_error("frames[%d] is null", i); return VGA_ERR_ARGUMENT; }
    for (int i = 0; i < nstreams * nch; i++)
        if (!pcm_out[i] && h->sample_count > 0) { set_error("pcm_out[%d] is null", i); return VGA_ERR_ARGUMENT; }
    if (int rc = require_device()) return rc;
    DevBuf d_pcm, d_frames, d_status, d_ws;
    const int n = h->sample_count;
    const int64_t ch_pitch = round_up(n > 0 ? n : 1, 8);
    const int64_t stream_pitch = ch_pitch * nch;
    const int64_t fbytes = (int64_t)h->frame_count * h->frame_size;
    const int64_t frames_pitch = frames_pitch_for(*h);
    VGA_HIP_TRY(d_pcm.alloc((size_t)nstreams * stream_pitch * 2));
    VGA_HIP_TRY(hipMemset(d_pcm.p, 0, (size_t)nstreams * stream_pitch * 2));
    VGA_HIP_TRY(d_frames.alloc((size_t)nstreams * frames_pitch));
    VGA_HIP_TRY(hipMemset(d_frames.p, 0, (size_t)nstreams * frames_pitch));     // the 8 bytes of slack behind every stream
    if (int rc = alloc_status_word(d_status)) return rc;
    const size_t wsb = vga_hca_decode_workspace_bytes(h, nstreams);
    VGA_HIP_TRY(d_ws.alloc(wsb));
    const size_t ws_per_stream = nstreams > 0 ? wsb / (size_t)nstreams : 0;
    pipe::Job job;
    job.units = nstreams;
    if (fbytes > 0) bind_in(job, (const void *const *)frames, (size_t)fbytes, d_frames.as<char>(), (size_t)frames_pitch);
    if (n > 0) {
        job.out_rows_per_unit = nch;
        bind_out(job, (void *const *)pcm_out, (size_t)n * 2, d_pcm.as<char>(), (size_t)ch_pitch * 2);
    }
    job.compute_lanes = planned_compute_lanes(1);                       // (nothing per lane)
    job.compute = chunk_compute([&](int first, int count, hipStream_t s) {
        return vga_hca_decode_device(h, d_frames.as<uint8_t>() + (int64_t)first * frames_pitch, frames_pitch, count,
                                     d_pcm.as<int16_t>() + (int64_t)first * stream_pitch, stream_pitch, ch_pitch,
                                     d_ws.as<char>() + (size_t)first * ws_per_stream, (size_t)count * ws_per_stream,
                                     d_status.as<int>(), s);
    });
    return run_status_job(job, HCA_CHUNK_STREAMS, d_status);
}

}  // extern "C"
