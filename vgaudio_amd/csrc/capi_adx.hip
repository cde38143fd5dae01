// capi_adx.hip -- C-ABI entry points for CRI ADX (see include/vgaudio_hip.h): the defaults, the conversions, the two device calls and
// the two equal-length host batches (ragged host batches: capi_adx_v.hip).  Every check and size comes from adx_host.hpp.
#include "adx_capi.hpp"

using namespace vga;

extern "C" {

void vga_adx_default_params(vga_adx_params *p)
{
    if (!p) return;
    p->sample_rate = 48000; p->highpass_frequency = 500; p->frame_size = 18; p->version = 4;
    p->history = 0; p->padding = 0; p->type = 3; p->filter = 0;
}

int vga_adx_calculate_coefficients(int highpass_freq, int sample_rate, int16_t *coefs_out)
{
    if (!coefs_out || sample_rate <= 0) { set_error("bad arguments"); return VGA_ERR_ARGUMENT; }
    adx::calculate_coefficients(highpass_freq, sample_rate, coefs_out);
    return VGA_OK;
}

int vga_adx_nibble_count_to_sample_count(int nibble_count, int frame_size) { return adx::nibble_count_to_sample_count(nibble_count, frame_size); }
int vga_adx_sample_count_to_nibble_count(int sample_count, int frame_size) { return adx::sample_count_to_nibble_count(sample_count, frame_size); }
int vga_adx_sample_count_to_byte_count(int sample_count, int frame_size) { return adx::sample_count_to_byte_count(sample_count, frame_size); }

int vga_adx_encoded_byte_count(int pcm_length, const vga_adx_params *p)
{
    return adx::validate(p) != VGA_OK || pcm_length < 0 ? VGA_ERR_ARGUMENT : adx::encoded_byte_count(pcm_length, *p);
}

int vga_adx_encode_device(const int16_t *d_pcm, int64_t pcm_pitch, int nch, int pcm_length, const vga_adx_params *p,
                          uint8_t *d_out, int64_t out_pitch, int16_t *d_history_out, void *stream)
{
    if (int rc = adx::check_encode(p, nch, pcm_length)) return rc;
    if (nch == 0) return VGA_OK;
    if (int rc = adx::check_encode_device_layout(pcm_pitch, pcm_length, d_out, out_pitch, adx::encoded_byte_count(pcm_length, *p))) return rc;
    return adx::launch_encode(d_pcm, pcm_pitch, nch, pcm_length, adx::make_device_params(p, true), d_out, out_pitch,
                              d_history_out, (hipStream_t)stream);
}

int vga_adx_decode_device(const uint8_t *d_adpcm, int64_t in_pitch, int adpcm_length, int nch, int sample_count,
                          const vga_adx_params *p, int16_t *d_pcm, int64_t pcm_pitch, int *d_status, void *stream)
{
    if (int rc = adx::check_decode(p, adpcm_length, nch, sample_count, in_pitch, pcm_pitch)) return rc;
    if (nch == 0 || sample_count == 0) return VGA_OK;
    return adx::launch_decode(d_adpcm, in_pitch, nch, sample_count, adx::make_device_params(p, false), d_pcm, pcm_pitch, d_status,
                              (hipStream_t)stream);
}

static int adx_encode_batch_one(const int16_t *const *pcm, int nch, int pcm_length, const vga_adx_params *p, uint8_t *const *out,
                                int16_t *history_out)
{
    if (int rc = adx::check_encode(p, nch, pcm_length, true, pcm, out)) return rc;
    if (nch == 0) return VGA_OK;
    if (int rc = require_device()) return rc;
    DevBuf d_pcm, d_out, d_hist;
    const int64_t pcm_pitch = round_up(pcm_length > 0 ? pcm_length : 1, 8);
    const int nbytes = adx::encoded_byte_count(pcm_length, *p);
    const int64_t out_pitch = round_up(nbytes > 0 ? nbytes : 2, 16);
    VGA_HIP_TRY(d_pcm.alloc((size_t)nch * pcm_pitch * 2));
    VGA_HIP_TRY(d_out.alloc((size_t)nch * out_pitch));
    VGA_HIP_TRY(d_hist.alloc((size_t)nch * 2));
    const adx::AdxDeviceParams dp = adx::make_device_params(p, true);
    pipe::Job job;
    job.units = nch;
    if (pcm_length > 0) bind_in(job, (const void *const *)pcm, (size_t)pcm_length * 2, d_pcm.as<char>(), (size_t)pcm_pitch * 2);
    if (nbytes > 0) bind_out(job, (void *const *)out, (size_t)nbytes, d_out.as<char>(), (size_t)out_pitch);
    job.compute_lanes = planned_compute_lanes(1);                       // (nothing per lane)
    job.compute = chunk_compute([&](int first, int count, hipStream_t s) {
        return adx::launch_encode(d_pcm.as<int16_t>() + (int64_t)first * pcm_pitch, pcm_pitch, count, pcm_length, dp,
                                  d_out.as<uint8_t>() + (int64_t)first * out_pitch, out_pitch, d_hist.as<int16_t>() + first, s);
    });
    if (int rc = run_batch_pipeline(job, adx::ADX_CHUNK_CHANNELS)) return rc;
    if (history_out) VGA_HIP_TRY(hipMemcpy(history_out, d_hist.p, (size_t)nch * 2, hipMemcpyDeviceToHost));
    return VGA_OK;
}

int vga_adx_encode_batch(const int16_t *const *pcm, int nch, int pcm_length, const vga_adx_params *p,
                         uint8_t *const *out, int16_t *history_out)
{
    return adx::for_each_share(nch, pcm && out, [&](int first, int count) {
        return adx_encode_batch_one(pcm + first, count, pcm_length, p, out + first, history_out ? history_out + first : nullptr);
    });
}

static int adx_decode_batch_one(const uint8_t *const *adpcm, int adpcm_length, int nch, int sample_count, const vga_adx_params *p,
                                int16_t *const *pcm_out)
{
    if (int rc = adx::check_decode(p, adpcm_length, nch, sample_count, adpcm_length, sample_count, true, adpcm, pcm_out)) return rc;
    if (nch == 0 || sample_count == 0) return VGA_OK;
    if (int rc = require_device()) return rc;
    DevBuf d_in, d_pcm, d_status;
    const int64_t in_pitch = round_up(adpcm_length, 16);
    const int64_t pcm_pitch = round_up(sample_count, 8);
    VGA_HIP_TRY(d_in.alloc((size_t)nch * in_pitch));
    VGA_HIP_TRY(d_pcm.alloc((size_t)nch * pcm_pitch * 2));
    VGA_HIP_TRY(d_status.alloc(sizeof(int)));
    VGA_HIP_TRY(hipMemset(d_status.p, 0, sizeof(int)));
    const adx::AdxDeviceParams dp = adx::make_device_params(p, false);
    pipe::Job job;
    job.units = nch;
    bind_in(job, (const void *const *)adpcm, (size_t)adpcm_length, d_in.as<char>(), (size_t)in_pitch);
    bind_out(job, (void *const *)pcm_out, (size_t)sample_count * 2, d_pcm.as<char>(), (size_t)pcm_pitch * 2);
    job.compute_lanes = planned_compute_lanes(1);                       // (nothing per lane)
    job.compute = chunk_compute([&](int first, int count, hipStream_t s) {
        return adx::launch_decode(d_in.as<uint8_t>() + (int64_t)first * in_pitch, in_pitch, count, sample_count, dp,
                                  d_pcm.as<int16_t>() + (int64_t)first * pcm_pitch, pcm_pitch, d_status.as<int>(), s);
    });
    return adx::run_decode_job(job, d_status);
}

int vga_adx_decode_batch(const uint8_t *const *adpcm, int adpcm_length, int nch, int sample_count,
                         const vga_adx_params *p, int16_t *const *pcm_out)
{
    return adx::for_each_share(nch, adpcm && pcm_out, [&](int first, int count) {
        return adx_decode_batch_one(adpcm + first, adpcm_length, count, sample_count, p, pcm_out + first);
    });
}

}  // extern "C"
