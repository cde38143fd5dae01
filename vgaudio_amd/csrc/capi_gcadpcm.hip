// capi_gcadpcm.hip -- C-ABI entry points for GC-ADPCM (see include/vgaudio_hip.h): the GcAdpcmMath exports, the device calls,
// the equal-length host batches and the dsptool-compatible exports.  Channel metadata and the DSP container are in
// capi_gc_channels.hip, ragged batches in capi_gcadpcm_v.hip; the library-wide state is in runtime.hip.
#include "gc_capi.hpp"
#include "../../include/vgaudio_hip_testing.h"

using namespace vga;

extern "C" {

int vga_testing_gc_plan_pieces(int cus, int groups, int frames, long long group_frames, int ragged, int *out5)
{
    if (!out5 || cus <= 0 || groups <= 0 || frames <= 0) return -1;
    bool persistent = false;
    gc::Pieces seg;
    // (1: the schedule of the self-served shape -- out5 holds two sizes: on uniform batches the schedule of the groups that keep
    // the coarse tail, which is the only one wherever the tail does not descend; vga_testing_gc_plan_pieces_n has both)
    const int segments = gc::plan_encode_pieces_on(cus, groups, frames, group_frames, ragged != 0, &persistent, &seg,
                                                     encoder_layout() == 1 ? 1 : 8);
    out5[0] = segments;
    out5[1] = seg.big;
    out5[2] = seg.nb;
    out5[3] = seg.small;
    out5[4] = persistent ? 1 : 0;
    return 0;
}

int vga_testing_gc_plan_pieces_n(int cus, int groups, int frames, long long group_frames, int ragged, int coarse, int *out10)
{
    if (!out10 || cus <= 0 || groups <= 0 || frames <= 0) return -1;
    bool persistent = false;
    gc::TailPieces seg;
    const int segments = gc::plan_encode_tail_pieces_on(cus, groups, frames, group_frames, ragged != 0, &persistent, &seg,
                                                          encoder_layout() == 1 ? 1 : 8, coarse != 0);
    const int out[10] = {segments, seg.big, seg.nb, seg.small, seg.n1, seg.s2, seg.n2, seg.s3, persistent ? 1 : 0, 0};
    for (int i = 0; i < 10; i++) out10[i] = out[i];
    return 0;
}

// GcAdpcmMath.cs:11-47 (gc_host.hpp)
int vga_gcadpcm_nibble_count_to_sample_count(int nibble_count) { return gc::nibble_count_to_sample_count(nibble_count); }
int vga_gcadpcm_sample_count_to_nibble_count(int sample_count) { return gc::sample_count_to_nibble_count(sample_count); }
int vga_gcadpcm_nibble_to_sample(int nibble) { return gc::nibble_to_sample(nibble); }
int vga_gcadpcm_sample_to_nibble(int sample) { return gc::sample_to_nibble(sample); }
int vga_gcadpcm_sample_count_to_byte_count(int sample_count) { return gc::sample_count_to_byte_count(sample_count); }
int vga_gcadpcm_byte_count_to_sample_count(int byte_count) { return gc::byte_count_to_sample_count(byte_count); }

// ---------------------------------------------------------------- device-resident
size_t vga_gcadpcm_coefs_workspace_bytes(int nch, int length)
{
    if (nch <= 0 || length < 0) return 0;
    const size_t frames = ((size_t)length + 13) / 14;
    return (size_t)nch * (size_t)vga::gc::coef_record_pitch((int64_t)frames) * 16;
}

int vga_gcadpcm_coefs_device(const int16_t *d_pcm, int64_t pcm_pitch, int nch, int length, int16_t *d_coefs,
                             void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (nch < 0 || length < 0) { set_error("negative size"); return VGA_ERR_ARGUMENT; }
    if (nch == 0) return VGA_OK;
    if (int rc = gc::check_pcm_layout(d_pcm, pcm_pitch, length, "vga_gcadpcm_coefs_device")) return rc;
    if (workspace_bytes < vga_gcadpcm_coefs_workspace_bytes(nch, length) || !d_workspace) {
        set_error("workspace too small: need %zu bytes", vga_gcadpcm_coefs_workspace_bytes(nch, length));
        return VGA_ERR_ARGUMENT;
    }
    return gc::launch_coefs(d_pcm, pcm_pitch, nch, length, d_coefs, d_workspace, (hipStream_t)stream);
}

int vga_gcadpcm_encode_device(const int16_t *d_pcm, int64_t pcm_pitch, int nch, int sample_count,
                              const int16_t *d_coefs, const int16_t *d_hist1, const int16_t *d_hist2,
                              uint8_t *d_adpcm, int64_t adpcm_pitch, void *stream)
{
    if (nch < 0 || sample_count < 0) { set_error("negative size"); return VGA_ERR_ARGUMENT; }
    if (nch == 0 || sample_count == 0) return VGA_OK;
    if (int rc = gc::check_pcm_layout(d_pcm, pcm_pitch, sample_count, "vga_gcadpcm_encode_device")) return rc;
    if (int rc = gc::check_adpcm_layout(d_adpcm, adpcm_pitch, gc::sample_count_to_byte_count(sample_count),
                                    "vga_gcadpcm_encode_device"))
        return rc;
    return gc::launch_encode(d_pcm, pcm_pitch, nch, sample_count, d_coefs, d_hist1, d_hist2, d_adpcm, adpcm_pitch,
                             (hipStream_t)stream);
}

int vga_gcadpcm_decode_device(const uint8_t *d_adpcm, int64_t adpcm_pitch, const int16_t *d_coefs, int nch,
                              int sample_count, const int16_t *d_hist1, const int16_t *d_hist2, int16_t *d_pcm,
                              int64_t pcm_pitch, int *d_status, void *stream)
{
    if (nch < 0 || sample_count < 0) { set_error("negative size"); return VGA_ERR_ARGUMENT; }
    if (nch == 0 || sample_count == 0) return VGA_OK;
    if (int rc = gc::check_pcm_layout(d_pcm, pcm_pitch, sample_count, "vga_gcadpcm_decode_device")) return rc;
    if (int rc = gc::check_adpcm_layout(d_adpcm, adpcm_pitch, gc::sample_count_to_byte_count(sample_count),
                                    "vga_gcadpcm_decode_device"))
        return rc;
    return gc::launch_decode(d_adpcm, adpcm_pitch, d_coefs, nch, sample_count, d_hist1, d_hist2, d_pcm, pcm_pitch,
                             d_status, (hipStream_t)stream);
}

int vga_synth_pcm16_device(int16_t *d_pcm, int64_t pcm_pitch, int nch, int length, int first_channel,
                           const uint32_t *d_params, void *stream)
{
    if (nch < 0 || length < 0 || pcm_pitch < length) { set_error("bad synth arguments"); return VGA_ERR_ARGUMENT; }
    return gc::launch_synth(d_pcm, pcm_pitch, nch, length, first_channel, d_params, (hipStream_t)stream);
}

// ---------------------------------------------------------------- host-buffer batch API
// Channels per pipeline chunk (LABNOTES.md 5, host path): small enough that the first kernels start after a quarter
// of configs[1] has arrived, large enough that the coefficient kernel (one wave per channel) still has a wave per SIMD.
static constexpr int GC_CHUNK_CHANNELS = 1024;

static int calculate_coefficients_batch_one(const int16_t *const *pcm, int nch, int length, int16_t *coefs_out)
{
    if (length < 0) { set_error("negative length"); return VGA_ERR_ARGUMENT; }
    if (int rc = gc::check_ptrs((const void *const *)pcm, length > 0 ? nch : 0, "pcm")) return rc;
    if (nch < 0 || (nch > 0 && !coefs_out)) { set_error("bad coefs_out/nch"); return VGA_ERR_ARGUMENT; }
    if (nch == 0) return VGA_OK;
    if (int rc = require_device()) return rc;
    gc::GcBatch b;
    b.pcm_pitch = round_up(length > 0 ? length : 1, 8);
    VGA_HIP_TRY(b.pcm.alloc((size_t)nch * b.pcm_pitch * sizeof(int16_t)));
    VGA_HIP_TRY(b.coefs.alloc((size_t)nch * 32));
    pipe::Job job;
    job.units = nch;
    if (length > 0) bind_in(job, (const void *const *)pcm, (size_t)length * sizeof(int16_t), b.pcm.as<char>(), (size_t)b.pcm_pitch * sizeof(int16_t));
    job.compute = chunk_compute([&](int first, int count, hipStream_t s) {
        return gc::launch_coefs(b.pcm.as<int16_t>() + (int64_t)first * b.pcm_pitch, b.pcm_pitch, count, length,
                                b.coefs.as<int16_t>() + (int64_t)first * 16, b.ws.p, s);
    });
    // one chunk's workspace: the chunks' kernels run one after the other on the compute stream (one lane, whatever the
    // lanes hook says)
    VGA_HIP_TRY(b.ws.alloc(vga_gcadpcm_coefs_workspace_bytes(planned_chunk_units(job, GC_CHUNK_CHANNELS), length)));
    if (int rc = run_batch_pipeline(job, GC_CHUNK_CHANNELS)) return rc;
    VGA_HIP_TRY(hipMemcpy(coefs_out, b.coefs.p, (size_t)nch * 32, hipMemcpyDeviceToHost));
    return VGA_OK;
}

int vga_gcadpcm_calculate_coefficients_batch(const int16_t *const *pcm, int nch, int length, int16_t *coefs_out)
{
    if (nch <= 0 || !pcm || !coefs_out) return calculate_coefficients_batch_one(pcm, nch, length, coefs_out);
    return for_each_device_share(nch, gc::GC_MIN_SHARE_CHANNELS, [&](int first, int count) {
        return calculate_coefficients_batch_one(pcm + first, count, length, coefs_out + (size_t)first * 16);
    });
}

static int encode_with_coefs_batch_one(const int16_t *const *pcm, int nch, int pcm_length, int sample_count, const int16_t *coefs,
                                      const int16_t *hist1, const int16_t *hist2, uint8_t *const *adpcm_out)
{
    if (sample_count == -1) sample_count = pcm_length;
    if (pcm_length < 0 || sample_count < 0) { set_error("negative length"); return VGA_ERR_ARGUMENT; }
    if (sample_count > pcm_length) {
        set_error("SampleCount (%d) exceeds pcm length (%d)", sample_count, pcm_length);
        return VGA_ERR_ARGUMENT;
    }
    if (int rc = gc::check_ptrs((const void *const *)pcm, sample_count > 0 ? nch : 0, "pcm")) return rc;
    if (int rc = gc::check_ptrs((const void *const *)adpcm_out, sample_count > 0 ? nch : 0, "adpcm_out")) return rc;
    if (nch > 0 && !coefs) { set_error("null coefs"); return VGA_ERR_ARGUMENT; }
    if (nch <= 0 || sample_count == 0) return nch < 0 ? VGA_ERR_ARGUMENT : VGA_OK;
    if (int rc = require_device()) return rc;
    gc::GcBatch b;
    VGA_HIP_TRY(b.st.create());
    b.pcm_pitch = round_up(sample_count, 8);
    VGA_HIP_TRY(b.pcm.alloc((size_t)nch * b.pcm_pitch * sizeof(int16_t)));
    if (int rc = gc::upload_hist(b.h1, b.h2, nch, hist1, hist2, &b.st)) return rc;
    VGA_HIP_TRY(b.coefs.alloc((size_t)nch * 32));
    VGA_HIP_TRY(hipMemcpyAsync(b.coefs.p, coefs, (size_t)nch * 32, hipMemcpyHostToDevice, b.st.s));
    VGA_HIP_TRY(hipStreamSynchronize(b.st.s));
    const int nbytes = gc::sample_count_to_byte_count(sample_count);
    b.adpcm_pitch = round_up(nbytes, 16);
    VGA_HIP_TRY(b.adpcm.alloc((size_t)nch * b.adpcm_pitch));
    DevBuf scratch;                                       // the encoder's piece states: one chunk at a time uses it (one lane)
    pipe::Job job;
    job.units = nch;
    bind_in(job, (const void *const *)pcm, (size_t)sample_count * sizeof(int16_t), b.pcm.as<char>(), (size_t)b.pcm_pitch * sizeof(int16_t));
    bind_out(job, (void *const *)adpcm_out, (size_t)nbytes, b.adpcm.as<char>(), (size_t)b.adpcm_pitch);
    job.compute = chunk_compute([&](int first, int count, hipStream_t s) {
        return gc::launch_encode(b.pcm.as<int16_t>() + (int64_t)first * b.pcm_pitch, b.pcm_pitch, count, sample_count,
                                 b.coefs.as<int16_t>() + (int64_t)first * 16,
                                 b.h1.p ? b.h1.as<int16_t>() + first : nullptr, b.h2.p ? b.h2.as<int16_t>() + first : nullptr,
                                 b.adpcm.as<uint8_t>() + (int64_t)first * b.adpcm_pitch, b.adpcm_pitch, s, scratch.p, scratch.bytes);
    });
    VGA_HIP_TRY(scratch.alloc(gc::encode_scratch_bytes(planned_chunk_units(job, GC_CHUNK_CHANNELS))));
    return run_batch_pipeline(job, GC_CHUNK_CHANNELS);
}

int vga_gcadpcm_encode_with_coefs_batch(const int16_t *const *pcm, int nch, int pcm_length, int sample_count,
                                        const int16_t *coefs, const int16_t *hist1, const int16_t *hist2,
                                        uint8_t *const *adpcm_out)
{
    if (nch <= 0 || !pcm || !coefs || !adpcm_out)
        return encode_with_coefs_batch_one(pcm, nch, pcm_length, sample_count, coefs, hist1, hist2, adpcm_out);
    return for_each_device_share(nch, gc::GC_MIN_SHARE_CHANNELS, [&](int first, int count) {
        return encode_with_coefs_batch_one(pcm + first, count, pcm_length, sample_count, coefs + (size_t)first * 16,
                                          hist1 ? hist1 + first : nullptr, hist2 ? hist2 + first : nullptr, adpcm_out + first);
    });
}

static int encode_batch_one(const int16_t *const *pcm, int nch, int sample_count, int16_t hist1, int16_t hist2, int16_t *coefs_out,
                           uint8_t *const *adpcm_out)
{
    if (sample_count < 0) { set_error("negative sample count"); return VGA_ERR_ARGUMENT; }
    if (int rc = gc::check_ptrs((const void *const *)pcm, sample_count > 0 ? nch : 0, "pcm")) return rc;
    if (int rc = gc::check_ptrs((const void *const *)adpcm_out, sample_count > 0 ? nch : 0, "adpcm_out")) return rc;
    if (nch < 0 || (nch > 0 && !coefs_out)) { set_error("bad coefs_out/nch"); return VGA_ERR_ARGUMENT; }
    if (nch == 0) return VGA_OK;
    if (int rc = require_device()) return rc;
    const double t_entry = pipe::detail::now();
    gc::GcBatch b;
    VGA_HIP_TRY(b.st.create());
    b.pcm_pitch = round_up(sample_count > 0 ? sample_count : 1, 8);
    VGA_HIP_TRY(b.pcm.alloc((size_t)nch * b.pcm_pitch * sizeof(int16_t)));
    std::vector<int16_t> h1v((size_t)nch, hist1), h2v((size_t)nch, hist2);
    const bool use_hist = hist1 != 0 || hist2 != 0;
    if (use_hist)
        if (int rc = gc::upload_hist(b.h1, b.h2, nch, h1v.data(), h2v.data(), &b.st)) return rc;
    VGA_HIP_TRY(hipStreamSynchronize(b.st.s));
    VGA_HIP_TRY(b.coefs.alloc((size_t)nch * 32));
    const int nbytes = gc::sample_count_to_byte_count(sample_count);
    b.adpcm_pitch = round_up(nbytes > 0 ? nbytes : 1, 16);
    VGA_HIP_TRY(b.adpcm.alloc((size_t)nch * b.adpcm_pitch));
    // two compute lanes: a chunk's kernels need not wait for the chunk before (the short chunks at the end of the upload
    // are bound by the latency of one channel's coefficient search, ~25 ms, not by the chip); each lane has its own
    // piece states and workspace.  A lane more than the queues hold would stall the copies.  One channel is one chunk: one lane.
    DevBuf scratch[pipe::kMaxComputeLanes], ws[pipe::kMaxComputeLanes];
    pipe::Job job;
    job.units = nch;
    job.compute_lanes = nch > 1 ? planned_compute_lanes(hardware_queues_requested() >= 6 ? 2 : 1) : 1;
    if (sample_count > 0) {
        bind_in(job, (const void *const *)pcm, (size_t)sample_count * sizeof(int16_t), b.pcm.as<char>(), (size_t)b.pcm_pitch * sizeof(int16_t));
        bind_out(job, (void *const *)adpcm_out, (size_t)nbytes, b.adpcm.as<char>(), (size_t)b.adpcm_pitch);
    }
    // EncodeChannel (GcAdpcmFormat.cs:129-135): coefficients, then encode -- per chunk of channels, so that the next
    // chunk's upload and the previous chunk's download overlap these kernels
    job.compute = chunk_compute([&](int first, int count, hipStream_t s) {
        const int lane = pipe::compute_lane();
        int rc = gc::launch_coefs(b.pcm.as<int16_t>() + (int64_t)first * b.pcm_pitch, b.pcm_pitch, count, sample_count,
                                  b.coefs.as<int16_t>() + (int64_t)first * 16, ws[lane].p, s);
        if (!rc)
            rc = gc::launch_encode(b.pcm.as<int16_t>() + (int64_t)first * b.pcm_pitch, b.pcm_pitch, count, sample_count,
                                   b.coefs.as<int16_t>() + (int64_t)first * 16,
                                   b.h1.p ? b.h1.as<int16_t>() + first : nullptr, b.h2.p ? b.h2.as<int16_t>() + first : nullptr,
                                   b.adpcm.as<uint8_t>() + (int64_t)first * b.adpcm_pitch, b.adpcm_pitch, s, scratch[lane].p,
                                   scratch[lane].bytes);
        return rc;
    });
    const int chunk = planned_chunk_units(job, GC_CHUNK_CHANNELS);
    for (int l = 0; l < job.compute_lanes; l++) {                     // (a single chunk of several channels may be split in two)
        VGA_HIP_TRY(scratch[l].alloc(gc::encode_scratch_bytes(chunk)));
        VGA_HIP_TRY(ws[l].alloc(vga_gcadpcm_coefs_workspace_bytes(chunk, sample_count)));
    }
    pipe_report().t_alloc = pipe::detail::now() - t_entry;
    if (int rc = run_batch_pipeline(job, GC_CHUNK_CHANNELS)) return rc;
    VGA_HIP_TRY(hipMemcpy(coefs_out, b.coefs.p, (size_t)nch * 32, hipMemcpyDeviceToHost));
    pipe_report().t_entry = pipe::detail::now() - t_entry;      // without the buffers' release (the destructors below)
    return VGA_OK;
}

int vga_gcadpcm_encode_batch(const int16_t *const *pcm, int nch, int sample_count, int16_t hist1, int16_t hist2,
                             int16_t *coefs_out, uint8_t *const *adpcm_out)
{
    if (nch <= 0 || !pcm || !coefs_out || !adpcm_out) return encode_batch_one(pcm, nch, sample_count, hist1, hist2, coefs_out, adpcm_out);
    return for_each_device_share(nch, gc::GC_MIN_SHARE_CHANNELS, [&](int first, int count) {
        return encode_batch_one(pcm + first, count, sample_count, hist1, hist2, coefs_out + (size_t)first * 16, adpcm_out + first);
    });
}

static int decode_batch_one(const uint8_t *const *adpcm, const int16_t *coefs, int nch, int sample_count, const int16_t *hist1,
                           const int16_t *hist2, int16_t *const *pcm_out)
{
    if (sample_count < 0) { set_error("negative sample count"); return VGA_ERR_ARGUMENT; }
    if (int rc = gc::check_ptrs((const void *const *)adpcm, sample_count > 0 ? nch : 0, "adpcm")) return rc;
    if (int rc = gc::check_ptrs((const void *const *)pcm_out, sample_count > 0 ? nch : 0, "pcm_out")) return rc;
    if (nch > 0 && !coefs) { set_error("null coefs"); return VGA_ERR_ARGUMENT; }
    if (nch <= 0 || sample_count == 0) return nch < 0 ? VGA_ERR_ARGUMENT : VGA_OK;
    if (int rc = require_device()) return rc;
    gc::GcBatch b;
    VGA_HIP_TRY(b.st.create());
    const int nbytes = gc::sample_count_to_byte_count(sample_count);
    b.adpcm_pitch = round_up(nbytes, 16);
    b.pcm_pitch = round_up(sample_count, 8);
    VGA_HIP_TRY(b.adpcm.alloc((size_t)nch * b.adpcm_pitch));
    VGA_HIP_TRY(b.pcm.alloc((size_t)nch * b.pcm_pitch * 2));
    VGA_HIP_TRY(b.coefs.alloc((size_t)nch * 32));
    VGA_HIP_TRY(b.status.alloc(sizeof(int)));
    VGA_HIP_TRY(hipMemsetAsync(b.status.p, 0, sizeof(int), b.st.s));
    VGA_HIP_TRY(hipMemcpyAsync(b.coefs.p, coefs, (size_t)nch * 32, hipMemcpyHostToDevice, b.st.s));
    if (int rc = gc::upload_hist(b.h1, b.h2, nch, hist1, hist2, &b.st)) return rc;
    VGA_HIP_TRY(hipStreamSynchronize(b.st.s));
    pipe::Job job;
    job.units = nch;
    bind_in(job, (const void *const *)adpcm, (size_t)nbytes, b.adpcm.as<char>(), (size_t)b.adpcm_pitch);
    bind_out(job, (void *const *)pcm_out, (size_t)sample_count * 2, b.pcm.as<char>(), (size_t)b.pcm_pitch * 2);
    job.compute_lanes = planned_compute_lanes(1);                       // (nothing per lane)
    job.compute = chunk_compute([&](int first, int count, hipStream_t s) {
        return gc::launch_decode(b.adpcm.as<uint8_t>() + (int64_t)first * b.adpcm_pitch, b.adpcm_pitch,
                                 b.coefs.as<int16_t>() + (int64_t)first * 16, count, sample_count,
                                 b.h1.p ? b.h1.as<int16_t>() + first : nullptr, b.h2.p ? b.h2.as<int16_t>() + first : nullptr,
                                 b.pcm.as<int16_t>() + (int64_t)first * b.pcm_pitch, b.pcm_pitch, b.status.as<int>(), s);
    });
    return run_status_job(job, 2 * GC_CHUNK_CHANNELS, b.status, gc::BAD_PREDICTOR);
}

int vga_gcadpcm_decode_batch(const uint8_t *const *adpcm, const int16_t *coefs, int nch, int sample_count,
                             const int16_t *hist1, const int16_t *hist2, int16_t *const *pcm_out)
{
    if (nch <= 0 || !adpcm || !coefs || !pcm_out) return decode_batch_one(adpcm, coefs, nch, sample_count, hist1, hist2, pcm_out);
    return for_each_device_share(nch, gc::GC_MIN_SHARE_CHANNELS, [&](int first, int count) {
        return decode_batch_one(adpcm + first, coefs + (size_t)first * 16, count, sample_count, hist1 ? hist1 + first : nullptr,
                               hist2 ? hist2 + first : nullptr, pcm_out + first);
    });
}

// ---------------------------------------------------------------- dsptool-compatible exports
// VGAudio.Tools/GcAdpcm/DspToolDll.cs:16-29,94-108.  void-returning like the DLLs:
// failures leave outputs untouched and are reported through vga_last_error().
void correlateCoefs(int16_t *src, uint32_t samples, int16_t *coefsOut)
{
    const int16_t *chans[1] = {src};
    (void)vga_gcadpcm_calculate_coefficients_batch(chans, 1, (int)samples, coefsOut);
}

void encode(int16_t *src, uint8_t *dst, ADPCMINFO *cxt, uint32_t samples)
{
    const int16_t *chans[1] = {src};
    uint8_t *outs[1] = {dst};
    int16_t coefs[16];
    if (vga_gcadpcm_encode_batch(chans, 1, (int)samples, 0, 0, coefs, outs) != VGA_OK) return;
    if (cxt) {
        memset(cxt, 0, sizeof *cxt);
        memcpy(cxt->coef, coefs, sizeof coefs);
        cxt->pred_scale = samples ? dst[0] : 0;
    }
}

void decode(uint8_t *src, int16_t *dst, ADPCMINFO *cxt, uint32_t samples)
{
    if (!cxt) return;
    const uint8_t *ins[1] = {src};
    int16_t *outs[1] = {dst};
    int16_t coefs[16];
    memcpy(coefs, cxt->coef, sizeof coefs);
    const int16_t h1 = cxt->yn1, h2 = cxt->yn2;
    (void)vga_gcadpcm_decode_batch(ins, coefs, 1, (int)samples, &h1, &h2, outs);
}

void encodeFrame(int16_t *src, uint8_t *dst, int16_t *coefs, uint8_t one)
{
    (void)one;
    // DspEncodeFrame (GcAdpcmEncoder.cs:48-94): src[0..1] history, src[2..15] in/out
    const int16_t *chans[1] = {src + 2};
    uint8_t *outs[1] = {dst};
    const int16_t h2 = src[0], h1 = src[1];
    if (vga_gcadpcm_encode_with_coefs_batch(chans, 1, 14, 14, coefs, &h1, &h2, outs) != VGA_OK) return;
    // the encoder's reconstruction equals the decoder's output (:156-160 vs GcAdpcmDecoder.cs:40-44)
    const uint8_t *ins[1] = {dst};
    int16_t *rec[1] = {src + 2};
    (void)vga_gcadpcm_decode_batch(ins, coefs, 1, 14, &h1, &h2, rec);
}

}  // extern "C"
