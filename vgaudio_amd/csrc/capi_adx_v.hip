// capi_adx_v.hip -- the ragged host-pointer entry points of CRI ADX (VGAudio.Cli/Batch.cs:24-25: a worker per FILE).
// Every channel with its own length and its own CriAdxParameters (a file's sample rate sets the high-pass coefficients,
// CriAdxCodec.cs:64): the channels are sorted into buckets of one parameter set and similar length (host_batch.hpp,
// plan_buckets), a bucket's rows are zero-padded on the device to its longest channel and run through the equal-length
// kernels; every channel receives the prefix that is its own encoding / decoding.
#include "adx_capi.hpp"

using namespace vga;

static int adx_encode_batch_v_one(const int16_t *const *pcm, const int *lengths, int nch, const vga_adx_params *params, uint8_t *const *out,
                                  int16_t *history_out)
{
    if (int rc = adx::check_encode_v(pcm, lengths, nch, params, out)) return rc;
    if (nch == 0) return VGA_OK;
    std::vector<adx::AdxDeviceParams> dps;
    std::vector<int> group(nch), length(lengths, lengths + nch);
    for (int c = 0; c < nch; c++)
        // An empty channel keeps buckets of its own: with padding % samplesPerFrame != 0 the reference SKIPS the frame in
        // which the padding ends (`if (samplesToCopy == 0) continue`, CriAdxCodec.cs:84) and leaves zero bytes there, while
        // the zero-padded run of a longer bucket would encode silence into it (a non-zero header for the Exponential and
        // Fixed types) -- the one case in which a channel's output is not a prefix of the padded channel's.
        group[c] = 2 * adx::group_of(dps, adx::make_device_params(&params[c], true)) + (lengths[c] == 0 ? 1 : 0);
    if (int rc = require_device()) return rc;
    // chunks of at most 256 channels: what is left after the upload (the last, largest chunk's kernels and its download) is
    // shorter, and the equal-length kernels still fill their launch (10 008 files: 578 ms against 591-601 with 1024, 647-651
    // with 128 -- 79 launches of ~10 ms are more than the upload hides; profiles/r05_q_ragged_host_orders.log)
    const BucketPlan plan = plan_buckets(group, length, 256, adx::ADX_BUCKET_VOLUME, false);
    const BucketLayout lay = layout_buckets(
        plan, 1, 1,
        [&](int k) {
            const vga_adx_params *p = &params[plan.order[plan.chunk_begin[k]]];
            return RowPitch{round_up(std::max(plan.chunk_length[k], 1), 8) * 2,
                            round_up(std::max(adx::encoded_byte_count(plan.chunk_length[k], *p), 2), 16)};
        },
        [&](int c, int) { return InRow{pcm[c], (size_t)lengths[c] * 2}; },
        [&](int c, int) { return OutRow{out[c], (size_t)adx::encoded_byte_count(lengths[c], params[c])}; });
    DevBuf d_pcm, d_out, d_hist, d_own;
    // every channel's own frame count, in the plan's order: the seams in a channel's padding are left alone (adx_kernels.hpp)
    std::vector<int> own(nch);
    for (int i = 0; i < nch; i++) own[i] = adx::own_frames(lengths[plan.order[i]], params[plan.order[i]]);
    VGA_HIP_TRY(d_own.alloc((size_t)nch * sizeof(int)));
    VGA_HIP_TRY(hipMemcpy(d_own.p, own.data(), (size_t)nch * sizeof(int), hipMemcpyHostToDevice));
    if (int rc = lay.alloc(d_pcm, d_out)) return rc;                                    // the padding behind every row is silence
    VGA_HIP_TRY(d_hist.alloc((size_t)nch * 2));
    pipe::Job job;
    job.units = nch;
    lay.bind(job, d_pcm, d_out);
    job.compute_lanes = planned_compute_lanes(1);                       // (nothing per lane)
    job.compute = chunk_compute([&](int first, int count, hipStream_t s) {
        const int k = plan.chunk_of(first);
        return adx::launch_encode(d_pcm.as<int16_t>() + lay.in.base[k] / 2, lay.in.pitch[k] / 2, count, plan.chunk_length[k],
                                  dps[plan.chunk_group[k] / 2], d_out.as<uint8_t>() + lay.out.base[k], lay.out.pitch[k],
                                  d_hist.as<int16_t>() + first, s, d_own.as<int>() + first);
    });
    if (int rc = run_batch_pipeline(job, adx::ADX_CHUNK_CHANNELS)) return rc;
    if (history_out) {
        std::vector<int16_t> h(nch);
        VGA_HIP_TRY(hipMemcpy(h.data(), d_hist.p, (size_t)nch * 2, hipMemcpyDeviceToHost));
        for (int i = 0; i < nch; i++) history_out[plan.order[i]] = h[i];
    }
    return VGA_OK;
}

static int adx_decode_batch_v_one(const uint8_t *const *adpcm, const int *adpcm_lengths, int nch, const int *sample_counts,
                                  const vga_adx_params *params, int16_t *const *pcm_out)
{
    if (int rc = adx::check_decode_v(adpcm, adpcm_lengths, nch, sample_counts, params, pcm_out)) return rc;
    if (nch == 0) return VGA_OK;
    std::vector<adx::AdxDeviceParams> dps;
    std::vector<int> group(nch), length(sample_counts, sample_counts + nch);
    for (int c = 0; c < nch; c++) group[c] = adx::group_of(dps, adx::make_device_params(&params[c], false));
    if (int rc = require_device()) return rc;
    const BucketPlan plan = plan_buckets(group, length, adx::ADX_CHUNK_CHANNELS, adx::ADX_BUCKET_VOLUME, false);
    const BucketLayout lay = layout_buckets(
        plan, 1, 1,
        [&](int k) {
            const int64_t bytes = adx::decode_bytes_read(plan.chunk_length[k], params[plan.order[plan.chunk_begin[k]]]);
            return RowPitch{round_up(std::max<int64_t>(bytes, 2), 16), round_up(std::max(plan.chunk_length[k], 1), 8) * 2};
        },
        [&](int c, int) { return InRow{adpcm[c], adx::decode_bytes_read_v(sample_counts[c], params[c])}; },
        [&](int c, int) { return OutRow{pcm_out[c], (size_t)sample_counts[c] * 2}; });
    DevBuf d_in, d_pcm, d_status, d_own;
    std::vector<int> own(nch);                                                      // (as the encoder's: the plan's order)
    for (int i = 0; i < nch; i++) own[i] = sample_counts[plan.order[i]];
    VGA_HIP_TRY(d_own.alloc((size_t)nch * sizeof(int)));
    VGA_HIP_TRY(hipMemcpy(d_own.p, own.data(), (size_t)nch * sizeof(int), hipMemcpyHostToDevice));
    if (int rc = lay.alloc(d_in, d_pcm)) return rc;                                 // frames behind a row's end: scale 0, filter 0
    VGA_HIP_TRY(d_status.alloc(sizeof(int)));
    VGA_HIP_TRY(hipMemset(d_status.p, 0, sizeof(int)));
    pipe::Job job;
    job.units = nch;
    lay.bind(job, d_in, d_pcm);
    job.compute_lanes = planned_compute_lanes(1);                       // (nothing per lane)
    job.compute = chunk_compute([&](int first, int count, hipStream_t s) {
        const int k = plan.chunk_of(first);
        if (plan.chunk_length[k] <= 0) return VGA_OK;
        return adx::launch_decode(d_in.as<uint8_t>() + lay.in.base[k], lay.in.pitch[k], count, plan.chunk_length[k], dps[plan.chunk_group[k]],
                                  d_pcm.as<int16_t>() + lay.out.base[k] / 2, lay.out.pitch[k] / 2, d_status.as<int>(), s,
                                  d_own.as<int>() + first);
    });
    return adx::run_decode_job(job, d_status);
}

extern "C" {

int vga_adx_encode_batch_v(const int16_t *const *pcm, const int *pcm_lengths, int nch, const vga_adx_params *params,
                           uint8_t *const *out, int16_t *history_out)
{
    return adx::for_each_share(nch, pcm && pcm_lengths && params && out, [&](int first, int count) {
        return adx_encode_batch_v_one(pcm + first, pcm_lengths + first, count, params + first, out + first,
                                      history_out ? history_out + first : nullptr);
    });
}

int vga_adx_decode_batch_v(const uint8_t *const *adpcm, const int *adpcm_lengths, int nch, const int *sample_counts,
                           const vga_adx_params *params, int16_t *const *pcm_out)
{
    return adx::for_each_share(nch, adpcm && adpcm_lengths && sample_counts && params && pcm_out, [&](int first, int count) {
        return adx_decode_batch_v_one(adpcm + first, adpcm_lengths + first, count, sample_counts + first, params + first, pcm_out + first);
    });
}

}  // extern "C"
