// capi_hca_v.hip -- CRI HCA over RAGGED host batches: every stream with its own shape in one call (vga_hca_encode_batch_v,
// vga_hca_decode_batch_v, include/vgaudio_hip.h).
#include "hca_capi.hpp"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

using namespace vga;
using namespace vga::hca;

// ---------------------------------------------------------------- ragged batches (VGAudio.Cli/Batch.cs:24-25: a worker per FILE)
// Every stream with its own CriHcaParameters (channel count, sample rate, length, quality, loop).  Streams that are not
// looping and differ in length only share their launches: sorted into buckets of similar length (host_batch.hpp,
// plan_buckets), zero-padded on the device to the bucket's longest and encoded with THAT stream's HcaInfo -- frame size
// and band counts come from the bitrate (CriHcaEncoder.cs:288-368), not from the length, every frame is encoded
// independently of the others (hca_encode_kernel.hip) and the encoder's own input past the end of the PCM is silence
// (:234-240), so a shorter stream's frames are the first frames of the padded one.  Looping streams (their loop audio is
// replayed behind the main audio, :209-232) share launches too, whatever their loops: a chunk of them is ONE launch of the
// PACKED encoder over the chunk's pitched rows, every stream with its own HcaInfo and its own stream map (hca_kernels.hpp:
// PackedRun, PackedLoopMap), the rows as long as the caller's files -- so a loop shorter than the post audio replays what the
// file holds behind its loop end, as the reference does (include/vgaudio_hip_files/hca_ragged_loops.h).
namespace {

struct HcaGroupKey {
    int quality, bitrate, limit_bitrate, channel_count, sample_rate, looping, shape_class;
};

struct HcaEncodeVStats { long long v[4] = {0, 0, 0, 0}; };          // vga_testing_hca_encode_v_stats
HcaEncodeVStats &hca_encode_v_last()
{
    static thread_local HcaEncodeVStats last;
    return last;
}

// shape_class: of a looping stream, among the job's streams (streams of one key have one class: the frame size and the bands
// follow from the key's fields; the launch is compiled data for the class, so the key says so); -1 for a plain one
int hca_group_of(std::vector<HcaGroupKey> &seen, const vga_hca_params &c, int shape_class)
{
    HcaGroupKey k = {c.quality, c.bitrate, c.limit_bitrate, c.channel_count, c.sample_rate, c.looping ? 1 : 0, c.looping ? shape_class : -1};
    for (size_t i = 0; i < seen.size(); i++)
        if (memcmp(&seen[i], &k, sizeof k) == 0) return (int)i;
    seen.push_back(k);
    return (int)seen.size() - 1;
}

// the streams of `units` (indices into the caller's arrays) that have `nch` channels: one pipelined job
int hca_encode_v_job(const std::vector<int> &units, int nch, const int16_t *const *pcm, const std::vector<size_t> &first_row,
                     const vga_hca_params *configs, const vga_hca_info *infos, uint8_t *const *frames_out)
{
    const int n = (int)units.size();
    std::vector<hca::DeviceInfo> dev(n);
    for (int i = 0; i < n; i++)
        if (int rc = make_device_info(infos[units[i]], dev[i])) return rc;
    std::vector<int> cls;
    decode_classes(dev.data(), n, cls);
    std::vector<HcaGroupKey> keys;
    std::vector<int> group(n), length(n);
    for (int i = 0; i < n; i++) {
        group[i] = hca_group_of(keys, configs[units[i]], cls[i]);
        length[i] = configs[units[i]].sample_count;
    }
    const BucketPlan plan = plan_buckets(group, length, HCA_CHUNK_STREAMS, HCA_BUCKET_VOLUME, true);
    const int chunks = (int)plan.chunk_begin.size() - 1;
    std::vector<vga_hca_info> chunk_info(chunks);
    std::vector<int64_t> chunk_frames_pitch(chunks);
    for (int k = 0; k < chunks; k++) {
        chunk_info[k] = infos[units[plan.order[plan.chunk_begin[k + 1] - 1]]];   // the bucket's longest stream
        chunk_frames_pitch[k] = frames_pitch_for(chunk_info[k]);
        // looping streams: the longest file need not have the most frames (its loop may end early)
        for (int i = plan.chunk_begin[k]; chunk_info[k].looping && i < plan.chunk_begin[k + 1]; i++)
            chunk_frames_pitch[k] = std::max(chunk_frames_pitch[k], frames_pitch_for(infos[units[plan.order[i]]]));
    }
    HcaEncodeVStats &stats = hca_encode_v_last();
    stats.v[0] += n;
    stats.v[1] += (long long)keys.size();
    stats.v[2] += chunks;
    // a unit is a stream: nch rows of PCM in, one row of frames out
    const BucketLayout lay = layout_buckets(
        plan, nch, 1,
        [&](int k) {
            return RowPitch{round_up(std::max(plan.chunk_length[k], 1), 8) * 2,
                            chunk_frames_pitch[k]};
        },
        [&](int i, int c) { return InRow{pcm[first_row[units[i]] + c], (size_t)configs[units[i]].sample_count * 2}; },
        [&](int i, int) { return OutRow{frames_out[units[i]], (size_t)infos[units[i]].frame_count * infos[units[i]].frame_size}; });
    DevBuf d_pcm, d_frames, d_status;
    if (int rc = lay.alloc(d_pcm, d_frames)) return rc;                             // silence behind every row
    if (int rc = alloc_status_word(d_status)) return rc;
    // the looping chunks' tables: the runs of every stream in the plan's order (run_at: position -> its first run), each with
    // the rows and frames of its place in the bucket layout, and the looping streams' maps; one upload for the whole job
    std::vector<hca::PackedRun> runs;
    std::vector<hca::PackedLoopMap> loops;
    std::vector<int> run_at(n + 1, 0);
    std::vector<char> chunk_wave(chunks, 0);
    const uint16_t *crc_pow = nullptr;
    for (int k = 0; k < chunks; k++) {
        const int begin = plan.chunk_begin[k], end = plan.chunk_begin[k + 1];
        if (chunk_info[k].looping) {
            if (int rc = crc_pow_table(&crc_pow)) return rc;
            int64_t total = 0;
            for (int i = begin; i < end; i++) total += infos[units[plan.order[i]]].frame_count;
            bool wave = false;
            const int per_run = hca::encode_frames_per_run(dev[plan.order[begin]], total, hca_frames_per_group_override(), &wave);
            chunk_wave[k] = wave;
            for (int i = begin; i < end; i++) {
                const vga_hca_info &h = infos[units[plan.order[i]]];
                run_at[i] = (int)runs.size();
                if (bitrate_too_low(h)) { set_error("Bitrate is set too low."); return VGA_ERR_INVALID_DATA; }
                hca::PackedRun r = {};
                r.frames_at = lay.out.base[k] + (int64_t)(i - begin) * lay.out.pitch[k];
                r.pcm_at = (lay.in.base[k] + (int64_t)(i - begin) * nch * lay.in.pitch[k]) / 2;
                r.frames_room = lay.out.base.back() + 64 - r.frames_at;
                r.ch_pitch = (int)(lay.in.pitch[k] / 2);
                r.frame_count = h.frame_count;
                r.sample_count = h.sample_count;
                r.inserted_samples = h.inserted_samples;
                if (int rc = set_encoder_map(r, h, configs[units[plan.order[i]]].sample_count, &loops)) return rc;
                for (int f = 0; f < h.frame_count; f += per_run) {
                    r.f0 = f;
                    r.len = std::min(per_run, h.frame_count - f);
                    runs.push_back(r);
                }
            }
        } else
            for (int i = begin; i < end; i++) run_at[i] = (int)runs.size();
        run_at[end] = (int)runs.size();
    }
    DevBuf d_runs, d_loops;
    if (!runs.empty()) {
        VGA_HIP_TRY(d_runs.alloc(runs.size() * sizeof(hca::PackedRun)));
        VGA_HIP_TRY(hipMemcpy(d_runs.p, runs.data(), runs.size() * sizeof(hca::PackedRun), hipMemcpyHostToDevice));
        VGA_HIP_TRY(d_loops.alloc(loops.size() * sizeof(hca::PackedLoopMap)));
        VGA_HIP_TRY(hipMemcpy(d_loops.p, loops.data(), loops.size() * sizeof(hca::PackedLoopMap), hipMemcpyHostToDevice));
    }
    for (int k = 0; k < chunks; k++) stats.v[3] += chunk_info[k].frame_count > 0 ? 1 : 0;
    pipe::Job job;
    job.units = n;
    lay.bind(job, d_pcm, d_frames);
    job.compute_lanes = planned_compute_lanes(1);                       // (nothing per lane)
    job.compute = chunk_compute([&](int first, int count, hipStream_t s) {
        const int k = plan.chunk_of(first);
        if (chunk_info[k].frame_count <= 0) return VGA_OK;
        if (chunk_info[k].looping)
            return hca::launch_encode_packed(d_pcm.as<int16_t>(), shape_class_of(dev[plan.order[first]]), d_runs.as<hca::PackedRun>() + run_at[first],
                                             run_at[first + count] - run_at[first], chunk_wave[k] != 0, d_frames.as<uint8_t>(),
                                             crc_pow, d_status.as<int>(), s, d_loops.as<hca::PackedLoopMap>());
        const int64_t ch_pitch = lay.in.pitch[k] / 2;
        return vga_hca_encode_device(d_pcm.as<int16_t>() + lay.in.base[k] / 2, ch_pitch * nch, ch_pitch, count, plan.chunk_length[k],
                                     &chunk_info[k], d_frames.as<uint8_t>() + lay.out.base[k], lay.out.pitch[k], d_status.as<int>(), s);
    });
    return run_status_job(job, HCA_CHUNK_STREAMS, d_status);
}

// ---- ragged decode.  Nothing in the decoder but three numbers depends on a stream's length: frame size, band layout,
// channel types and the ATH curve follow from the bitrate, the quality and the rate (above), and the kernels take
// {frame_count, sample_count, inserted_samples} per stream from a table (hca_decode_kernels.hip, RAGGED).  So streams are
// sorted into SHAPE CLASSES -- equality of what make_device_info() builds with those three fields ignored; the loop fields,
// comment_length and header_size of the HcaInfo are not in it, the decoder reads none of them -- and inside a class into
// buckets of similar length that share one launch set, exactly as the encoder's (plan_buckets).  No stream is padded with
// work: the rows behind a short stream are zeros nobody decodes.
struct HcaDecodeVStats { long long v[5] = {0, 0, 0, 0, 0}; };       // vga_testing_hca_decode_v_stats
HcaDecodeVStats &hca_decode_v_last()
{
    static thread_local HcaDecodeVStats last;
    return last;
}

struct HcaDecodeVCall {
    const vga_hca_info *infos = nullptr;
    const uint8_t *const *frames = nullptr;
    int16_t *const *pcm_out = nullptr;
    std::vector<size_t> first_row;                                      // stream -> its first row of pcm_out
    std::vector<hca::DeviceInfo> dev;
    std::vector<int> cls;
};

// the streams of `units` (indices into the caller's arrays), all of `nch` channels: one pipelined job
int hca_decode_v_job(const HcaDecodeVCall &call, const std::vector<int> &units, int nch, HcaDecodeVStats &stats)
{
    if (int rc = require_device()) return rc;                           // (a device share's own thread)
    const int n = (int)units.size();
    const vga_hca_info *infos = call.infos;
    auto frame_bytes = [&](int u) { return (int64_t)infos[u].frame_count * infos[u].frame_size; };
    // length[i]: the stream's BYTES of frames (not its frame count): inside a class the frame size is one, so the order is
    // the same, and plan_buckets' additive slack of 1024 units is then a frame or three, not a thousand frames
    std::vector<int> group(n), length(n);
    for (int i = 0; i < n; i++) {
        group[i] = call.cls[units[i]];
        length[i] = (int)std::min<int64_t>(frame_bytes(units[i]), INT32_MAX);
    }
    const BucketPlan plan = plan_buckets(group, length, HCA_DECODE_CHUNK_STREAMS, HCA_DECODE_BUCKET_VOLUME, true);
    const int chunks = (int)plan.chunk_begin.size() - 1;
    // a chunk's launches carry its longest frame count; the table carries every stream's own (in the plan's order)
    std::vector<hca::DeviceInfo> chunk_dev(chunks);
    std::vector<int> chunk_samples(chunks, 0);
    std::vector<int4> dims(n);
    std::vector<size_t> ws_at(chunks + 1, 0);
    for (int k = 0; k < chunks; k++) {
        hca::DeviceInfo &d = chunk_dev[k];
        d = shape_class_of(call.dev[units[plan.order[plan.chunk_begin[k]]]]);
        for (int i = plan.chunk_begin[k]; i < plan.chunk_begin[k + 1]; i++) {
            const vga_hca_info &h = infos[units[plan.order[i]]];
            dims[i] = make_int4(h.frame_count, h.sample_count, h.inserted_samples, 0);
            d.frame_count = std::max(d.frame_count, h.frame_count);
            chunk_samples[k] = std::max(chunk_samples[k], h.sample_count);
            stats.v[3] += h.frame_count;
        }
        d.sample_count = chunk_samples[k];
        const int count = plan.chunk_begin[k + 1] - plan.chunk_begin[k];
        stats.v[4] += (long long)count * d.frame_count;
        ws_at[k + 1] = ws_at[k] + hca::decode_record_bytes(d) * (size_t)count * (size_t)d.frame_count;   // count x longest, as ever
    }
    stats.v[0] += 1;
    stats.v[1] += chunks;
    // a unit is a stream: one row of frames in (8 bytes of slack behind the longest), nch rows of PCM out
    const BucketLayout lay = layout_buckets(
        plan, 1, nch,
        [&](int k) {
            return RowPitch{round_up((int64_t)chunk_dev[k].frame_count * chunk_dev[k].frame_size + 8, 16),
                            round_up(std::max(chunk_samples[k], 1), 8) * 2};
        },
        [&](int i, int) { return InRow{call.frames[units[i]], (size_t)frame_bytes(units[i])}; },
        [&](int i, int c) { return OutRow{call.pcm_out[call.first_row[units[i]] + c], (size_t)infos[units[i]].sample_count * 2}; });
    DevBuf d_frames, d_pcm, d_status, d_ws, d_dims;
    if (int rc = lay.alloc(d_frames, d_pcm)) return rc;                  // zeros behind every stream's frames: the slack, the padding
    // samples no frame covers (a header that declares more samples than its frames hold) are zeros, as in vga_hca_decode_batch
    VGA_HIP_TRY(hipMemset(d_pcm.p, 0, (size_t)lay.out.base.back() + 64));
    if (int rc = alloc_status_word(d_status)) return rc;
    VGA_HIP_TRY(d_ws.alloc(ws_at[chunks]));
    VGA_HIP_TRY(d_dims.alloc(dims.size() * sizeof(int4)));               // the whole call's table, one copy
    VGA_HIP_TRY(hipMemcpy(d_dims.p, dims.data(), dims.size() * sizeof(int4), hipMemcpyHostToDevice));
    pipe::Job job;
    job.units = n;
    lay.bind(job, d_frames, d_pcm);
    job.compute_lanes = planned_compute_lanes(1);                       // (nothing per lane)
    job.compute = chunk_compute([&](int first, int count, hipStream_t s) {
        const int k = plan.chunk_of(first);
        const int64_t ch_pitch = lay.out.pitch[k] / 2;
        return hca::launch_decode(d_frames.as<uint8_t>() + lay.in.base[k], lay.in.pitch[k], count, chunk_dev[k],
                                  d_pcm.as<int16_t>() + lay.out.base[k] / 2, ch_pitch * nch, ch_pitch, d_ws.as<char>() + ws_at[k],
                                  d_status.as<int>(), s, d_dims.as<int4>() + first);
    });
    return run_status_job(job, HCA_DECODE_CHUNK_STREAMS, d_status);
}

}  // namespace

extern "C" {

int vga_hca_encode_batch_v(const int16_t *const *pcm, int nstreams, const vga_hca_params *configs, vga_hca_info *infos_out,
                           uint8_t *const *frames_out)
{
    hca_encode_v_last() = HcaEncodeVStats();
    if (nstreams < 0) { set_error("negative stream count"); return VGA_ERR_ARGUMENT; }
    if (nstreams == 0) return VGA_OK;
    if (!pcm || !configs || !infos_out || !frames_out) { set_error("null array"); return VGA_ERR_ARGUMENT; }
    std::vector<size_t> first_row(nstreams);
    size_t rows = 0;
    for (int s = 0; s < nstreams; s++) {
        if (int rc = vga_hca_encoder_initialize(&configs[s], &infos_out[s])) return rc;
        first_row[s] = rows;
        rows += (size_t)configs[s].channel_count;
        if (!frames_out[s] && infos_out[s].frame_count > 0) { set_error("frames_out[%d] is null", s); return VGA_ERR_ARGUMENT; }
        for (int c = 0; c < configs[s].channel_count; c++)
            if (!pcm[first_row[s] + c] && configs[s].sample_count > 0) { set_error("stream %d channel %d is null", s, c); return VGA_ERR_ARGUMENT; }
    }
    if (int rc = require_device()) return rc;
    return for_each_channel_count(0, nstreams, [&](int s) { return configs[s].channel_count; }, [&](const std::vector<int> &units, int nch) {
        return hca_encode_v_job(units, nch, pcm, first_row, configs, infos_out, frames_out);
    });
}

int vga_hca_decode_batch_v(const vga_hca_info *infos, const uint8_t *const *frames, int nstreams, int16_t *const *pcm_out)
{
    HcaDecodeVStats &last = hca_decode_v_last();
    last = HcaDecodeVStats();
    if (nstreams < 0) { set_error("negative stream count"); return VGA_ERR_ARGUMENT; }
    if (nstreams == 0) return VGA_OK;
    if (!infos || !frames || !pcm_out) { set_error("null array"); return VGA_ERR_ARGUMENT; }
    HcaDecodeVCall call;
    call.infos = infos;
    call.frames = frames;
    call.pcm_out = pcm_out;
    call.first_row.resize(nstreams);
    call.dev.resize(nstreams);
    size_t rows = 0;
    for (int s = 0; s < nstreams; s++) {
        if (infos[s].channel_count < 1 || infos[s].channel_count > 8) { set_error("stream %d: bad channel count", s); return VGA_ERR_ARGUMENT; }
        call.first_row[s] = rows;
        rows += (size_t)infos[s].channel_count;
    }
    // every stream's own checks, as one vga_hca_decode_batch call for it would make them
    for (int s = 0; s < nstreams; s++) {
        const vga_hca_info &h = infos[s];
        if (int rc = make_device_info(h, call.dev[s])) return rc;
        if (h.sample_count < 0) { set_error("negative size"); return VGA_ERR_ARGUMENT; }
        if (!frames[s] && h.frame_count > 0) { set_error("frames[%d] is null", s); return VGA_ERR_ARGUMENT; }
        for (int c = 0; c < h.channel_count; c++)
            if (!pcm_out[call.first_row[s] + c] && h.sample_count > 0) { set_error("pcm_out[%d] is null", (int)call.first_row[s] + c); return VGA_ERR_ARGUMENT; }
    }
    last.v[2] = decode_classes(call.dev.data(), nstreams, call.cls);
    if (int rc = require_device()) return rc;
    HcaDecodeVStats sum;                                                // the shares run on threads of their own
    std::mutex sum_mu;
    const int rc = for_each_device_share(nstreams, HCA_MIN_SHARE_STREAMS, [&](int first, int count) {
        HcaDecodeVStats mine;
        const int rc = for_each_channel_count(first, count, [&](int s) { return infos[s].channel_count; }, [&](const std::vector<int> &units, int nch) {
            return hca_decode_v_job(call, units, nch, mine);
        });
        std::lock_guard<std::mutex> g(sum_mu);
        for (int i = 0; i < 5; i++) sum.v[i] += mine.v[i];
        return rc;
    });
    sum.v[2] = last.v[2];
    last = sum;
    return rc;
}

int vga_testing_hca_decode_classes(const void *infos, int nstreams, int *class_out)
{
    if (nstreams < 0 || (nstreams > 0 && (!infos || !class_out))) { set_error("bad arguments"); return VGA_ERR_ARGUMENT; }
    const vga_hca_info *h = static_cast<const vga_hca_info *>(infos);
    std::vector<hca::DeviceInfo> dev(nstreams);
    for (int s = 0; s < nstreams; s++)
        if (int rc = make_device_info(h[s], dev[s])) return rc;
    std::vector<int> cls;
    const int classes = decode_classes(dev.data(), nstreams, cls);
    for (int s = 0; s < nstreams; s++) class_out[s] = cls[s];
    return classes;
}

int vga_testing_hca_encode_v_stats(long long *out, int n)
{
    const HcaEncodeVStats &last = hca_encode_v_last();
    for (int i = 0; out && i < n && i < 4; i++) out[i] = last.v[i];
    return 4;
}

int vga_testing_hca_decode_v_stats(long long *out, int n)
{
    const HcaDecodeVStats &last = hca_decode_v_last();
    for (int i = 0; out && i < n && i < 5; i++) out[i] = last.v[i];
    return 5;
}

}  // extern "C"
