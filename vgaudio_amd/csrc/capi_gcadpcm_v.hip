// capi_gcadpcm_v.hip -- GC-ADPCM over RAGGED batches: channels of different lengths in one call.
//
// The reference's batch path is a Parallel.ForEach over FILES (VGAudio.Cli/Batch.cs:24-25 -> Convert.cs:19), every file
// with its own length and channel count, each ending up in GcAdpcmFormat.EncodeFromPcm16 (Formats/GcAdpcm/GcAdpcmFormat.cs:
// 58-74) one channel at a time.  One call per file leaves the chip idle (a lone 60 s channel: 0.4 % of the batch rate);
// here the channels of many files travel in ONE call.  The kernels are the ones of the equal-length entry points with
// per-channel shapes read from device tables (gc::Ragged, gcadpcm_kernels.hpp): channels are cut into time pieces of one
// common length, work slots are handed out longest channel first.
// The rows' layout, the chunk cut and the longest-first order are gc_host.hpp's; RaggedShape and the group launches are
// gc_capi.hpp's.
#include "gc_capi.hpp"

using namespace vga;
using gc::RaggedShape;

// ---------------------------------------------------------------- device-resident ragged batches
struct vga_gcadpcm_ragged {
    RaggedShape shape;
    gc::Ragged view;
    void *d_tables = nullptr;
    int device = 0;
    int64_t pcm_samples = 0, adpcm_bytes = 0;
};

extern "C" {

int vga_gcadpcm_ragged_create(const int *sample_counts, int nch, vga_gcadpcm_ragged **out)
{
    if (!out) { set_error("null output"); return VGA_ERR_ARGUMENT; }
    *out = nullptr;
    if (int rc = gc::check_counts(sample_counts, nch, "vga_gcadpcm_ragged_create")) return rc;
    if (int rc = require_device()) return rc;
    vga_gcadpcm_ragged *r = new vga_gcadpcm_ragged;
    r->shape.build(sample_counts, nch, 0, 0);
    r->pcm_samples = r->shape.pcm_end + gc::GUARD_BYTES / 2;
    r->adpcm_bytes = r->shape.adpcm_end + gc::GUARD_BYTES;
    (void)hipGetDevice(&r->device);
    const size_t tb = r->shape.table_bytes();
    std::vector<unsigned char> host(tb ? tb : 16);
    r->shape.write_tables(host.data());
    hipError_t e = device_malloc(&r->d_tables, host.size());
    if (e == hipSuccess) e = hipMemcpy(r->d_tables, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (r->d_tables) (void)hipFree(r->d_tables);
        delete r;
        set_error("ragged tables: %s", hipGetErrorString(e));
        return VGA_ERR_DEVICE;
    }
    r->view = r->shape.device_view(static_cast<const unsigned char *>(r->d_tables));
    *out = r;
    return VGA_OK;
}

void vga_gcadpcm_ragged_destroy(vga_gcadpcm_ragged *r)
{
    if (!r) return;
    if (r->d_tables) (void)hipFree(r->d_tables);
    delete r;
}

int vga_gcadpcm_ragged_channels(const vga_gcadpcm_ragged *r) { return r ? r->shape.count : 0; }
int64_t vga_gcadpcm_ragged_pcm_samples(const vga_gcadpcm_ragged *r) { return r ? r->pcm_samples : 0; }
int64_t vga_gcadpcm_ragged_adpcm_bytes(const vga_gcadpcm_ragged *r) { return r ? r->adpcm_bytes : 0; }
size_t vga_gcadpcm_ragged_coefs_workspace_bytes(const vga_gcadpcm_ragged *r) { return r ? (size_t)std::max<int64_t>(r->shape.records, 1) * 16 : 0; }

int vga_gcadpcm_ragged_offsets(const vga_gcadpcm_ragged *r, int64_t *pcm_offsets_out, int64_t *adpcm_offsets_out)
{
    if (!r) { set_error("null ragged batch"); return VGA_ERR_ARGUMENT; }
    for (int c = 0; c < r->shape.count; c++) {
        if (pcm_offsets_out) pcm_offsets_out[c] = r->shape.pcm_off[c];
        if (adpcm_offsets_out) adpcm_offsets_out[c] = r->shape.adpcm_off[c];
    }
    return VGA_OK;
}

static int check_ragged_call(const vga_gcadpcm_ragged *r, const void *a, const void *b, const char *what)
{
    if (!r) { set_error("%s: null ragged batch", what); return VGA_ERR_ARGUMENT; }
    if (r->shape.count > 0 && (!a || !b)) { set_error("%s: null device buffer", what); return VGA_ERR_ARGUMENT; }
    if (((uintptr_t)a & 15) || ((uintptr_t)b & 15)) { set_error("%s: device buffers must be 16-byte aligned", what); return VGA_ERR_ARGUMENT; }
    int device = -1;
    (void)hipGetDevice(&device);
    if (device != r->device) { set_error("%s: the ragged batch was created on device %d, the current one is %d", what, r->device, device); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

int vga_gcadpcm_coefs_device_v(const vga_gcadpcm_ragged *r, const int16_t *d_pcm, int16_t *d_coefs, void *d_workspace,
                               size_t workspace_bytes, void *stream)
{
    if (int rc = check_ragged_call(r, d_pcm, d_coefs, "vga_gcadpcm_coefs_device_v")) return rc;
    if (r->shape.count == 0) return VGA_OK;
    if (!d_workspace || workspace_bytes < vga_gcadpcm_ragged_coefs_workspace_bytes(r)) {
        set_error("workspace too small: need %zu bytes", vga_gcadpcm_ragged_coefs_workspace_bytes(r));
        return VGA_ERR_ARGUMENT;
    }
    return gc::launch_coefs_group(r->shape, r->view, d_pcm, d_coefs, d_workspace, (hipStream_t)stream);
}

int vga_gcadpcm_encode_device_v(const vga_gcadpcm_ragged *r, const int16_t *d_pcm, const int16_t *d_coefs, const int16_t *d_hist1,
                                const int16_t *d_hist2, uint8_t *d_adpcm, void *stream)
{
    if (int rc = check_ragged_call(r, d_pcm, d_adpcm, "vga_gcadpcm_encode_device_v")) return rc;
    if (r->shape.count > 0 && !d_coefs) { set_error("null coefficients"); return VGA_ERR_ARGUMENT; }
    return gc::launch_encode_group(r->shape, r->view, d_pcm, d_coefs, d_hist1, d_hist2, d_adpcm, (hipStream_t)stream, nullptr, 0);
}

int vga_gcadpcm_decode_device_v(const vga_gcadpcm_ragged *r, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *d_hist1,
                                const int16_t *d_hist2, int16_t *d_pcm, int *d_status, void *stream)
{
    if (int rc = check_ragged_call(r, d_adpcm, d_pcm, "vga_gcadpcm_decode_device_v")) return rc;
    if (r->shape.count > 0 && !d_coefs) { set_error("null coefficients"); return VGA_ERR_ARGUMENT; }
    return gc::launch_decode_group(r->shape, r->view, d_adpcm, d_coefs, d_hist1, d_hist2, d_pcm, d_status, (hipStream_t)stream);
}

}  // extern "C"

// ---------------------------------------------------------------- host rows: the pipelined calls
namespace {

// One ragged call: the whole batch's rows packed on the device, chunks of channels by volume, every chunk with its own
// shape tables (local channel indices, offsets from the call's buffers).
struct RaggedCall {
    int nch = 0;
    RaggedRows pcm_rows, adpcm_rows;                  // per channel (caller order)
    std::vector<int> chunk_begin;
    std::vector<RaggedShape> chunks;
    std::vector<gc::Ragged> views;
    DevBuf pcm, adpcm, coefs, h1, h2, tables, status;
    int64_t max_chunk_records = 1;
    int max_chunk_channels = 1;

    int build(const int *counts, int n)
    {
        nch = n;
        chunk_begin = gc::cut_chunks(counts, n, pipe_override().chunk_units);
        chunks.resize(chunk_begin.size() - 1);
        int64_t pcm_base = 0, adpcm_base = 0;
        size_t table_total = 0;
        for (size_t k = 0; k + 1 < chunk_begin.size(); k++) {
            chunks[k].build(counts + chunk_begin[k], chunk_begin[k + 1] - chunk_begin[k], pcm_base, adpcm_base);
            pcm_base = chunks[k].pcm_end;
            adpcm_base = chunks[k].adpcm_end;
            table_total += (size_t)round_up((int64_t)chunks[k].table_bytes(), 16);
            max_chunk_records = std::max(max_chunk_records, chunks[k].records);
            max_chunk_channels = std::max(max_chunk_channels, chunks[k].count);
        }
        pcm_rows.size.resize(n); pcm_rows.off.resize(n); adpcm_rows.size.resize(n); adpcm_rows.off.resize(n);
        for (size_t k = 0; k < chunks.size(); k++)
            for (int i = 0; i < chunks[k].count; i++) {
                const int c = chunk_begin[k] + i;
                pcm_rows.size[c] = (size_t)counts[c] * 2;
                pcm_rows.off[c] = (size_t)chunks[k].pcm_off[i] * 2;
                adpcm_rows.size[c] = (size_t)gc::sample_count_to_byte_count(counts[c]);
                adpcm_rows.off[c] = (size_t)chunks[k].adpcm_off[i];
                pcm_rows.max_pitch = std::max<size_t>(pcm_rows.max_pitch, (size_t)round_up((int64_t)pcm_rows.size[c], 16));
                adpcm_rows.max_pitch = std::max<size_t>(adpcm_rows.max_pitch, (size_t)round_up((int64_t)adpcm_rows.size[c], 16));
            }
        VGA_HIP_TRY(pcm.alloc((size_t)pcm_base * 2 + gc::GUARD_BYTES));
        VGA_HIP_TRY(adpcm.alloc((size_t)adpcm_base + gc::GUARD_BYTES));
        VGA_HIP_TRY(coefs.alloc((size_t)std::max(n, 1) * 32));
        VGA_HIP_TRY(tables.alloc(table_total ? table_total : 16));
        std::vector<unsigned char> host(table_total ? table_total : 16);
        size_t at = 0;
        views.resize(chunks.size());
        for (size_t k = 0; k < chunks.size(); k++) {
            chunks[k].write_tables(host.data() + at);
            views[k] = chunks[k].device_view(tables.as<unsigned char>() + at);
            at += (size_t)round_up((int64_t)chunks[k].table_bytes(), 16);
        }
        VGA_HIP_TRY(hipMemcpy(tables.p, host.data(), host.size(), hipMemcpyHostToDevice));
        return VGA_OK;
    }
    int chunk_of(int first) const
    {
        return (int)(std::upper_bound(chunk_begin.begin(), chunk_begin.end(), first) - chunk_begin.begin()) - 1;
    }
};

int encode_batch_v_rows(const int16_t *const *pcm, const int *counts, int nch, const int16_t *hist1, const int16_t *hist2,
                        int16_t *coefs_out, uint8_t *const *adpcm_out, bool with_coefs, const int16_t *coefs_in)
{
    if (int rc = gc::check_encode_v(pcm, counts, nch, coefs_out, adpcm_out, with_coefs, coefs_in)) return rc;
    if (nch == 0) return VGA_OK;
    if (int rc = require_device()) return rc;
    RaggedCall call;
    if (int rc = call.build(counts, nch)) return rc;
    if (int rc = gc::upload_hist(call.h1, call.h2, nch, hist1, hist2, nullptr)) return rc;
    if (!with_coefs) VGA_HIP_TRY(hipMemcpy(call.coefs.p, coefs_in, (size_t)nch * 32, hipMemcpyHostToDevice));
    const bool encode = adpcm_out != nullptr;
    DevBuf scratch[pipe::kMaxComputeLanes], ws[pipe::kMaxComputeLanes];   // per lane (vga_gcadpcm_encode_batch)
    pipe::Job job;
    job.units = nch;
    job.compute_lanes = planned_compute_lanes(hardware_queues_requested() >= 6 ? 2 : 1);
    job.chunk_begin = call.chunk_begin;
    bind_in(job, (const void *const *)pcm, call.pcm_rows, call.pcm.as<char>());
    if (encode) bind_out(job, (void *const *)adpcm_out, call.adpcm_rows, call.adpcm.as<char>());
    // EncodeChannel (GcAdpcmFormat.cs:129-135) for the chunk's channels: coefficients, then encode
    job.compute = chunk_compute([&](int first, int count, hipStream_t s) {
        const int lane = pipe::compute_lane();
        const int k = call.chunk_of(first);
        const RaggedShape &sh = call.chunks[k];
        int rc = VGA_OK;
        if (sh.count != count) { set_error("internal: chunk %d has %d channels, asked for %d", k, sh.count, count); rc = VGA_ERR_DEVICE; }
        int16_t *d_coefs = call.coefs.as<int16_t>() + (int64_t)first * 16;
        if (!rc && with_coefs) rc = gc::launch_coefs_group(sh, call.views[k], call.pcm.as<int16_t>(), d_coefs, ws[lane].p, s);
        if (!rc && encode)
            rc = gc::launch_encode_group(sh, call.views[k], call.pcm.as<int16_t>(), d_coefs, call.h1.p ? call.h1.as<int16_t>() + first : nullptr,
                                         call.h2.p ? call.h2.as<int16_t>() + first : nullptr, call.adpcm.as<uint8_t>(), s, scratch[lane].p,
                                         scratch[lane].bytes);
        return rc;
    });
    for (int l = 0; l < job.compute_lanes; l++) {
        if (encode) VGA_HIP_TRY(scratch[l].alloc(gc::encode_scratch_bytes(call.max_chunk_channels)));
        if (with_coefs) VGA_HIP_TRY(ws[l].alloc((size_t)call.max_chunk_records * 16));
    }
    if (int rc = run_batch_pipeline(job, nch)) return rc;
    if (with_coefs) VGA_HIP_TRY(hipMemcpy(coefs_out, call.coefs.p, (size_t)nch * 32, hipMemcpyDeviceToHost));
    return VGA_OK;
}

int decode_batch_v_rows(const uint8_t *const *adpcm, const int16_t *coefs, const int *counts, int nch, const int16_t *hist1,
                        const int16_t *hist2, int16_t *const *pcm_out)
{
    if (int rc = gc::check_decode_v(adpcm, coefs, counts, nch, pcm_out)) return rc;
    if (nch == 0) return VGA_OK;
    if (int rc = require_device()) return rc;
    RaggedCall call;
    if (int rc = call.build(counts, nch)) return rc;
    if (int rc = gc::upload_hist(call.h1, call.h2, nch, hist1, hist2, nullptr)) return rc;
    VGA_HIP_TRY(hipMemcpy(call.coefs.p, coefs, (size_t)nch * 32, hipMemcpyHostToDevice));
    VGA_HIP_TRY(call.status.alloc(sizeof(int)));
    VGA_HIP_TRY(hipMemset(call.status.p, 0, sizeof(int)));
    pipe::Job job;
    job.units = nch;
    job.chunk_begin = call.chunk_begin;
    bind_in(job, (const void *const *)adpcm, call.adpcm_rows, call.adpcm.as<char>());
    bind_out(job, (void *const *)pcm_out, call.pcm_rows, call.pcm.as<char>());
    job.compute_lanes = planned_compute_lanes(1);                       // (nothing per lane)
    job.compute = chunk_compute([&](int first, int count, hipStream_t s) {
        const int k = call.chunk_of(first);
        const RaggedShape &sh = call.chunks[k];
        int rc = VGA_OK;
        if (sh.count != count) { set_error("internal: chunk %d has %d channels, asked for %d", k, sh.count, count); rc = VGA_ERR_DEVICE; }
        if (!rc)
            rc = gc::launch_decode_group(sh, call.views[k], call.adpcm.as<uint8_t>(), call.coefs.as<int16_t>() + (int64_t)first * 16,
                                         call.h1.p ? call.h1.as<int16_t>() + first : nullptr, call.h2.p ? call.h2.as<int16_t>() + first : nullptr,
                                         call.pcm.as<int16_t>(), call.status.as<int>(), s);
        return rc;
    });
    return run_status_job(job, nch, call.status, gc::BAD_PREDICTOR);
}

// the rows longest first (gc::LongestFirst); results go back to the caller's rows
int encode_batch_v_one(const int16_t *const *pcm, const int *counts, int nch, const int16_t *hist1, const int16_t *hist2,
                       int16_t *coefs_out, uint8_t *const *adpcm_out, bool with_coefs, const int16_t *coefs_in)
{
    if (int rc = gc::check_encode_v(pcm, counts, nch, coefs_out, adpcm_out, with_coefs, coefs_in)) return rc;
    const gc::LongestFirst lf(counts, nch);
    if (nch < 2 || lf.identity) return encode_batch_v_rows(pcm, counts, nch, hist1, hist2, coefs_out, adpcm_out, with_coefs, coefs_in);
    const std::vector<int> n2 = lf.gather(counts);
    const std::vector<const int16_t *> in2 = lf.gather(pcm);
    std::vector<uint8_t *> out2;
    if (adpcm_out) out2 = lf.gather(adpcm_out);
    std::vector<int16_t> h1, h2, cin, cout;
    if (hist1) h1 = lf.gather(hist1);
    if (hist2) h2 = lf.gather(hist2);
    if (!with_coefs) cin = lf.gather_rows(coefs_in, 16);
    if (with_coefs) cout.resize((size_t)nch * 16);
    const int rc = encode_batch_v_rows(in2.data(), n2.data(), nch, hist1 ? h1.data() : nullptr, hist2 ? h2.data() : nullptr,
                                       with_coefs ? cout.data() : nullptr, adpcm_out ? out2.data() : nullptr, with_coefs,
                                       with_coefs ? nullptr : cin.data());
    if (rc == VGA_OK && with_coefs) lf.scatter_rows(cout, 16, coefs_out);
    return rc;
}

int decode_batch_v_one(const uint8_t *const *adpcm, const int16_t *coefs, const int *counts, int nch, const int16_t *hist1,
                       const int16_t *hist2, int16_t *const *pcm_out)
{
    if (int rc = gc::check_decode_v(adpcm, coefs, counts, nch, pcm_out)) return rc;
    const gc::LongestFirst lf(counts, nch);
    if (nch < 2 || lf.identity) return decode_batch_v_rows(adpcm, coefs, counts, nch, hist1, hist2, pcm_out);
    const std::vector<int> n2 = lf.gather(counts);
    const std::vector<const uint8_t *> in2 = lf.gather(adpcm);
    const std::vector<int16_t *> out2 = lf.gather(pcm_out);
    const std::vector<int16_t> c2 = lf.gather_rows(coefs, 16);
    std::vector<int16_t> h1, h2;
    if (hist1) h1 = lf.gather(hist1);
    if (hist2) h2 = lf.gather(hist2);
    return decode_batch_v_rows(in2.data(), c2.data(), n2.data(), nch, hist1 ? h1.data() : nullptr, hist2 ? h2.data() : nullptr, out2.data());
}

}  // namespace

extern "C" {

int vga_gcadpcm_encode_batch_v(const int16_t *const *pcm, const int *sample_counts, int nch, const int16_t *hist1, const int16_t *hist2,
                               int16_t *coefs_out, uint8_t *const *adpcm_out)
{
    if (nch > 0 && !adpcm_out) { set_error("null adpcm_out"); return VGA_ERR_ARGUMENT; }
    if (nch <= 0 || !pcm || !sample_counts || !coefs_out)
        return encode_batch_v_one(pcm, sample_counts, nch, hist1, hist2, coefs_out, adpcm_out, true, nullptr);
    return for_each_device_share(nch, gc::GC_MIN_SHARE_CHANNELS, [&](int first, int count) {
        return encode_batch_v_one(pcm + first, sample_counts + first, count, hist1 ? hist1 + first : nullptr, hist2 ? hist2 + first : nullptr,
                                  coefs_out + (size_t)first * 16, adpcm_out + first, true, nullptr);
    });
}

int vga_gcadpcm_calculate_coefficients_batch_v(const int16_t *const *pcm, const int *lengths, int nch, int16_t *coefs_out)
{
    if (nch <= 0 || !pcm || !lengths || !coefs_out) return encode_batch_v_one(pcm, lengths, nch, nullptr, nullptr, coefs_out, nullptr, true, nullptr);
    return for_each_device_share(nch, gc::GC_MIN_SHARE_CHANNELS, [&](int first, int count) {
        return encode_batch_v_one(pcm + first, lengths + first, count, nullptr, nullptr, coefs_out + (size_t)first * 16, nullptr, true, nullptr);
    });
}

int vga_gcadpcm_encode_with_coefs_batch_v(const int16_t *const *pcm, const int *sample_counts, int nch, const int16_t *coefs,
                                          const int16_t *hist1, const int16_t *hist2, uint8_t *const *adpcm_out)
{
    if (nch > 0 && !adpcm_out) { set_error("null adpcm_out"); return VGA_ERR_ARGUMENT; }
    if (nch <= 0 || !pcm || !sample_counts || !coefs)
        return encode_batch_v_one(pcm, sample_counts, nch, hist1, hist2, nullptr, adpcm_out, false, coefs);
    return for_each_device_share(nch, gc::GC_MIN_SHARE_CHANNELS, [&](int first, int count) {
        return encode_batch_v_one(pcm + first, sample_counts + first, count, hist1 ? hist1 + first : nullptr, hist2 ? hist2 + first : nullptr,
                                  nullptr, adpcm_out + first, false, coefs + (size_t)first * 16);
    });
}

int vga_gcadpcm_decode_batch_v(const uint8_t *const *adpcm, const int16_t *coefs, const int *sample_counts, int nch, const int16_t *hist1,
                               const int16_t *hist2, int16_t *const *pcm_out)
{
    if (nch <= 0 || !adpcm || !coefs || !sample_counts || !pcm_out) return decode_batch_v_one(adpcm, coefs, sample_counts, nch, hist1, hist2, pcm_out);
    return for_each_device_share(nch, gc::GC_MIN_SHARE_CHANNELS, [&](int first, int count) {
        return decode_batch_v_one(adpcm + first, coefs + (size_t)first * 16, sample_counts + first, count, hist1 ? hist1 + first : nullptr,
                                  hist2 ? hist2 + first : nullptr, pcm_out + first);
    });
}

}  // extern "C"
