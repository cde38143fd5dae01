// capi_hca_ragged.hip -- device-resident CRI HCA batches of streams of different lengths (include/vgaudio_hip/hca_ragged.h).
// Host side only: the packed layout, the shape-class check and the tables the PACKED instantiations of the kernels read
// (hca_kernels.hpp: PackedRun, PackedScanStream), made once at create; a call checks its pointers and launches.
#include "hca_capi.hpp"
#include "../../include/vgaudio_hip_files/hca_ragged_loops.h"

#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

using namespace vga;

using hca::RaggedLayout;

int vga::hca::make_layout(const vga_hca_info *infos, int nstreams, RaggedLayout &L)
{
    if (nstreams < 0) { set_error("negative stream count"); return VGA_ERR_ARGUMENT; }
    if (nstreams > 0 && !infos) { set_error("null HcaInfo array"); return VGA_ERR_ARGUMENT; }
    L.infos.assign(infos, infos + nstreams);
    std::vector<hca::DeviceInfo> dev(nstreams);
    for (int s = 0; s < nstreams; s++) {   // every stream's own checks, as vga_hca_decode_device makes them
        if (int rc = make_device_info(infos[s], dev[s])) return rc;
        if (infos[s].sample_count < 0) { set_error("stream %d: negative sample count", s); return VGA_ERR_ARGUMENT; }
        if (infos[s].looping && L.first_looping < 0) L.first_looping = s;
    }
    std::vector<int> cls;
    if (decode_classes(dev.data(), nstreams, cls) > 1) {
        int bad = 0;
        while (cls[bad] == 0) bad++;
        set_error("stream %d is of another shape class than stream 0 (channels, frame size, bands or ATH curve differ): "
                  "one vga_hca_ragged object per class", bad);
        return VGA_ERR_ARGUMENT;
    }
    memset(&L.cls, 0, sizeof L.cls);
    if (nstreams > 0) L.cls = shape_class_of(dev[0]);
    L.frame_at.resize(nstreams);
    L.first_row.resize(nstreams);
    L.first_record.resize(nstreams);
    int64_t fcur = 0, pcur = 0, frames = 0;
    for (int s = 0; s < nstreams; s++) {
        const vga_hca_info &h = infos[s];
        L.frame_at[s] = fcur;
        fcur += round_up((int64_t)h.frame_count * h.frame_size, 4);
        L.first_row[s] = L.row_at.size();
        L.first_record[s] = (int)frames;
        frames += h.frame_count;
        if (frames > INT32_MAX) { set_error("more than 2^31 - 1 frames in one batch"); return VGA_ERR_ARGUMENT; }
        for (int c = 0; c < h.channel_count; c++) {
            L.row_at.push_back(pcur);
            pcur += round_up(h.sample_count, 8);
        }
    }
    L.totals.frame_bytes = fcur + 8;
    L.totals.pcm_samples = pcur;
    L.totals.rows = (int)L.row_at.size();
    L.totals.total_frames = (int)frames;
    L.totals.decode_workspace_bytes = nstreams > 0 ? hca::decode_record_bytes(L.cls) * (size_t)frames : 0;
    return VGA_OK;
}

namespace {

struct RunTable {
    hca::PackedRun *d = nullptr;
    int count = 0;
    hca::PackedLoopMap *d_loops = nullptr;   // the encoder's, where a stream loops (vga_hca_encode_loops_device_v)
};

}  // namespace

struct vga_hca_ragged {
    RaggedLayout L;
    int device = 0;
    void *d_scan = nullptr;
    int dec_per_group = 1, enc_per_run = 1;
    bool enc_wave = false;
    RunTable dec_runs, enc_runs;           // at the launchers' own frames per run
    // tables cut at a run length the test hook forces (vga_testing_hca_frames_per_group_this_thread), made on first use
    mutable std::mutex mu;
    // and the encoder's tables of an object that holds a looping stream (hook value 0 included), made on first use too
    mutable std::map<int, RunTable> hooked;   // key: hook value, + (1 << 20) for the encoder's, + (1 << 21) with loop maps
    ~vga_hca_ragged()
    {
        if (d_scan) (void)hipFree(d_scan);
        if (dec_runs.d) (void)hipFree(dec_runs.d);
        if (enc_runs.d) (void)hipFree(enc_runs.d);
        for (auto &kv : hooked) {
            if (kv.second.d) (void)hipFree(kv.second.d);
            if (kv.second.d_loops) (void)hipFree(kv.second.d_loops);
        }
    }
};

std::vector<hca::PackedRun> vga::hca::cut_runs(const RaggedLayout &L, int per_run, bool encoder, std::vector<hca::PackedLoopMap> *loops)
{
    std::vector<hca::PackedRun> runs;
    for (int s = 0; s < (int)L.infos.size(); s++) {
        const vga_hca_info &h = L.infos[s];
        if (h.frame_count <= 0 || (!encoder && h.sample_count <= 0)) continue;
        hca::PackedRun r = {};
        r.frames_at = L.frame_at[s];
        r.pcm_at = L.row_at[L.first_row[s]];
        r.frames_room = L.totals.frame_bytes - L.frame_at[s];
        r.ch_pitch = (int)round_up(h.sample_count, 8);
        r.first_record = L.first_record[s];
        r.frame_count = h.frame_count;
        r.sample_count = h.sample_count;
        r.inserted_samples = h.inserted_samples;
        if (encoder) (void)hca::set_encoder_map(r, h, h.sample_count, loops);    // (encoder_checks refuses what this refuses)
        r.stream = s;
        for (int f = 0; f < h.frame_count; f += per_run) {
            r.f0 = f;
            r.len = std::min(per_run, h.frame_count - f);
            runs.push_back(r);
        }
    }
    return runs;
}

namespace {

using hca::cut_runs;

int upload_runs(const std::vector<hca::PackedRun> &runs, RunTable &t, const std::vector<hca::PackedLoopMap> &loops = {})
{
    t.count = (int)runs.size();
    if (runs.empty()) return VGA_OK;
    VGA_HIP_TRY(device_malloc(reinterpret_cast<void **>(&t.d), runs.size() * sizeof(hca::PackedRun)));
    VGA_HIP_TRY(hipMemcpy(t.d, runs.data(), runs.size() * sizeof(hca::PackedRun), hipMemcpyHostToDevice));
    if (loops.empty()) return VGA_OK;
    VGA_HIP_TRY(device_malloc(reinterpret_cast<void **>(&t.d_loops), loops.size() * sizeof(hca::PackedLoopMap)));
    VGA_HIP_TRY(hipMemcpy(t.d_loops, loops.data(), loops.size() * sizeof(hca::PackedLoopMap), hipMemcpyHostToDevice));
    return VGA_OK;
}

// what the encoder refuses, as one vga_hca_encode_device call per stream would; vga_hca_encode_device_v refuses loops too
int encoder_checks(const RaggedLayout &L, bool loops_allowed)
{
    if (L.first_looping >= 0 && !loops_allowed) {
        set_error("stream %d loops: vga_hca_encode_device_v encodes streams that do not loop (one vga_hca_encode_device call for a looping one)",
                  L.first_looping);
        return VGA_ERR_INVALID_OP;
    }
    for (int s = 0; s < (int)L.infos.size(); s++) {
        const vga_hca_info &h = L.infos[s];
        if (hca::bitrate_too_low(h)) { set_error("Bitrate is set too low."); return VGA_ERR_INVALID_DATA; }
        hca::PcmMap m;
        if (int rc = hca::make_pcm_map(h, h.sample_count, m)) return rc;
    }
    return VGA_OK;
}

int upload_tables(vga_hca_ragged &r)
{
    const RaggedLayout &L = r.L;
    const int total = L.totals.total_frames;
    if (total <= 0) return VGA_OK;
    // the scan: the streams that have frames, and for every wave the one that holds its first frame
    std::vector<hca::PackedScanStream> streams;
    for (int s = 0; s < (int)L.infos.size(); s++) {
        if (L.infos[s].frame_count <= 0) continue;
        hca::PackedScanStream e = {};
        e.frames_at = L.frame_at[s];
        e.frames_room = L.totals.frame_bytes - L.frame_at[s];
        e.first_record = L.first_record[s];
        e.frame_count = L.infos[s].frame_count;
        e.stream = s;
        streams.push_back(e);
    }
    const int waves = (total + 63) / 64;
    std::vector<unsigned char> host(hca::packed_scan_table_bytes((int)streams.size(), total));
    const int head[4] = {(int)streams.size(), total, 0, 0};
    memcpy(host.data(), head, sizeof head);
    memcpy(host.data() + 16, streams.data(), streams.size() * sizeof(hca::PackedScanStream));
    int *first_stream = reinterpret_cast<int *>(host.data() + 16 + streams.size() * sizeof(hca::PackedScanStream));
    for (int w = 0, k = 0; w < waves; w++) {
        while (64 * w >= streams[k].first_record + streams[k].frame_count) k++;
        first_stream[w] = k;
    }
    VGA_HIP_TRY(device_malloc(&r.d_scan, host.size()));
    VGA_HIP_TRY(hipMemcpy(r.d_scan, host.data(), host.size(), hipMemcpyHostToDevice));
    r.dec_per_group = hca::decode_frames_per_group(total, 0);
    if (int rc = upload_runs(cut_runs(L, r.dec_per_group, false), r.dec_runs)) return rc;
    if (L.first_looping < 0) {
        const uint16_t *pow = nullptr;      // the encoder's CRC table: made here, so that no call has to
        if (int rc = hca::crc_pow_table(&pow)) return rc;
        r.enc_per_run = hca::encode_frames_per_run(L.cls, total, 0, &r.enc_wave);
        if (int rc = upload_runs(cut_runs(L, r.enc_per_run, true), r.enc_runs)) return rc;
    }
    return VGA_OK;
}

int check_object(const vga_hca_ragged *r, const char *what)
{
    if (!r) { set_error("%s: null vga_hca_ragged", what); return VGA_ERR_ARGUMENT; }
    int device = -1;
    (void)hipGetDevice(&device);
    if (device != r->device) { set_error("%s: the ragged batch was created on device %d, the current one is %d", what, r->device, device); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

// the runs of this call: the object's own, or (test hook) a table cut at the forced length, made once per length
int runs_for_call(const vga_hca_ragged *r, bool encoder, int hook, RunTable &out, bool *wave)
{
    const bool with_loops = encoder && r->L.first_looping >= 0;
    if (hook == 0 && !with_loops) {
        out = encoder ? r->enc_runs : r->dec_runs;
        *wave = r->enc_wave;
        return VGA_OK;
    }
    const int total = r->L.totals.total_frames;
    const int per_run = encoder ? hca::encode_frames_per_run(r->L.cls, total, hook, wave)
                                : hca::decode_frames_per_group(total, hook >= 1000 ? hook - 1000 : hook);
    std::lock_guard<std::mutex> g(r->mu);
    RunTable &t = r->hooked[hook + (encoder ? 1 << 20 : 0) + (with_loops ? 1 << 21 : 0)];
    if (!t.d && total > 0) {
        std::vector<hca::PackedLoopMap> loops;
        const std::vector<hca::PackedRun> runs = cut_runs(r->L, per_run, encoder, with_loops ? &loops : nullptr);
        if (int rc = upload_runs(runs, t, loops)) {             // never keep half a table: runs that name maps need the maps
            if (t.d) (void)hipFree(t.d);
            if (t.d_loops) (void)hipFree(t.d_loops);
            t = RunTable();
            return rc;
        }
    }
    out = t;
    return VGA_OK;
}

// both packed encode calls: the checks of one vga_hca_encode_device call per stream, the layout's, the launch
int encode_call(const vga_hca_ragged *r, const int16_t *d_pcm, uint8_t *d_frames, int *d_status, void *stream, bool loops_allowed,
                const char *what)
{
    if (int rc = encoder_checks(r->L, loops_allowed)) return rc;
    const vga_hca_ragged_totals &t = r->L.totals;
    if (t.total_frames <= 0) return VGA_OK;
    if (!d_frames || !d_status || (!d_pcm && t.pcm_samples > 0)) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (((uintptr_t)d_frames & 3) || ((uintptr_t)d_pcm & 15)) {
        set_error("bad alignment for %s (frames need 4-byte alignment, PCM 16)", what);
        return VGA_ERR_ARGUMENT;
    }
    const uint16_t *pow = nullptr;
    if (int rc = hca::crc_pow_table(&pow)) return rc;
    RunTable runs;
    bool wave = false;
    if (int rc = runs_for_call(r, true, hca_frames_per_group_override(), runs, &wave)) return rc;
    return hca::launch_encode_packed(d_pcm, r->L.cls, runs.d, runs.count, wave, d_frames, pow, d_status, (hipStream_t)stream,
                                     runs.d_loops);
}

}  // namespace

extern "C" {

int vga_hca_ragged_layout_for(const vga_hca_info *infos, int nstreams, int64_t *frame_offsets_out, int64_t *pcm_row_offsets_out,
                              vga_hca_ragged_totals *totals_out)
{
    if (!frame_offsets_out && !pcm_row_offsets_out && !totals_out) { set_error("vga_hca_ragged_layout_for: no output"); return VGA_ERR_ARGUMENT; }
    RaggedLayout L;
    if (int rc = hca::make_layout(infos, nstreams, L)) return rc;
    if (frame_offsets_out) std::copy(L.frame_at.begin(), L.frame_at.end(), frame_offsets_out);
    if (pcm_row_offsets_out) std::copy(L.row_at.begin(), L.row_at.end(), pcm_row_offsets_out);
    if (totals_out) *totals_out = L.totals;
    return VGA_OK;
}

int vga_hca_ragged_create(const vga_hca_info *infos, int nstreams, vga_hca_ragged **out)
{
    if (!out) { set_error("null output"); return VGA_ERR_ARGUMENT; }
    *out = nullptr;
    vga_hca_ragged *r = new vga_hca_ragged;
    int rc = hca::make_layout(infos, nstreams, r->L);
    if (!rc) rc = require_device();
    if (!rc) {
        (void)hipGetDevice(&r->device);
        rc = upload_tables(*r);
    }
    if (rc) {
        delete r;
        return rc;
    }
    *out = r;
    return VGA_OK;
}

void vga_hca_ragged_destroy(vga_hca_ragged *r) { delete r; }

int vga_hca_ragged_streams(const vga_hca_ragged *r) { return r ? (int)r->L.infos.size() : 0; }

int vga_hca_ragged_totals_of(const vga_hca_ragged *r, vga_hca_ragged_totals *out)
{
    if (!r || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    *out = r->L.totals;
    return VGA_OK;
}

int vga_hca_ragged_offsets(const vga_hca_ragged *r, int64_t *frame_offsets_out, int64_t *pcm_row_offsets_out)
{
    if (!r) { set_error("null vga_hca_ragged"); return VGA_ERR_ARGUMENT; }
    if (frame_offsets_out) std::copy(r->L.frame_at.begin(), r->L.frame_at.end(), frame_offsets_out);
    if (pcm_row_offsets_out) std::copy(r->L.row_at.begin(), r->L.row_at.end(), pcm_row_offsets_out);
    return VGA_OK;
}

int vga_hca_decode_device_v(const vga_hca_ragged *r, const uint8_t *d_frames, int16_t *d_pcm, void *d_workspace,
                            size_t workspace_bytes, int *d_status, void *stream)
{
    if (int rc = check_object(r, "vga_hca_decode_device_v")) return rc;
    const vga_hca_ragged_totals &t = r->L.totals;
    if (t.total_frames <= 0) return VGA_OK;
    if (!d_frames || !d_status || !d_workspace || (!d_pcm && t.pcm_samples > 0)) { set_error("vga_hca_decode_device_v: null pointer"); return VGA_ERR_ARGUMENT; }
    if (((uintptr_t)d_frames & 3) || ((uintptr_t)d_pcm & 15) || ((uintptr_t)d_workspace & 15) || workspace_bytes < t.decode_workspace_bytes) {
        set_error("bad alignment / workspace for vga_hca_decode_device_v (frames need 4-byte alignment, PCM and workspace 16, the workspace %zu bytes)",
                  t.decode_workspace_bytes);
        return VGA_ERR_ARGUMENT;
    }
    RunTable runs;
    bool wave = false;
    if (int rc = runs_for_call(r, false, hca_frames_per_group_override(), runs, &wave)) return rc;
    return hca::launch_decode_packed(d_frames, r->L.cls, t.total_frames, r->d_scan, runs.d, runs.count, d_pcm, d_workspace, d_status,
                                     (hipStream_t)stream);
}

int vga_hca_encode_device_v(const vga_hca_ragged *r, const int16_t *d_pcm, uint8_t *d_frames, int *d_status, void *stream)
{
    if (int rc = check_object(r, "vga_hca_encode_device_v")) return rc;
    return encode_call(r, d_pcm, d_frames, d_status, stream, false, "vga_hca_encode_device_v");
}

int vga_hca_encode_loops_device_v(const vga_hca_ragged *r, const int16_t *d_pcm, uint8_t *d_frames, int *d_status, void *stream)
{
    if (int rc = check_object(r, "vga_hca_encode_loops_device_v")) return rc;
    return encode_call(r, d_pcm, d_frames, d_status, stream, true, "vga_hca_encode_loops_device_v");
}

int vga_hca_loop_may_read_tail(const vga_hca_info *info)
{
    if (!info) { set_error("null HcaInfo"); return VGA_ERR_ARGUMENT; }
    hca::PcmMap m;
    if (int rc = hca::make_pcm_map(*info, info->sample_count, m)) return rc;
    if (!info->looping) return 0;
    // SaveLoopAudio (CriHcaEncoder.cs:244-254) fills _postAudio from the loop start on; a loop shorter than the post audio
    // makes it run on into what the file holds behind HcaInfo.SampleCount
    const int post = m.post_end - m.main_end, loop_len = info->sample_count - m.loop_start;
    return loop_len < post ? 1 : 0;
}

int vga_testing_hca_ragged_stats(const void *ragged, long long *out, int n)
{
    const vga_hca_ragged *r = static_cast<const vga_hca_ragged *>(ragged);
    if (!r) return 4;
    const long long total = r->L.totals.total_frames;
    const long long v[4] = {total, (total + 63) / 64 * 64, r->dec_runs.count, r->dec_runs.count};
    for (int i = 0; out && i < n && i < 4; i++) out[i] = v[i];
    return 4;
}

}  // extern "C"
