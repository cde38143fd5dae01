// adx_host.hpp -- the host side of CRI ADX without HIP: the parameter check of every entry point, the encoded size, and for a
// ragged device-resident batch (include/vgaudio_hip/adx_ragged.h) the packed layout, the longest-first work slots, the time
// pieces and the table of (group, piece) items the kernels are launched over, and how the caller's workspace is cut.
// Header-only and free of <hip/hip_runtime.h>, so that a stand-alone host program can include it
// (tests/host/adx_host_driver.cpp) as the C-ABI files do; whoever includes it supplies vga::set_error.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../../include/vgaudio_hip/adx_ragged.h"

namespace vga {

void set_error(const char *fmt, ...);               // (common.hpp)

namespace adx {

inline int64_t pad_to(int64_t v, int64_t m) { return (v + m - 1) / m * m; }           // (common.hpp's round_up)

// what every ADX entry point asks of its parameters
inline int validate(const vga_adx_params *p)
{
    if (!p) { set_error("null ADX parameters"); return VGA_ERR_ARGUMENT; }
    if (p->frame_size < 4 || (p->frame_size & 1) || p->frame_size > 255) {
        set_error("ADX frame size %d unsupported (even, 4..254)", p->frame_size);
        return VGA_ERR_ARGUMENT;
    }
    if (p->type != 2 && p->type != 3 && p->type != 4) { set_error("ADX type %d unknown", p->type); return VGA_ERR_ARGUMENT; }
    if (p->type == 2 && (p->filter < 0 || p->filter > 3)) {
        set_error("ADX fixed filter %d out of range", p->filter);       // Coefs[c.Filter] throws
        return VGA_ERR_ARGUMENT;
    }
    if (p->padding < 0) { set_error("negative padding"); return VGA_ERR_ARGUMENT; }
    if (p->type != 2 && p->sample_rate <= 0) { set_error("sample rate must be positive"); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

// frames / bytes of CriAdxCodec.Encode's output (CriAdxCodec.cs:59-62) for valid parameters
inline int64_t encoded_frames(int pcm_length, const vga_adx_params &p)
{
    const int spf = (p.frame_size - 2) * 2;
    return ((int64_t)pcm_length + p.padding + spf - 1) / spf;
}
inline int64_t encoded_bytes(int pcm_length, const vga_adx_params &p) { return encoded_frames(pcm_length, p) * p.frame_size; }

// ---- time pieces (seams.hpp's plan_pieces with the test hook's count as an argument): `want` pieces of a stream of
// `frames` frames, each at least `min_frames` long, at most MAX_PIECES; hook > 0 wins, down to pieces of `hook_floor`
// frames.  seg_frames is a multiple of `align`.
constexpr int MAX_PIECES = 64;
struct Pieces {
    int segments = 1, seg_frames = 2;
};
inline Pieces cut_pieces(int frames, int want, int min_frames, int hook_floor, int align, int hook)
{
    int segments = want;
    if (segments > frames / min_frames) segments = frames / min_frames;
    if (segments < 1) segments = 1;
    if (segments > MAX_PIECES) segments = MAX_PIECES;
    if (hook > 0) segments = std::min(std::max(frames / hook_floor, 1), hook);
    if (segments > MAX_PIECES) segments = MAX_PIECES;
    Pieces out;
    out.segments = segments;
    out.seg_frames = std::max(((frames + segments - 1) / segments + align - 1) / align * align, align);
    return out;
}
// the launchers' figures (adx_kernels.hip: launch_encode / launch_decode)
constexpr int ENCODE_WAVES_PER_SIMD = 2, ENCODE_MIN_PIECE_FRAMES = 2560, ENCODE_HOOK_FLOOR = 64;
constexpr int DECODE_WAVES_PER_SIMD = 1, DECODE_MIN_PIECE_FRAMES = 512, DECODE_HOOK_FLOOR = 8;

// ---- ragged batches
constexpr int64_t GUARD_BYTES = 256;      // after the last row of a packed buffer (gc::GUARD_BYTES): clamped loads of short rows stay inside
constexpr int GROUP_SLOTS = 64;           // work slots per group = lanes of the wave that runs one piece of them

// one direction's launch plan: the pieces of the longest channel and the (group, piece) items whose first frame lies
// inside the group's longest channel -- no launched wave lies wholly behind its group's frames
struct RaggedPlan {
    Pieces pieces;
    std::vector<int32_t> items;           // pairs: group, piece (group-major)
    int item_count() const { return (int)(items.size() / 2); }
};

struct RaggedLayout {
    vga_adx_params p = {};
    int count = 0;
    std::vector<int> length, order;            // order: work slot -> channel, longest first (stable)
    std::vector<int64_t> pcm_off, adx_off;     // samples / bytes, per CHANNEL
    std::vector<int> group_frames;             // per group of 64 work slots: the encoded frames of its longest channel (slot 0)
    std::vector<int64_t> crumb_base;           // per group: where its [group_frames][64] block of crumbs starts (in crumbs)
    int64_t lane_frames = 0;                   // 64 * sum(group_frames): the lane-frames a full set of pieces launches
    bool time_pieces = false;                  // 18-byte frames, no padding: the time-piece kernels
    int first_empty = -1;                      // first channel of 0 samples
    vga_adx_ragged_totals totals = {};

    int groups() const { return (int)group_frames.size(); }
    int slots() const { return groups() * GROUP_SLOTS; }
};

// The caller's workspace, encoder: [segments][slots] final histories (2 shorts), [slots] first open seam,
// [segments - 1][slots] seam_open and seam_end, the fix-up's queue and the open seams' count (16 bytes), then the crumbs,
// 8 bytes per frame and lane, group after group.  Every part is a multiple of 16 bytes (slots is a multiple of 64).
struct EncodeWorkspace {
    size_t state_at = 0, first_open_at = 0, seam_open_at = 0, seam_end_at = 0, queue_at = 0, crumbs_at = 0, bytes = 0;
    size_t flag_bytes = 0;
};
inline EncodeWorkspace cut_encode_workspace(int slots, int segments, int64_t lane_frames)
{
    EncodeWorkspace w;
    w.flag_bytes = (size_t)(segments - 1) * slots * sizeof(int);
    w.state_at = 0;
    w.first_open_at = w.state_at + (size_t)segments * slots * 2 * sizeof(int16_t);
    w.seam_open_at = w.first_open_at + (size_t)slots * sizeof(int);
    w.seam_end_at = w.seam_open_at + w.flag_bytes;
    w.queue_at = w.seam_end_at + w.flag_bytes;
    w.crumbs_at = w.queue_at + 16;
    w.bytes = w.crumbs_at + (size_t)lane_frames * 8;
    return w;
}
// ... decoder: [slots] first open seam, [segments - 1][slots] seam_open, slow_seams (16 bytes), and a line of 64 x 16
// bytes that takes the turned stores of rows that have ended (adx_decode_fs18_direct_ragged_kernel)
constexpr size_t DECODE_SINK_BYTES = 1024;
struct DecodeWorkspace {
    size_t first_open_at = 0, seam_open_at = 0, slow_at = 0, sink_at = 0, bytes = 0, flag_bytes = 0;
};
inline DecodeWorkspace cut_decode_workspace(int slots, int segments)
{
    DecodeWorkspace w;
    w.flag_bytes = (size_t)(segments - 1) * slots * sizeof(int);
    w.first_open_at = 0;
    w.seam_open_at = (size_t)slots * sizeof(int);
    w.slow_at = w.seam_open_at + w.flag_bytes;
    w.sink_at = w.slow_at + 16;
    w.bytes = w.sink_at + DECODE_SINK_BYTES;
    return w;
}

inline int make_layout(const vga_adx_params *p, const int *sample_counts, int nch, RaggedLayout &L)
{
    if (int rc = validate(p)) return rc;
    if (nch < 0) { set_error("negative channel count"); return VGA_ERR_ARGUMENT; }
    if (nch > 0 && !sample_counts) { set_error("null sample counts"); return VGA_ERR_ARGUMENT; }
    for (int c = 0; c < nch; c++)
        if (sample_counts[c] < 0) { set_error("channel %d has a negative sample count", c); return VGA_ERR_ARGUMENT; }
    L.p = *p;
    L.count = nch;
    L.length.assign(sample_counts, sample_counts + nch);
    L.order.resize(nch);
    L.pcm_off.resize(nch);
    L.adx_off.resize(nch);
    std::iota(L.order.begin(), L.order.end(), 0);
    std::stable_sort(L.order.begin(), L.order.end(), [&](int a, int b) { return L.length[a] > L.length[b]; });
    int64_t pcm_at = 0, adx_at = 0, frames = 0;
    L.first_empty = -1;
    for (int c = 0; c < nch; c++) {
        if (encoded_bytes(L.length[c], *p) > INT32_MAX) { set_error("channel %d: the encoded stream exceeds 2 GiB", c); return VGA_ERR_ARGUMENT; }
        L.pcm_off[c] = pcm_at;
        L.adx_off[c] = adx_at;
        pcm_at += pad_to(L.length[c], 8);
        adx_at += pad_to(encoded_bytes(L.length[c], *p), 16);
        frames += encoded_frames(L.length[c], *p);
        if (L.length[c] == 0 && L.first_empty < 0) L.first_empty = c;
    }
    L.time_pieces = p->frame_size == 18 && p->padding == 0;
    L.group_frames.assign((nch + GROUP_SLOTS - 1) / GROUP_SLOTS, 0);
    L.crumb_base.assign(L.group_frames.size(), 0);
    L.lane_frames = 0;
    for (size_t g = 0; g < L.group_frames.size(); g++) {
        L.group_frames[g] = (int)encoded_frames(L.length[L.order[g * GROUP_SLOTS]], *p);
        L.crumb_base[g] = L.lane_frames;
        L.lane_frames += (int64_t)GROUP_SLOTS * L.group_frames[g];
    }
    L.totals.pcm_samples = pcm_at + GUARD_BYTES / 2;
    L.totals.adx_bytes = adx_at + GUARD_BYTES;
    L.totals.channels = nch;
    L.totals.total_frames = frames;
    // sizes that hold for any plan of up to MAX_PIECES pieces; the general kernels need no scratch
    const bool scratch = L.time_pieces && nch > 0;
    L.totals.encode_workspace_bytes = scratch ? cut_encode_workspace(L.slots(), MAX_PIECES, L.lane_frames).bytes : 0;
    L.totals.decode_workspace_bytes = scratch ? cut_decode_workspace(L.slots(), MAX_PIECES).bytes : 0;
    return VGA_OK;
}

// The plan of one direction for a chip of `cus` compute units (hook: vga_testing_gc_encoder_segments_this_thread's count).
// The general kernels walk a channel as one piece.
inline RaggedPlan make_plan(const RaggedLayout &L, int cus, int hook, bool encode)
{
    RaggedPlan plan;
    const int groups = L.groups();
    if (groups == 0) return plan;
    if (!L.time_pieces) hook = 1;
    // The launchers' arithmetic on the longest channel -- waves wanted / groups -- with the groups counted by the frames they
    // hold: sum(group_frames) / group_frames[0] groups of the longest channel's length (the same number for equal lengths).
    // Counting every group as a full-length one would cut a batch of one long file beside thousands of short ones into
    // pieces that leave most of the chip idle (GC-ADPCM's ragged plan divides the batch's own frames too).
    const int frames = L.group_frames[0];
    const int64_t waves = (int64_t)cus * 4 * (encode ? ENCODE_WAVES_PER_SIMD : DECODE_WAVES_PER_SIMD);
    const int want = (int)std::min<int64_t>(MAX_PIECES, frames > 0 ? waves * frames / (L.lane_frames / GROUP_SLOTS) : waves / groups);
    plan.pieces = encode ? cut_pieces(frames, want, ENCODE_MIN_PIECE_FRAMES, ENCODE_HOOK_FLOOR, 2, hook)
                         : cut_pieces(frames, want, DECODE_MIN_PIECE_FRAMES, DECODE_HOOK_FLOOR, 2, hook);
    for (int g = 0; g < groups; g++)
        for (int k = 0; k < plan.pieces.segments && (int64_t)k * plan.pieces.seg_frames < L.group_frames[g]; k++) {
            plan.items.push_back(g);
            plan.items.push_back(k);
        }
    return plan;
}

}  // namespace adx
}  // namespace vga
