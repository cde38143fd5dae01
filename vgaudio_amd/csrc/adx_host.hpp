// adx_host.hpp -- the host side of CRI ADX without HIP: the predictor coefficients and the kernels' parameters, the
// CriAdxHelpers conversions, the sizes, every entry point's argument checks, the time pieces and their figures, and for a
// ragged device-resident batch (include/vgaudio_hip/adx_ragged.h) the packed layout, the longest-first work slots, the table
// of (group, piece) items the kernels are launched over, and how the caller's workspace is cut.
// Header-only and free of <hip/hip_runtime.h>, so that a stand-alone host program can include it
// (tests/host/adx_host_driver.cpp) as the kernel and C-ABI files do (adx_kernels.hpp); whoever includes it supplies vga::set_error.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
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

// ---- the predictor coefficients (CriAdxCodec.cs:173-191; host side: libm cos / sqrt, as the reference uses Math.Cos / Math.Sqrt)
constexpr int16_t FIXED_COEFS[4][2] = {{0, 0}, {0x0F00, 0}, {0x1CC0, (int16_t)0xF300}, {0x1880, (int16_t)0xF240}};
inline void calculate_coefficients(int highpass_freq, int sample_rate, int16_t coefs[2])
{
    const double sqrt2 = std::sqrt(2.0);
    const double a = sqrt2 - std::cos(2.0 * M_PI * highpass_freq / sample_rate);
    const double b = sqrt2 - 1;
    const double c = (a - std::sqrt((a + b) * (a - b))) / b;
    coefs[0] = (int16_t)(int)(c * 8192);
    coefs[1] = (int16_t)(int)(c * c * -4096);
}
// What the kernels take: CriAdxParameters (Codecs/CriAdx/CriAdxParameters.cs:5-12) with the two predictor coefficients
// resolved on the host (Fixed: Coefs[Filter]; else CalculateCoefficients).  Eight ints without padding: equal values are equal bytes.
struct AdxDeviceParams {
    int frame_size, version, type, filter, padding, history;   // type: 2 Fixed, 3 Linear, 4 Exponential
    int coef0, coef1;
};
// ... of valid parameters: the encoder's high-pass is 500 Hz (CriAdxCodec.cs:64), the decoder takes the stream's (:13)
inline AdxDeviceParams make_device_params(const vga_adx_params *p, bool encode)
{
    int16_t c[2] = {FIXED_COEFS[p->filter & 3][0], FIXED_COEFS[p->filter & 3][1]};
    if (p->type != 2) calculate_coefficients(encode ? 500 : p->highpass_frequency, p->sample_rate, c);
    return {p->frame_size, p->version, p->type, p->filter, p->padding, p->history, c[0], c[1]};
}

// ---- Formats/CriAdx/CriAdxHelpers.cs:7-31
inline int nibble_count_to_sample_count(int nibble_count, int frame_size)
{
    const int npf = frame_size * 2, spf = npf - 4;
    const int frames = nibble_count / npf, extra = nibble_count % npf;
    return spf * frames + (extra < 4 ? 0 : extra - 4);
}
inline int sample_count_to_nibble_count(int sample_count, int frame_size)
{
    const int npf = frame_size * 2, spf = npf - 4;
    const int frames = sample_count / spf, extra = sample_count % spf;
    return npf * frames + (extra == 0 ? 0 : extra + 4);
}
inline int sample_count_to_byte_count(int sample_count, int frame_size)
{
    const int n = sample_count_to_nibble_count(sample_count, frame_size);
    return (n / 2) + (n & 1);
}

// ---- sizes
// Extensions.cs:145, (int)Math.Ceiling((double)v / d), for every int v and d > 0: the quotient truncates towards zero, so
// only a positive remainder rounds up (-7 / 2 is -3 and stays -3)
inline int divide_by_round_up(int v, int d) { return v / d + (v % d > 0 ? 1 : 0); }
// Bytes of CriAdxCodec.Encode's output (CriAdxCodec.cs:59-62) as the reference computes them and vga_adx_encoded_byte_count
// returns them: in ints, so pcm_length + padding wraps above 2^31 - 1 and so does the product -- where encoded_bytes() parts.
inline int encoded_byte_count(int pcm_length, const vga_adx_params &p) { return divide_by_round_up(pcm_length + p.padding, (p.frame_size - 2) * 2) * p.frame_size; }
// ... and without the wrap, for make_layout, which refuses a stream above 2 GiB: equal while pcm_length + padding and the bytes fit an int
inline int64_t encoded_frames(int pcm_length, const vga_adx_params &p)
{
    const int spf = (p.frame_size - 2) * 2;
    return ((int64_t)pcm_length + p.padding + spf - 1) / spf;
}
inline int64_t encoded_bytes(int pcm_length, const vga_adx_params &p) { return encoded_frames(pcm_length, p) * p.frame_size; }
// bytes CriAdxCodec.Decode reads (CriAdxCodec.cs:18-24): up to the frame the padding ends in, then ceil(sample_count / spf) frames
inline int64_t decode_bytes_read(int sample_count, const vga_adx_params &p)
{
    const int spf = (p.frame_size - 2) * 2;
    return (int64_t)(p.padding / spf) * p.frame_size + (int64_t)divide_by_round_up(sample_count, spf) * p.frame_size;
}

// a channel's own frames of the padded stream in a bucket of the ragged host encoder (d_own_frames): the 18-byte kernels', of 32 samples
constexpr int OWN_FRAME_SAMPLES = 32;
inline int own_frames(int pcm_length, const vga_adx_params &p) { return divide_by_round_up(pcm_length + p.padding, OWN_FRAME_SAMPLES); }

// ---- argument checks, each list in the order its entry point applies it: of two bad arguments the first one's message is
// the call's.  A call with nothing to do (no channels, no samples) passes: the caller asks again.
inline int check_pcm_not_empty(int pcm_length, const vga_adx_params &p, int channel = -1)   // channel >= 0: of a ragged call
{
    if (pcm_length != 0 || p.version != 4 || p.padding != 0) return VGA_OK;
    char who[32] = "";
    if (channel >= 0) snprintf(who, sizeof who, "channel %d: ", channel);
    set_error("%sempty PCM: the reference reads pcm[0] (CriAdxCodec.cs:71)", who);
    return VGA_ERR_ARGUMENT;
}
// the row arrays of an equal-length call, if it is one of host rows (in_needed: the input rows hold something)
inline int check_rows(bool host_rows, const void *const *in, const void *const *out, int nch, bool in_needed)
{
    if (!host_rows) return VGA_OK;
    if (!in || !out) { set_error("null channel array"); return VGA_ERR_ARGUMENT; }
    for (int c = 0; c < nch; c++)
        if ((!in[c] && in_needed) || !out[c]) { set_error("channel %d is null", c); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}
// an equal-length encode; host_rows: of the host rows (pcm, out), else of device rows: check_encode_device_layout follows
inline int check_encode(const vga_adx_params *p, int nch, int pcm_length, bool host_rows = false, const int16_t *const *pcm = nullptr, uint8_t *const *out = nullptr)
{
    if (int rc = validate(p)) return rc;
    if (nch < 0 || pcm_length < 0) { set_error("negative size"); return VGA_ERR_ARGUMENT; }
    if (nch == 0) return VGA_OK;
    if (int rc = check_rows(host_rows, (const void *const *)pcm, (const void *const *)out, nch, pcm_length > 0)) return rc;
    return check_pcm_not_empty(pcm_length, *p);
}
inline int check_encode_device_layout(int64_t pcm_pitch, int pcm_length, const void *d_out, int64_t out_pitch, int nbytes)
{
    if (pcm_pitch >= pcm_length && out_pitch >= nbytes && !(out_pitch & 1) && !((uintptr_t)d_out & 1)) return VGA_OK;
    set_error("bad pitch/alignment (pcm_pitch=%lld, out_pitch=%lld, need >= %d and even)", (long long)pcm_pitch, (long long)out_pitch, nbytes);
    return VGA_ERR_ARGUMENT;
}
// the stream holds what the decoder reads (IndexOutOfRange in C#) and the device rows their lengths: one refusal
inline int check_decode_device_layout(int adpcm_length, int64_t in_pitch, int sample_count, int64_t pcm_pitch, const vga_adx_params &p)
{
    const long long need = decode_bytes_read(sample_count, p);
    if (adpcm_length >= need && in_pitch >= adpcm_length && pcm_pitch >= sample_count) return VGA_OK;
    set_error("ADX stream too short: %d bytes, decoder reads %lld", adpcm_length, need);
    return VGA_ERR_ARGUMENT;
}
// an equal-length decode of device rows at (in_pitch, pcm_pitch), or of the host rows (adpcm, pcm_out): their pitches are their lengths
inline int check_decode(const vga_adx_params *p, int adpcm_length, int nch, int sample_count, int64_t in_pitch, int64_t pcm_pitch,
                        bool host_rows = false, const uint8_t *const *adpcm = nullptr, int16_t *const *pcm_out = nullptr)
{
    if (int rc = validate(p)) return rc;
    if (nch < 0 || sample_count < 0 || adpcm_length < 0) { set_error("negative size"); return VGA_ERR_ARGUMENT; }
    if (nch == 0 || sample_count == 0) return VGA_OK;
    if (int rc = check_rows(host_rows, (const void *const *)adpcm, (const void *const *)pcm_out, nch, true)) return rc;
    return check_decode_device_layout(adpcm_length, in_pitch, sample_count, pcm_pitch, *p);
}
// the ragged host calls: the arrays, then channel by channel
inline int check_encode_v(const int16_t *const *pcm, const int *lengths, int nch, const vga_adx_params *params, uint8_t *const *out)
{
    if (nch < 0) { set_error("negative channel count"); return VGA_ERR_ARGUMENT; }
    if (nch == 0) return VGA_OK;
    if (!pcm || !lengths || !params || !out) { set_error("null array"); return VGA_ERR_ARGUMENT; }
    for (int c = 0; c < nch; c++) {
        if (int rc = validate(&params[c])) return rc;
        if (lengths[c] < 0) { set_error("channel %d: negative length", c); return VGA_ERR_ARGUMENT; }
        if (int rc = check_pcm_not_empty(lengths[c], params[c], c)) return rc;
        if ((!pcm[c] && lengths[c] > 0) || !out[c]) { set_error("channel %d is null", c); return VGA_ERR_ARGUMENT; }
    }
    return VGA_OK;
}
inline size_t decode_bytes_read_v(int sample_count, const vga_adx_params &p) { return sample_count == 0 ? 0 : (size_t)decode_bytes_read(sample_count, p); }
inline int check_decode_v(const uint8_t *const *adpcm, const int *adpcm_lengths, int nch, const int *sample_counts,
                          const vga_adx_params *params, int16_t *const *pcm_out)
{
    if (nch < 0) { set_error("negative channel count"); return VGA_ERR_ARGUMENT; }
    if (nch == 0) return VGA_OK;
    if (!adpcm || !adpcm_lengths || !sample_counts || !params || !pcm_out) { set_error("null array"); return VGA_ERR_ARGUMENT; }
    for (int c = 0; c < nch; c++) {
        if (int rc = validate(&params[c])) return rc;
        if (sample_counts[c] < 0 || adpcm_lengths[c] < 0) { set_error("channel %d: negative size", c); return VGA_ERR_ARGUMENT; }
        const size_t need = decode_bytes_read_v(sample_counts[c], params[c]);
        if ((size_t)adpcm_lengths[c] < need) {
            set_error("channel %d: ADX stream too short: %d bytes, decoder reads %zu", c, adpcm_lengths[c], need);
            return VGA_ERR_ARGUMENT;
        }
        if (sample_counts[c] > 0 && (!adpcm[c] || !pcm_out[c])) { set_error("channel %d is null", c); return VGA_ERR_ARGUMENT; }
    }
    return VGA_OK;
}

// ---- time pieces (seams.hpp's plan_pieces with the test hook's count as an argument): `want` pieces of a stream of
// `frames` frames, each at least `min_frames` long, at most MAX_PIECES; hook > 0 wins, down to pieces of `hook_floor`
// frames.  seg_frames is a multiple of `align`.
constexpr int MAX_PIECES = 64;
struct Pieces { int segments = 1, seg_frames = 2; };
inline Pieces cut_pieces(int frames, int want, int min_frames, int hook_floor, int align, int hook)
{
    int segments = want;
    if (segments > frames / min_frames) segments = frames / min_frames;
    if (segments < 1) segments = 1;
    if (segments > MAX_PIECES) segments = MAX_PIECES;
    if (hook > 0) segments = std::min(std::max(frames / hook_floor, 1), hook);
    if (segments > MAX_PIECES) segments = MAX_PIECES;
    return {segments, std::max(((frames + segments - 1) / segments + align - 1) / align * align, align)};
}
// The pieces' figures, of the equal-length launchers (adx_kernels.hip, which says what was measured) and of the ragged plan
// below alike: waves per SIMD, a piece's least frames, the same under the test hook; a piece is a multiple of PIECE_ALIGN_FRAMES
constexpr int ENCODE_WAVES_PER_SIMD = 2, ENCODE_MIN_PIECE_FRAMES = 2560, ENCODE_HOOK_FLOOR = 64;
constexpr int DECODE_WAVES_PER_SIMD = 1, DECODE_MIN_PIECE_FRAMES = 512, DECODE_HOOK_FLOOR = 8, PIECE_ALIGN_FRAMES = 2;

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
    plan.pieces = encode ? cut_pieces(frames, want, ENCODE_MIN_PIECE_FRAMES, ENCODE_HOOK_FLOOR, PIECE_ALIGN_FRAMES, hook)
                         : cut_pieces(frames, want, DECODE_MIN_PIECE_FRAMES, DECODE_HOOK_FLOOR, PIECE_ALIGN_FRAMES, hook);
    for (int g = 0; g < groups; g++)
        for (int k = 0; k < plan.pieces.segments && (int64_t)k * plan.pieces.seg_frames < L.group_frames[g]; k++) {
            plan.items.push_back(g);
            plan.items.push_back(k);
        }
    return plan;
}

}  // namespace adx
}  // namespace vga
