// gc_host.hpp -- the host side of GC-ADPCM without HIP: the GcAdpcmMath conversions, the channel-metadata and DSP layouts,
// the alignment plan of vga_gcadpcm_build_channels_device, the argument checks of the entry points, the packed layout of a
// ragged batch, the chunk cut of a ragged host call and its longest-first order.  Header-only and free of
// <hip/hip_runtime.h>, so that a stand-alone host program can include it (tests/host/gc_host_driver.cpp) as the C-ABI
// files do (gc_capi.hpp); whoever includes it supplies vga::set_error.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../../include/vgaudio_hip.h"

namespace vga {

void set_error(const char *fmt, ...);               // (common.hpp)

namespace gc {

inline int64_t pad_to(int64_t v, int64_t m) { return (v + m - 1) / m * m; }           // (common.hpp's round_up)

// ---- GcAdpcmMath.cs:11-47
inline int divide_by2_round_up(int v) { return (v / 2) + (v & 1); }
inline int divide_by_round_up(int v, int d) { return v / d + (v % d != 0 ? 1 : 0); }   // Utilities/Extensions.cs:145
inline int get_next_multiple(int value, int multiple)                                  // Utilities/Helpers.cs:71-80
{
    if (multiple <= 0) return value;
    if (value % multiple == 0) return value;
    return value + multiple - value % multiple;
}
inline int nibble_count_to_sample_count(int nibble_count)
{
    int frames = nibble_count / 16;
    int extra_nibbles = nibble_count % 16;
    int extra_samples = extra_nibbles < 2 ? 0 : extra_nibbles - 2;
    return 14 * frames + extra_samples;
}
inline int sample_count_to_nibble_count(int sample_count)
{
    int frames = sample_count / 14;
    int extra_samples = sample_count % 14;
    int extra_nibbles = extra_samples == 0 ? 0 : extra_samples + 2;
    return 16 * frames + extra_nibbles;
}
inline int nibble_to_sample(int nibble)
{
    int frames = nibble / 16;
    int extra_nibbles = nibble % 16;
    return 14 * frames + extra_nibbles - 2;
}
inline int sample_to_nibble(int sample)
{
    int frames = sample / 14;
    int extra_samples = sample % 14;
    return 16 * frames + extra_samples + 2;
}
inline int sample_count_to_byte_count(int sample_count) { return divide_by2_round_up(sample_count_to_nibble_count(sample_count)); }
inline int byte_count_to_sample_count(int byte_count) { return nibble_count_to_sample_count(byte_count * 2); }

// ---- argument checks
inline int check_pcm_layout(const void *p, int64_t pitch, int n, const char *what)
{
    if (((uintptr_t)p & 3) != 0 || (pitch & 1) != 0 || pitch < n) {
        set_error("%s: base must be 4-byte aligned and pitch even and >= length (pitch=%lld, n=%d)", what,
                  (long long)pitch, n);
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}
inline int check_adpcm_layout(const void *p, int64_t pitch, int nbytes, const char *what)
{
    if (((uintptr_t)p & 7) != 0 || (pitch & 7) != 0 || pitch < nbytes) {
        set_error("%s: base must be 8-byte aligned and pitch a multiple of 8 and >= byte count (pitch=%lld, bytes=%d)",
                  what, (long long)pitch, nbytes);
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}
inline int check_ptrs(const void *const *pp, int nch, const char *what)
{
    if (nch < 0) { set_error("%s: negative channel count", what); return VGA_ERR_ARGUMENT; }
    if (nch > 0 && !pp) { set_error("%s: null channel array", what); return VGA_ERR_ARGUMENT; }
    for (int c = 0; c < nch; c++)
        if (!pp[c]) { set_error("%s: channel %d is null", what, c); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}
inline int check_counts(const int *counts, int n, const char *what)
{
    if (n < 0) { set_error("%s: negative channel count", what); return VGA_ERR_ARGUMENT; }
    if (n > 0 && !counts) { set_error("%s: null sample counts", what); return VGA_ERR_ARGUMENT; }
    for (int c = 0; c < n; c++)
        if (counts[c] < 0) { set_error("%s: channel %d has a negative sample count", what, c); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}
inline int check_rows(const void *const *pp, const int *counts, int n, const char *what)
{
    if (n > 0 && !pp) { set_error("%s: null channel array", what); return VGA_ERR_ARGUMENT; }
    for (int c = 0; c < n; c++)
        if (counts[c] > 0 && !pp[c]) { set_error("%s: channel %d is null", what, c); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}
// the ragged host calls' arguments, before anything is read through the arrays (with_coefs: the coefficients are searched
// for and handed out, adpcm_out may then be null; else they are coefs_in)
inline int check_encode_v(const int16_t *const *pcm, const int *counts, int nch, const int16_t *coefs_out, uint8_t *const *adpcm_out,
                          bool with_coefs, const int16_t *coefs_in)
{
    if (int rc = check_counts(counts, nch, "sample_counts")) return rc;
    if (int rc = check_rows((const void *const *)pcm, counts, nch, "pcm")) return rc;
    if (adpcm_out || !with_coefs)
        if (int rc = check_rows((const void *const *)adpcm_out, counts, nch, "adpcm_out")) return rc;
    if (nch > 0 && with_coefs && !coefs_out) { set_error("null coefs_out"); return VGA_ERR_ARGUMENT; }
    if (nch > 0 && !with_coefs && !coefs_in) { set_error("null coefs"); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}
inline int check_decode_v(const uint8_t *const *adpcm, const int16_t *coefs, const int *counts, int nch, int16_t *const *pcm_out)
{
    if (int rc = check_counts(counts, nch, "sample_counts")) return rc;
    if (int rc = check_rows((const void *const *)adpcm, counts, nch, "adpcm")) return rc;
    if (int rc = check_rows((const void *const *)pcm_out, counts, nch, "pcm_out")) return rc;
    if (nch > 0 && !coefs) { set_error("null coefs"); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

// ---- channel metadata
inline int channel_layout_for(const vga_gcadpcm_channel_params *p, vga_gcadpcm_channel_layout *out)
{
    if (!p || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (p->sample_count < 0 || p->loop_start < 0 || p->loop_end < p->loop_start || p->loop_alignment_multiple < 0 ||
        p->samples_per_seek_table_entry < 0) {
        set_error("channel parameters out of range (samples %d, loop %d..%d, alignment %d, seek entry %d)", p->sample_count,
                  p->loop_start, p->loop_end, p->loop_alignment_multiple, p->samples_per_seek_table_entry);
        return VGA_ERR_OUT_OF_RANGE;
    }
    const int multiple = p->loop_alignment_multiple;
    out->alignment_needed = (multiple != 0 && p->loop_start % multiple != 0) ? 1 : 0;    // Helpers.cs:82-83
    out->loop_start_aligned = p->loop_start;
    out->sample_count_aligned = p->sample_count;
    if (out->alignment_needed) {                                                         // GcAdpcmAlignment.cs:29-31
        const int64_t aligned = (int64_t)p->loop_start + multiple - p->loop_start % multiple;
        const int64_t count = (int64_t)p->loop_end + (aligned - p->loop_start);
        if (count > 0x7FFFFFFF - 16) { set_error("aligned sample count overflows"); return VGA_ERR_OUT_OF_RANGE; }
        out->loop_start_aligned = get_next_multiple(p->loop_start, multiple);
        out->sample_count_aligned = (int)count;
    }
    out->seek_table_entries = p->samples_per_seek_table_entry != 0                       // GcAdpcmSeekTable.cs:27
        ? divide_by_round_up(out->sample_count_aligned, p->samples_per_seek_table_entry) : 0;
    return VGA_OK;
}

inline size_t build_channels_workspace_bytes(int nch, const vga_gcadpcm_channel_params *p)
{
    vga_gcadpcm_channel_layout L;
    if (nch <= 0 || channel_layout_for(p, &L) != VGA_OK) return 0;
    // decoded PCM (caller may not want it) + the re-encode input + two history arrays + a status word
    size_t bytes = (size_t)nch * (size_t)pad_to(L.sample_count_aligned > 0 ? L.sample_count_aligned : 1, 8) * 2;
    if (L.alignment_needed) {
        const int keep = p->loop_end / 14 * 14;
        bytes += (size_t)nch * (size_t)pad_to(L.sample_count_aligned - keep + 1, 8) * 2;
    }
    return bytes + (size_t)pad_to(nch * 2, 16) * 2 + 64;
}

// The numbers of vga_gcadpcm_build_channels_device: where its workspace is cut and, when the loop needs alignment
// (GcAdpcmAlignment.cs:33-62), what is kept of the stream and what is encoded again.  Offsets are bytes from the workspace.
struct ChannelsPlan {
    int64_t ws_pcm_pitch = 0;                      // samples: rows of the decoded PCM when it lives in the workspace
    int frames_to_keep = 0, bytes_to_keep = 0, samples_to_keep = 0, samples_to_encode = 0;
    int64_t new_pitch = 0;                         // samples: rows of the tail to encode
    size_t new_pcm_at = 0, hist1_at = 0, hist2_at = 0;
};
// the refusals that need the layout: the loop context's read, then the loop that cannot be aligned
inline int plan_channels(const vga_gcadpcm_channel_params *p, const vga_gcadpcm_channel_layout &L, int nch, bool want_ctx,
                         ChannelsPlan &plan)
{
    // the loop context reads the pred/scale byte from the ORIGINAL stream (GcAdpcmChannelBuilder.cs:179)
    if (want_ctx && L.loop_start_aligned != 0 && L.loop_start_aligned / 14 * 8 >= sample_count_to_byte_count(p->sample_count)) {
        set_error("loop context: the aligned loop start (%d) lies past the original ADPCM data (the reference reads "
                  "Adpcm, not AlignedAdpcm: IndexOutOfRangeException)", L.loop_start_aligned);
        return VGA_ERR_OUT_OF_RANGE;
    }
    const int n_al = L.sample_count_aligned;
    plan.ws_pcm_pitch = pad_to(n_al > 0 ? n_al : 1, 8);
    if (!L.alignment_needed) return VGA_OK;
    plan.frames_to_keep = p->loop_end / 14;
    plan.bytes_to_keep = plan.frames_to_keep * 8;
    plan.samples_to_keep = plan.frames_to_keep * 14;
    plan.samples_to_encode = n_al - plan.samples_to_keep;
    if (p->loop_end - p->loop_start <= 0 && p->loop_end - plan.samples_to_keep < plan.samples_to_encode) {
        set_error("a zero-length loop cannot be aligned (the reference's fill loop never ends, GcAdpcmAlignment.cs:48)");
        return VGA_ERR_INVALID_OP;
    }
    plan.new_pitch = pad_to(plan.samples_to_encode + 1, 8);
    plan.new_pcm_at = (size_t)nch * plan.ws_pcm_pitch * 2;
    plan.hist1_at = plan.new_pcm_at + (size_t)nch * plan.new_pitch * 2;
    plan.hist2_at = plan.hist1_at + (size_t)pad_to(nch, 8) * 2;
    return VGA_OK;
}

// ---- DSP container
inline int dsp_layout_for(const vga_dsp_params *p, int nch, vga_dsp_layout *out)
{
    if (!p || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (nch < 1) { set_error("a DSP file needs at least one channel"); return VGA_ERR_ARGUMENT; }
    if (p->samples_per_interleave < 1) {                         // DspConfiguration.cs:31-40
        set_error("Number of samples per interleave must be positive");
        return VGA_ERR_OUT_OF_RANGE;
    }
    if (p->samples_per_interleave % 14 != 0) {
        set_error("Number of samples per interleave must be divisible by 14");
        return VGA_ERR_OUT_OF_RANGE;
    }
    if (p->sample_count < 0 || p->loop_start < 0 || p->loop_end < 0) { set_error("negative sample count / loop point"); return VGA_ERR_OUT_OF_RANGE; }
    // DspWriter.cs:22-36
    const int alignment_samples = get_next_multiple(p->loop_start, p->loop_point_alignment) - p->loop_start;
    out->loop_start = p->loop_start + alignment_samples;
    out->loop_end = p->loop_end + alignment_samples;
    out->sample_count = (p->trim_file && p->looping) ? out->loop_end : std::max(p->sample_count, out->loop_end);
    out->bytes_per_interleave = sample_count_to_byte_count(p->samples_per_interleave);
    out->frames_per_interleave = out->bytes_per_interleave / 8;
    out->start_addr = sample_to_nibble(p->looping ? out->loop_start : 0);
    out->end_addr = sample_to_nibble(p->looping ? out->loop_end : out->sample_count - 1);
    out->cur_addr = sample_to_nibble(0);
    out->audio_data_size = get_next_multiple(sample_count_to_byte_count(out->sample_count), nch == 1 ? 1 : 8);   // :99-100
    const int64_t fs = ((int64_t)0x60 + out->audio_data_size) * nch;                                              // :18
    if (fs > 0x7FFFFFFF) { set_error("DSP file would exceed 2 GiB (the reference's FileSize is an int)"); return VGA_ERR_OUT_OF_RANGE; }
    out->file_size = (int)fs;
    return VGA_OK;
}

// ---- ragged batches
constexpr int64_t GUARD_BYTES = 256;      // after the last row of a packed buffer: clamped loads of short rows stay inside

// Where the rows of one group of channels lie (a whole ragged batch, or one pipeline chunk of it), as the kernels index
// them: LOCAL channel i = 0 .. count-1; offsets count from the device buffers' bases.
struct RaggedLayout {
    int count = 0;
    std::vector<int> length, order;            // order: work slot -> channel, longest first (stable)
    std::vector<int64_t> pcm_off, adpcm_off;   // samples / bytes
    int64_t pcm_end = 0, adpcm_end = 0;        // behind the last row
    int max_length = 0;
    int64_t total_frames = 0;
    bool uniform = false;                      // every channel the same length: the equal-length kernels apply
    int64_t pcm_pitch = 0, adpcm_pitch = 0;    // ... with these pitches
    std::vector<int> group_frames;             // per group of sixteen work slots: the frames of its longest channel (slot 0)

    // lengths[0 .. n); the rows start at pcm_base (samples) / adpcm_base (bytes) and follow each other, every row
    // rounded up to 8 samples / 16 bytes
    void lay_out(const int *lengths, int n, int64_t pcm_base, int64_t adpcm_base)
    {
        count = n;
        length.assign(lengths, lengths + n);
        order.resize(n);
        pcm_off.resize(n);
        adpcm_off.resize(n);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return length[a] > length[b]; });
        max_length = 0;
        total_frames = 0;
        uniform = n > 0;
        for (int c = 0; c < n; c++) {
            pcm_off[c] = pcm_base;
            adpcm_off[c] = adpcm_base;
            pcm_base += pad_to(length[c], 8);
            adpcm_base += pad_to(sample_count_to_byte_count(length[c]), 16);
            total_frames += ((int64_t)length[c] + 13) / 14;
            max_length = std::max(max_length, length[c]);
            uniform = uniform && length[c] == length[0];
        }
        if (uniform) {
            pcm_pitch = pad_to(length[0], 8);
            adpcm_pitch = pad_to(sample_count_to_byte_count(length[0]), 16);
        }
        pcm_end = pcm_base;
        adpcm_end = adpcm_base;
        group_frames.resize((n + 15) / 16);
        for (size_t g = 0; g < group_frames.size(); g++) group_frames[g] = (length[order[g * 16]] + 13) / 14;
    }
};

// channels per pipeline chunk of a ragged host call, by volume: what 1024 channels of BASELINE configs[1] hold (the
// equal-length entry points' chunk); a call below 256 MB of rows is one chunk
constexpr int64_t CHUNK_SAMPLES = (int64_t)1024 * 2880000;

// chunk k = channels [chunk_begin[k], chunk_begin[k + 1]); chunk_units > 0 (the test hook) cuts by channels instead
inline std::vector<int> cut_chunks(const int *counts, int n, int chunk_units)
{
    int64_t total = 0;
    for (int c = 0; c < n; c++) total += counts[c];
    const bool small = (size_t)total * 2 < ((size_t)256 << 20);
    std::vector<int> chunk_begin(1, 0);
    int64_t acc = 0;
    for (int c = 0; c < n; c++) {
        acc += counts[c];
        const bool cut = chunk_units > 0 ? (c + 1 - chunk_begin.back()) >= chunk_units : (!small && acc >= CHUNK_SAMPLES);
        if (cut && c + 1 < n) {
            chunk_begin.push_back(c + 1);
            acc = 0;
        }
    }
    // the last chunk once more, into (5/8, 3/8) of its samples: what runs after the last upload is a short chunk's kernels
    // and download (the equal-length entry points do the same: host_batch.hpp, tail_units)
    if (!small && chunk_units <= 0 && n - chunk_begin.back() >= 2) {
        const int first = chunk_begin.back();
        int64_t rest = 0, head = 0;
        for (int c = first; c < n; c++) rest += counts[c];
        int cut = first;
        while (cut + 1 < n && head + counts[cut] <= rest * 5 / 8) head += counts[cut++];
        if (cut > first && cut < n) chunk_begin.push_back(cut);
    }
    chunk_begin.push_back(n);
    return chunk_begin;
}

// The pipeline works through the rows in order, and what runs after the last upload -- the last chunk's kernels and its
// download -- is the call's tail.  With the caller's (any) order that chunk holds files of every length, and the
// coefficient search of a few hundred channels lasts as long as its LONGEST one (one wave per channel: 31 ms for 120 s):
// the mixed-lengths set of bench.py ended 100 ms after its upload.  The rows are therefore taken longest first (a stable
// sort of pointers; results go back to the caller's rows, coefficients and histories are gathered / scattered by the
// caller): the long files' kernels run under the uploads that follow them and the tail is a chunk of short files.
struct LongestFirst {
    std::vector<int> order;                           // position -> the caller's index
    bool identity = true;
    LongestFirst(const int *counts, int n)
    {
        order.resize(n > 0 ? n : 0);
        for (int i = 0; i < n; i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return counts[a] > counts[b]; });
        for (int i = 0; i < n && identity; i++) identity = order[i] == i;
    }
    template <class T> std::vector<T> gather(const T *v) const
    {
        std::vector<T> out(order.size());
        for (size_t i = 0; i < order.size(); i++) out[i] = v[order[i]];
        return out;
    }
    // rows of `width` elements
    template <class T> std::vector<T> gather_rows(const T *v, int width) const
    {
        std::vector<T> out(order.size() * (size_t)width);
        for (size_t i = 0; i < order.size(); i++) std::copy(v + (size_t)order[i] * width, v + (size_t)(order[i] + 1) * width, out.begin() + i * width);
        return out;
    }
    template <class T> void scatter_rows(const std::vector<T> &v, int width, T *out) const
    {
        for (size_t i = 0; i < order.size(); i++) std::copy(v.begin() + i * width, v.begin() + (i + 1) * width, out + (size_t)order[i] * width);
    }
};

}  // namespace gc
}  // namespace vga
