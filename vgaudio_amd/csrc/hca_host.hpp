// hca_host.hpp -- the host side of CRI HCA without HIP: CriHcaEncoder.Initialize and HcaInfo (stream parameters), channel
// typing, the ATH curve, the kernels' DeviceInfo, shape classes, the status word and the counters of the encoder's
// streaming shell.  Header-only and free of <hip/hip_runtime.h>, so that a stand-alone host program can include it
// (tests/host/hca_host_driver.cpp) as the C-ABI files do (hca_capi.hpp); whoever includes it supplies vga::set_error.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/vgaudio_hip.h"
#include "hca_info.hpp"

namespace vga {

void set_error(const char *fmt, ...);               // (common.hpp)

namespace hca {

namespace hosttab {
#include "hca_tables_host.inc"
}

inline int divide_by_round_up(int v, int d) { return (int)std::ceil((double)v / d); }        // Extensions.cs:145
inline int get_next_multiple(int value, int multiple)                                        // Helpers.cs:71-80
{
    if (multiple <= 0) return value;
    if (value % multiple == 0) return value;
    return value + multiple - value % multiple;
}

// CriHcaEncoder.cs:288-324
inline int calculate_bitrate(const vga_hca_info &h, int quality, int bitrate, int limit_bitrate)
{
    const int pcm_bitrate = h.sample_rate * h.channel_count * 16;
    const int max_bitrate = pcm_bitrate / 4;
    int min_bitrate = 0;
    int ratio = 6;
    switch (quality) {
    case 1: ratio = 4; break;
    case 2: ratio = 6; break;
    case 3: ratio = 8; break;
    case 4: ratio = h.channel_count == 1 ? 10 : 12; break;
    case 5: ratio = h.channel_count == 1 ? 12 : 16; break;
    default: break;
    }
    bitrate = bitrate != 0 ? bitrate : pcm_bitrate / ratio;
    if (limit_bitrate) min_bitrate = std::min(h.channel_count == 1 ? 42666 : 32000 * h.channel_count, pcm_bitrate / 6);
    return bitrate < min_bitrate ? min_bitrate : (bitrate > max_bitrate ? max_bitrate : bitrate);
}

// CriHcaEncoder.cs:326-368
inline void calculate_band_counts(vga_hca_info &h, int bitrate, int cutoff_freq)
{
    h.frame_size = bitrate * 1024 / h.sample_rate / 8;
    int num_groups = 0;
    const int pcm_bitrate = h.sample_rate * h.channel_count * 16;
    int hfr_ratio, cutoff_ratio;
    if (h.channel_count <= 1 || pcm_bitrate / bitrate <= 6) { hfr_ratio = 6; cutoff_ratio = 12; }
    else { hfr_ratio = 8; cutoff_ratio = 16; }
    if (bitrate < pcm_bitrate / cutoff_ratio)
        cutoff_freq = std::min(cutoff_freq, cutoff_ratio * bitrate / (32 * h.channel_count));
    const int total_band_count = (int)std::nearbyint(cutoff_freq * 256.0 / h.sample_rate);        // Math.Round
    const int hfr_start_band = (int)std::min((double)total_band_count,
                                             std::nearbyint((hfr_ratio * bitrate * 128.0) / pcm_bitrate));
    const int stereo_start_band = hfr_ratio == 6 ? hfr_start_band : (hfr_start_band + 1) / 2;
    const int hfr_band_count = total_band_count - hfr_start_band;
    const int bands_per_group = divide_by_round_up(hfr_band_count, 8);
    if (bands_per_group > 0) num_groups = divide_by_round_up(hfr_band_count, bands_per_group);
    h.total_band_count = total_band_count;
    h.base_band_count = stereo_start_band;
    h.stereo_band_count = hfr_start_band - stereo_start_band;
    h.hfr_group_count = num_groups;
    h.bands_per_hfr_group = bands_per_group;
}

// CriHcaFrame.cs:33-52
inline void channel_types(const vga_hca_info &h, int types[8])
{
    for (int i = 0; i < 8; i++) types[i] = CH_DISCRETE;
    const int cpt = h.channel_count / (h.track_count > 0 ? h.track_count : 1);
    if (h.stereo_band_count == 0 || cpt == 1) return;
    const int P = CH_STEREO_PRIMARY, S = CH_STEREO_SECONDARY, D = CH_DISCRETE;
    const int t2[] = {P, S}, t3[] = {P, S, D}, t4a[] = {P, S, D, D}, t4b[] = {P, S, P, S}, t5a[] = {P, S, D, D, D},
              t5b[] = {P, S, D, P, S}, t6[] = {P, S, D, D, P, S}, t7[] = {P, S, D, D, P, S, D},
              t8[] = {P, S, D, D, P, S, P, S};
    const int *src = nullptr;
    switch (cpt) {
    case 2: src = t2; break;
    case 3: src = t3; break;
    case 4: src = h.channel_config != 0 ? t4a : t4b; break;
    case 5: src = h.channel_config > 2 ? t5a : t5b; break;
    case 6: src = t6; break;
    case 7: src = t7; break;
    case 8: src = t8; break;
    default: break;
    }
    if (src) for (int i = 0; i < cpt; i++) types[i] = src[i];
}

// CriHcaEncoder.Initialize (CriHcaEncoder.cs:61-114)
inline int encoder_initialize(const vga_hca_params *c, vga_hca_info *h)
{
    if (!c || !h) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    memset(h, 0, sizeof *h);
    if (c->channel_count > 8 || c->channel_count < 1) {
        set_error("HCA channel count must be 8 or below");
        return VGA_ERR_OUT_OF_RANGE;
    }
    if (c->sample_rate <= 0 || c->sample_count < 0) { set_error("bad sample rate / count"); return VGA_ERR_ARGUMENT; }
    const int cutoff = c->sample_rate / 2;
    h->channel_count = c->channel_count;
    h->track_count = 1;
    h->sample_count = c->sample_count;
    h->sample_rate = c->sample_rate;
    h->min_resolution = 1;
    h->max_resolution = 15;
    h->inserted_samples = SPSF;
    const int bitrate = calculate_bitrate(*h, c->quality, c->bitrate, c->limit_bitrate);
    if (bitrate <= 0) { set_error("bitrate resolves to %d", bitrate); return VGA_ERR_OUT_OF_RANGE; }
    calculate_band_counts(*h, bitrate, cutoff);
    if (h->bands_per_hfr_group > 0) {                           // HcaInfo.CalculateHfrValues :52-58
        h->hfr_band_count = h->total_band_count - h->base_band_count - h->stereo_band_count;
        h->hfr_group_count = divide_by_round_up(h->hfr_band_count, h->bands_per_hfr_group);
    }
    {                                                           // SetChannelConfiguration :370-381
        const int cpt = h->channel_count / h->track_count;
        const int cfg = hosttab::HCA_DefaultChannelMapping[cpt];
        if (hosttab::HCA_ValidChannelMappings[cpt - 1][cfg] != 1) {
            set_error("Channel mapping is not valid.");
            return VGA_ERR_OUT_OF_RANGE;
        }
        h->channel_config = cfg;
    }
    int input_sample_count = h->sample_count;
    if (c->looping) {
        h->looping = 1;
        h->sample_count = std::min(c->loop_end, c->sample_count);
        h->inserted_samples += get_next_multiple(c->loop_start, SPF) - c->loop_start;
        {                                                       // CalculateLoopInfo :383-398
            const int ls = c->loop_start + h->inserted_samples, le = c->loop_end + h->inserted_samples;
            h->loop_start_frame = ls / SPF;
            h->pre_loop_samples = ls % SPF;
            h->loop_end_frame = le / SPF;
            h->post_loop_samples = SPF - le % SPF;
            if (h->post_loop_samples == SPF) { h->loop_end_frame--; h->post_loop_samples = 0; }
        }
        input_sample_count = std::min(get_next_multiple(h->sample_count, SPSF), c->sample_count);
        input_sample_count += SPSF * 2;
    }
    {                                                           // CalculateHeaderSize :400-418
        h->header_size = get_next_multiple(96 + h->comment_length, 32);
        if (h->looping) {
            if (h->frame_size <= 0) {
                // the reference divides by FrameSize here (CriHcaEncoder.cs:411: a catchable DivideByZeroException);
                // the non-looping path reports the same condition from the encoder ("Bitrate is set too low.")
                set_error("Bitrate is set too low.");
                return VGA_ERR_INVALID_DATA;
            }
            const int off = h->header_size + h->frame_size * h->loop_start_frame;
            const int padding_bytes = get_next_multiple(off, 2048) - off;
            const int padding_frames = padding_bytes / h->frame_size;
            h->inserted_samples += padding_frames * SPF;
            h->loop_start_frame += padding_frames;
            h->loop_end_frame += padding_frames;
            h->header_size += padding_bytes % h->frame_size;
        }
    }
    const int total_samples = input_sample_count + h->inserted_samples;
    h->frame_count = divide_by_round_up(total_samples, SPF);
    h->appended_samples = h->frame_count * SPF - h->inserted_samples - input_sample_count;
    return VGA_OK;
}

// A negative StereoBandCount (a dec chunk whose base band count exceeds the total, HcaReader.cs:179-186) and a negative
// HfrGroupCount (comp bands beyond the total, HcaInfo.CalculateHfrValues) decode in the reference: ApplyIntensityStereo
// and the HFR scales need counts above 0 (CriHcaDecoder.cs:119, :149; CriHcaPacking.cs:101), as the kernels do.  What
// it indexes past its arrays for is VGA_ERR_OUT_OF_RANGE (IndexOutOfRangeException), refused before any frame.
inline int make_device_info(const vga_hca_info &h, DeviceInfo &d)
{
    if (h.channel_count < 1 || h.channel_count > 8 || h.frame_size < 8 || h.frame_size > 0xFFFF || h.frame_count < 0 ||
        h.total_band_count < 0 || h.total_band_count > 128 || h.base_band_count < 0 || h.hfr_group_count > 8 ||
        (h.hfr_group_count > 0 && h.bands_per_hfr_group <= 0)) {
        set_error("HcaInfo is inconsistent (channels %d, frame size %d, bands %d/%d/%d, hfr groups %d)", h.channel_count,
                  h.frame_size, h.total_band_count, h.base_band_count, h.stereo_band_count, h.hfr_group_count);
        return VGA_ERR_ARGUMENT;
    }
    // GetChannelTypes returns channelsPerTrack entries and new CriHcaFrame indexes them for every channel
    // (CriHcaFrame.cs:20-29, :36-51): with stereo bands and more than one track it throws before the first frame
    const int cpt = h.channel_count / (h.track_count > 0 ? h.track_count : 1);
    if (h.stereo_band_count != 0 && cpt != 1 && cpt < h.channel_count) {
        set_error("Index was outside the bounds of the array (%d channels, %d per track, stereo bands %d)", h.channel_count, cpt,
                  h.stereo_band_count);
        return VGA_ERR_OUT_OF_RANGE;
    }
    memset(&d, 0, sizeof d);
    d.nch = h.channel_count;
    d.frame_size = h.frame_size;
    d.frame_count = h.frame_count;
    d.sample_count = h.sample_count;
    d.inserted_samples = h.inserted_samples;
    d.total_band_count = h.total_band_count;
    d.base_band_count = h.base_band_count;
    d.stereo_band_count = h.stereo_band_count;
    d.hfr_band_count = h.hfr_band_count;
    d.bands_per_hfr_group = h.bands_per_hfr_group;
    d.hfr_group_count = h.hfr_group_count;
    int types[8];
    channel_types(h, types);
    for (int i = 0; i < 8; i++) {
        d.channel_type[i] = types[i];
        d.coded_count[i] = types[i] == CH_STEREO_SECONDARY ? h.base_band_count : h.base_band_count + h.stereo_band_count;
        if (i >= h.channel_count) continue;
        if (d.coded_count[i] < 0) {
            set_error("HcaInfo is inconsistent (channel %d codes %d bands)", i, d.coded_count[i]);
            return VGA_ERR_ARGUMENT;
        }
        if (d.coded_count[i] > 128) {                           // ScaleFactors / Resolution[i] (CriHcaPacking.cs:89-95, :120-122)
            set_error("Index was outside the bounds of the array (channel %d codes %d bands)", i, d.coded_count[i]);
            return VGA_ERR_OUT_OF_RANGE;
        }
    }
    if (h.use_ath_curve) {                                     // CriHcaFrame.ScaleAthCurve :60-83
        int acc = 0, i;
        for (i = 0; i < 128; i++) {
            acc += h.sample_rate;
            const int index = acc >> 13;
            if (index >= 654) break;
            d.ath_curve[i] = hosttab::HCA_AthCurve[index];
        }
        for (; i < 128; i++) d.ath_curve[i] = 0xff;
    }
    return VGA_OK;
}

// fewer bits than sync + noise level + checksum + one 3-bit channel header each: the reference's CalculateNoiseLevel
// necessarily ends in InvalidDataException "Bitrate is set too low." (CriHcaEncoder.cs:469-472).  A channel count outside
// 1..8 is not this rule's to refuse: make_device_info does (VGA_ERR_ARGUMENT).
inline bool bitrate_too_low(const vga_hca_info &h)
{
    return h.channel_count >= 1 && h.channel_count <= 8 && h.frame_size * 8 < 48 + 3 * h.channel_count + 16;
}

// bytes from one stream's frames to the next in the host entry points' device buffers: 8 bytes of slack for the decoder
inline int64_t frames_pitch_for(const vga_hca_info &h)
{
    return ((int64_t)h.frame_count * h.frame_size + 8 + 15) / 16 * 16;
}

// Nothing in the decoder but three numbers depends on a stream's length, and the kernels can take those per stream from a
// table: a SHAPE CLASS is what make_device_info() builds with those three fields ignored
inline DeviceInfo shape_class_of(DeviceInfo d)
{
    d.frame_count = d.sample_count = d.inserted_samples = 0;
    return d;
}

// cls[s]: the shape class of stream s, dense ids in order of first appearance (one hash lookup per stream); returns the count
inline int decode_classes(const DeviceInfo *dev, int n, std::vector<int> &cls)
{
    std::unordered_map<std::string, int> ids;
    cls.resize(n);
    for (int s = 0; s < n; s++) {
        const DeviceInfo d = shape_class_of(dev[s]);                    // (memset by make_device_info: no stray bytes)
        cls[s] = ids.emplace(std::string(reinterpret_cast<const char *>(&d), sizeof d), (int)ids.size()).first->second;
    }
    return (int)ids.size();
}

// the kernels' status word (include/vgaudio_hip.h, vga_hca_encode_device) as the call's error
inline int status_to_error(int status)
{
    if (status & 16) { set_error("internal: the encoder's bit-cost table could not be built"); return VGA_ERR_DEVICE; }   // (hca_encode_kernel.hip: cost_lut_build)
    if (status & 4) { set_error("Bitrate is set too low."); return VGA_ERR_INVALID_DATA; }     // CriHcaEncoder.cs:471
    if (status & 8) { set_error("evaluation boundary search failed (NotImplementedException in the reference)"); return VGA_ERR_INVALID_OP; }
    if (status & 1) { set_error("Invalid frame header"); return VGA_ERR_INVALID_DATA; }        // CriHcaPacking.cs:76
    // (hca_decode_core.hpp scan_frame) a frame whose secondary channel carries intensity 15: IntensityRatioTable has 15
    // entries (CriHcaDecoder.cs:157).  A batch that also holds a bad sync word reports that, whichever frame comes first.
    if (status & 32) { set_error("Index was outside the bounds of the array (intensity 15)"); return VGA_ERR_OUT_OF_RANGE; }
    if (status & 2) { set_error("scale-factor delta out of range (frame state would be stale in the reference)"); return VGA_ERR_INVALID_DATA; }
    return VGA_OK;
}

// The counters of CriHcaEncoder's streaming shell (Initialize :61-114, Encode :126-269): BufferPreSamples, BufferPosition,
// SamplesProcessed, FramesProcessed and PostSamples.  A plain value: the shell (capi_hca_stream.hip) saves it before a call
// and assigns it back when the frames the walk promises cannot be delivered.
struct StreamCounters {
    int buffer_pre = 0, buffer_pos = 0, samples_processed = 0, frames_processed = 0, post_samples = 0;

    // one Encode() call with a block of 1024 samples: the number of frames it completes -- none while the buffer fills,
    // several when the pre-audio of a looping stream or the post-audio at the end flush whole frames
    int advance_one_block(const vga_hca_info &h)
    {
        const int first = frames_processed;
        auto flush = [&]() {                                                            // OutputFrame :256-269
            if (buffer_pos != SPF) return;
            buffer_pos = 0;
            frames_processed++;
        };
        int pcm_pos = 0;
        if (buffer_pre > 0) {                                                           // EncodePreAudio :163-183
            while (buffer_pre > SPF) {
                buffer_pos = SPF;
                flush();
                buffer_pre -= SPF;
            }
            buffer_pos = buffer_pre;
            buffer_pre = 0;
        }
        while (SPF - pcm_pos > 0 && h.sample_count > samples_processed) {               // EncodeMainAudio :185-200
            int n = std::min(SPF - buffer_pos, SPF - pcm_pos);
            n = std::min(n, h.sample_count - samples_processed);
            buffer_pos += n;
            samples_processed += n;
            pcm_pos += n;
            flush();
        }
        if (h.sample_count == samples_processed) {                                      // EncodePostAudio :202-242
            int post_pos = 0;
            while (post_pos < post_samples) {
                const int n = std::min(SPF - buffer_pos, post_samples - post_pos);
                buffer_pos += n;
                post_pos += n;
                flush();
            }
            while (frames_processed < h.frame_count) {
                buffer_pos = SPF;
                flush();
            }
        }
        return frames_processed - first;
    }
};

// the counters before the first block (Initialize :70, :99, :113)
inline StreamCounters stream_counters_for(const vga_hca_info &h)
{
    StreamCounters c;
    const int input_samples = h.frame_count * SPF - h.inserted_samples - h.appended_samples;
    c.post_samples = h.looping ? input_samples - h.sample_count : SPSF;
    c.buffer_pre = h.inserted_samples - SPSF;
    return c;
}

// Encode :128-131: "All audio frames have already been output by the encoder"
inline bool stream_finished(const StreamCounters &c, const vga_hca_info &h) { return c.frames_processed >= h.frame_count; }

}  // namespace hca
}  // namespace vga
