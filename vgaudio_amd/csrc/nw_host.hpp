// nw_host.hpp -- the host side of the NintendoWare streams (nwstm.hip, nw_files_host.hpp) without HIP: the constants of the
// formats, the version predicates, BxstmConfiguration's rules and the size math of BrstmWriter.cs / BCFstmWriter.cs
// (nw_layout), the PCM readers' check of a parsed info, and the numbers the header kernels write (HeaderGeom).  Header-only
// and free of <hip/hip_runtime.h>, so that a stand-alone host program can include it (tests/host/nw_files_host_driver.cpp);
// whoever includes it supplies vga::set_error.
#pragma once
#include "container_math.hpp"

#include <cstring>

namespace vga {
namespace nw {

using namespace vga::container;

constexpr int kDefaultSamples = 14336;                      // BytesToSamples(0x2000) (BxstmConfiguration.cs:17,48)
constexpr int kOffsetMarker = 0x01000000, kOffsetMarkerV2 = 0x01010000;   // BrstmWriter.cs:76-80
// Structures/ReferenceType.cs
enum : int {
    kByteTable = 0x0100, kReferenceTable = 0x0101, kGcAdpcmInfo = 0x0300, kSampleData = 0x1F00, kStreamInfoBlock = 0x4000,
    kStreamSeekBlock = 0x4001, kStreamDataBlock = 0x4002, kStreamRegionBlock = 0x4003, kStreamPrefetchDataBlock = 0x4004,
    kStreamInfo = 0x4100, kTrackInfo = 0x4101, kChannelInfo = 0x4102
};
constexpr int kCodecPcm8 = 0, kCodecPcm16 = 1, kCodecGcAdpcm = 2;   // NwCodec.cs

// Common.cs:103-140 on a packed NwVersion
inline bool include_track_info(uint32_t v) { const int major = v >> 24; return (major == 0 && v <= 0x00020000u) || (major >= 2 && v <= 0x02010000u); }
inline bool include_region_info(uint32_t v) { const int major = v >> 24; return (major >= 2 && v >= 0x02010000u) || major == 0; }
inline bool include_unaligned_loop(uint32_t v) { const int major = v >> 24; return (major == 0 && v >= 0x00040000u) || (major >= 2 && v >= 0x02030000u); }
inline bool include_checksum(uint32_t v) { return (v >> 24) == 0 && v >= 0x00050000u; }

// the target's byte order and the version fields (BrstmWriter.cs:119, BCFstmWriter.cs:27,57-65,147-162)
inline int target_and_version(const vga_nwstm_params *p, vga_nwstm_layout *L)
{
    L->target = p->target;
    if (p->target == VGA_NW_RSTM) {
        L->endianness = VGA_NW_BIG_ENDIAN;                  // BrstmWriter.cs:119
        L->version = 0x01000000u;
    } else {
        L->endianness = p->endianness < 0 ? (p->target == VGA_NW_CSTM ? VGA_NW_LITTLE_ENDIAN : VGA_NW_BIG_ENDIAN) : (p->endianness != 0);
        uint32_t v = p->version ? p->version : (p->target == VGA_NW_CSTM ? 0x02010000u : 0x00030000u);
        const int major = v >> 24, minor = (v >> 16) & 0xff;
        if ((v & 0xffff) != 0 || (p->target == VGA_NW_CSTM ? (major != 2 || minor > 3) : (major != 0 || minor < 2 || minor > 5))) {
            set_error("version %u.%u.%u is not one this writer produces (BCSTM 2.0-2.3, BFSTM 0.2-0.5)", major, minor, (v >> 8) & 0xff);
            return VGA_ERR_OUT_OF_RANGE;
        }
        L->version = v;
        L->include_track_info = include_track_info(v);
        L->include_region_info = include_region_info(v);
        L->include_unaligned_loop = include_unaligned_loop(v);
        // BCFstmWriter.GetVersion (:147-162): the configured Version only selects which fields exist
        const int word = p->target == VGA_NW_FSTM ? (L->include_unaligned_loop ? 4 : 3)
                         : (L->include_track_info && L->include_region_info) ? 0x201
                         : (!L->include_track_info && L->include_region_info) ? 0x202 : 0x200;
        L->version_word = word << 16;
    }
    return VGA_OK;
}

// BxstmConfiguration.cs:42-100 and the size math of BrstmWriter.cs:22-74 / BCFstmWriter.cs:23-83 for a GC-ADPCM, PCM8 or
// PCM16 stream (L zeroed by the caller).  PCM has no divisible-by-14 rule, no loop alignment, no seek block and no
// channel info body, and no version with unaligned loop points.
inline int nw_layout(const vga_nwstm_params *p, int codec, int nch, vga_nwstm_layout *L)
{
    const bool gc = codec == kCodecGcAdpcm;
    const int bps = codec == kCodecPcm16 ? 2 : 1;           // PCM bytes per sample
    auto bytes = [&](int samples) { return gc ? bytes_of(samples) : samples * bps; };
    if (p->target < VGA_NW_RSTM || p->target > VGA_NW_FSTM) { set_error("unknown NintendoWare target %d", p->target); return VGA_ERR_ARGUMENT; }
    if (nch < 1 || nch > VGA_NW_MAX_CHANNELS) { set_error("channel count %d out of range (1..%d)", nch, VGA_NW_MAX_CHANNELS); return VGA_ERR_ARGUMENT; }
    if (gc && (p->keep_seek_table || p->keep_loop_context)) {
        set_error("only RecalculateSeekTable = RecalculateLoopContext = true is supported: the tables come from the channel builder");
        return VGA_ERR_ARGUMENT;
    }
    const int def = gc ? kDefaultSamples : 0x2000 / bps;    // BytesToSamples(DefaultInterleave, Codec)
    const int spi = p->samples_per_interleave ? p->samples_per_interleave : def;
    if (spi < 1) return out_of_range("Number of samples per interleave must be positive");
    if (gc && spi % 14 != 0) return out_of_range("Number of samples per interleave must be divisible by 14");
    const int spe = p->samples_per_seek_table_entry ? p->samples_per_seek_table_entry : def;
    if (spe < 2) return out_of_range("Number of samples per interleave must be 2 or greater");
    const int align = p->loop_point_alignment ? p->loop_point_alignment : kDefaultSamples;
    if (gc && align < 0) return out_of_range("negative loop point alignment");
    if (p->sample_rate < 0 || p->sample_count < 0) return out_of_range("negative sample rate / sample count");
    if (p->track_type != VGA_NW_TRACK_STANDARD && p->track_type != VGA_NW_TRACK_SHORT) { set_error("unknown BRSTM track type"); return VGA_ERR_ARGUMENT; }
    if (p->seek_table_type != VGA_NW_SEEK_STANDARD && p->seek_table_type != VGA_NW_SEEK_SHORT) { set_error("unknown BRSTM seek table type"); return VGA_ERR_ARGUMENT; }
    if (p->track_count < 0 || p->track_count > VGA_NW_MAX_TRACKS) {
        set_error("track count %d out of range (0 = the default list, at most %d)", p->track_count, VGA_NW_MAX_TRACKS);
        return VGA_ERR_OUT_OF_RANGE;
    }
    if (int rc = check_loop(p->looping, p->loop_start, p->loop_end, p->sample_count)) return rc;
    const int loop_start = p->looping ? p->loop_start : 0, loop_end = p->looping ? p->loop_end : 0;
    if (int rc = target_and_version(p, L)) return rc;
    int shift = 0;
    if (gc) {
        // SetupWriter (BrstmWriter.cs:88-103): WithAlignment when the loop start is not aligned; every channel is then
        // rebuilt with LoopAlignmentMultiple and SamplesPerSeekTableEntry -- vga_gcadpcm_build_channels_* does both
        L->channel.sample_count = p->sample_count;
        L->channel.looping = p->looping ? 1 : 0;
        L->channel.loop_start = loop_start;
        L->channel.loop_end = loop_end;
        L->channel.loop_alignment_multiple = align;
        L->channel.samples_per_seek_table_entry = spe;
        vga_gcadpcm_channel_layout cl;
        if (int rc = gc::channel_layout_for(&L->channel, &cl)) return rc;
        L->alignment_needed = cl.alignment_needed;
        L->channel_sample_count = cl.sample_count_aligned;
        L->channel_adpcm_bytes = bytes_of(cl.sample_count_aligned);
        L->channel_seek_entries = cl.seek_table_entries;
        shift = cl.alignment_needed ? cl.loop_start_aligned - loop_start : 0;          // GcAdpcmFormat.cs:19-22
    } else {
        if (L->include_unaligned_loop) {                    // BCFstmWriter.cs:250-254 reads Adpcm.LoopStart
            set_error("BCSTM 2.3+ / BFSTM 0.4+ carry GC-ADPCM unaligned loop points, which a PCM stream does not have "
                      "(the reference writer fails on a null GcAdpcmFormat): choose an earlier version");
            return VGA_ERR_INVALID_OP;
        }
        const int64_t row = (int64_t)p->sample_count * bps;
        if ((int64_t)spi * bps > 0x7FFFFFFF) return out_of_range("Number of samples per interleave too large for the interleave's int size");
        if (row > 0x7FFFFFFF) { set_error("file would exceed 2 GiB (the reference's FileSize is an int)"); return VGA_ERR_OUT_OF_RANGE; }
        L->channel_sample_count = p->sample_count;
        L->channel_adpcm_bytes = (int)row;
    }
    L->looping = p->looping ? 1 : 0;
    L->loop_start = loop_start + shift;
    L->loop_end = loop_end + shift;
    const int sc = L->looping ? L->loop_end : p->sample_count;                                       // SampleCount (:27)
    L->sample_count = sc;
    L->track_count = p->track_count ? p->track_count : div_round_up(nch, 2);
    const bool rstm = p->target == VGA_NW_RSTM;
    L->samples_per_interleave = spi;
    L->interleave_size = bytes(spi);
    L->interleave_count = div_round_up(sc, spi);
    L->last_block_samples = sc - (L->interleave_count - 1) * spi;
    L->last_block_size_without_padding = bytes(L->last_block_samples);
    L->last_block_size = (int)next_multiple(L->last_block_size_without_padding, 0x20);
    L->samples_per_seek_table_entry = gc || !rstm ? spe : 0;  // a PCM BRSTM writes zeros (BrstmWriter.cs:51-52)
    L->bytes_per_seek_table_entry = gc || !rstm ? 4 : 0;
    if (gc) L->seek_table_entry_count = rstm && p->seek_table_type == VGA_NW_SEEK_SHORT ? bytes_of(sc) / spe + 1 : div_round_up(sc, spe);
    const int64_t audio_data_size = next_multiple(bytes(sc), 0x20);
    const int T = L->track_count;
    L->header_size = 0x40;
    if (rstm) {
        L->head1_size = 0x34;
        L->head2_size = 4 + 8 * T + (p->track_type == VGA_NW_TRACK_SHORT ? 4 : 0x0c) * T;
        L->head3_size = 4 + 8 * nch + (gc ? 0x38 : 8) * nch;                              // ChannelInfoSize
    } else {
        L->head1_size = 0x38 + (L->include_region_info ? 0xc : 0) + (L->include_unaligned_loop ? 8 : 0);
        L->head2_size = L->include_track_info ? 4 + 8 * T : 0;
        L->head3_size = 4 + 8 * nch + (L->include_track_info ? 0x14 * T : 0) + 8 * nch + (gc ? 0x2e : 0) * nch;
    }
    const int64_t head = next_multiple(8 + 24 + L->head1_size + L->head2_size + L->head3_size, 0x20);
    const int64_t seek = gc ? next_multiple(8 + (int64_t)L->seek_table_entry_count * nch * 4, 0x20) : 0;   // PCM: no ADPC / SEEK
    const int64_t data = 0x20 + audio_data_size * nch;
    const int64_t file = 0x40 + head + seek + data;
    if (file > 0x7FFFFFFF) { set_error("file would exceed 2 GiB (the reference's FileSize is an int)"); return VGA_ERR_OUT_OF_RANGE; }
    L->head_block_offset = 0x40;
    L->head_block_size = (int)head;
    L->seek_block_offset = gc ? (int)(0x40 + head) : 0;
    L->seek_block_size = (int)seek;
    L->data_block_offset = (int)(0x40 + head + seek);
    L->data_block_size = (int)data;
    L->audio_data_offset = L->data_block_offset + 0x20;
    L->audio_data_size = (int)audio_data_size;
    L->file_size = (int)file;
    return VGA_OK;
}

// What vga_nwstm_pcm_read_device checks of a parsed info before it looks at a pointer, for that call and for every file of a
// set for reading (nw_pcm_files_host.hpp) alike.  moves: the call has images to read; the geometry is looked at only then, and
// only of a stream that has samples.
inline int pcm_read_info_check(const vga_nwstm_info *I, int sample_kind, bool moves)
{
    if (I->codec != kCodecPcm8 && I->codec != kCodecPcm16) { set_error("info is not a PCM8 / PCM16 stream (vga_nwstm_pcm_parse)"); return VGA_ERR_ARGUMENT; }
    if (int rc = check_sample_kind(sample_kind)) return rc;
    if (I->codec == kCodecPcm16 && sample_kind != VGA_SAMPLES_S16) { set_error("a PCM16 stream is read to VGA_SAMPLES_S16 rows"); return VGA_ERR_ARGUMENT; }
    if (!moves || I->adpcm_bytes == 0) return VGA_OK;
    const int nch = I->channel_count, bps = I->codec == kCodecPcm16 ? 2 : 1;
    if (nch < 1 || I->interleave_size <= 0 || I->audio_data_length < 0 || I->audio_data_length % nch || I->adpcm_bytes != I->sample_count * bps) {
        set_error("info does not describe a stream");
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}

// AudioTrack (Formats/AudioTrack.cs) as the header kernels write it
struct TrackK { int channel_count; uint8_t left, right, volume, panning; };

// everything a header kernel writes of one file that is not per channel and not a track
struct HeaderGeom {
    int target, big, nch, looping, sample_rate, loop_start, loop_end, sample_count;
    int interleave_count, interleave_size, samples_per_interleave, last_block_size_without_padding, last_block_samples;
    int last_block_size, samples_per_seek_table_entry, track_short, track_info, region_info, unaligned_loop, version_word;
    int head_offset, head_size, head1_size, head2_size, seek_offset, seek_size, data_offset, data_size, audio_offset;
    int file_size, track_count;
    int codec, bytes_per_seek_table_entry;                  // NwCodec: GC-ADPCM, or PCM8 / PCM16 (no seek block)
};

inline void header_geom(const vga_nwstm_layout &L, const vga_nwstm_params *p, int nch, int codec, HeaderGeom *a)
{
    std::memset(a, 0, sizeof *a);
    a->target = L.target; a->big = L.endianness; a->nch = nch; a->looping = L.looping; a->sample_rate = p->sample_rate;
    a->loop_start = L.loop_start; a->loop_end = L.loop_end; a->sample_count = L.sample_count;
    a->interleave_count = L.interleave_count; a->interleave_size = L.interleave_size;
    a->samples_per_interleave = L.samples_per_interleave; a->last_block_size_without_padding = L.last_block_size_without_padding;
    a->last_block_samples = L.last_block_samples; a->last_block_size = L.last_block_size;
    a->samples_per_seek_table_entry = L.samples_per_seek_table_entry; a->track_short = p->track_type == VGA_NW_TRACK_SHORT;
    a->track_info = L.include_track_info; a->region_info = L.include_region_info; a->unaligned_loop = L.include_unaligned_loop;
    a->version_word = L.version_word; a->head_offset = L.head_block_offset; a->head_size = L.head_block_size;
    a->head1_size = L.head1_size; a->head2_size = L.head2_size; a->seek_offset = L.seek_block_offset;
    a->seek_size = L.seek_block_size; a->data_offset = L.data_block_offset; a->data_size = L.data_block_size;
    a->audio_offset = L.audio_data_offset; a->file_size = L.file_size; a->track_count = L.track_count;
    a->codec = codec; a->bytes_per_seek_table_entry = L.bytes_per_seek_table_entry;
}

}  // namespace nw
}  // namespace vga
