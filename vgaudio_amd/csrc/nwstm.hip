// nwstm.hip -- NintendoWare streams for GC-ADPCM: BRSTM (Containers/NintendoWare/BrstmWriter.cs, BrstmReader.cs) and
// BCSTM / BFSTM (BCFstmWriter.cs, BCFstmReader.cs).  Size math and parsing are host code; the images are assembled
// and taken apart in HBM, nfiles equally shaped files per launch.  Everything on the device is byte movement:
// HBM-bound, every byte of an image read or written once.
#include "container_host.hpp"
#include "pcm_kernels.hpp"

using namespace vga;
using namespace vga::container;

namespace {

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
bool include_track_info(uint32_t v) { const int major = v >> 24; return (major == 0 && v <= 0x00020000u) || (major >= 2 && v <= 0x02010000u); }
bool include_region_info(uint32_t v) { const int major = v >> 24; return (major >= 2 && v >= 0x02010000u) || major == 0; }
bool include_unaligned_loop(uint32_t v) { const int major = v >> 24; return (major == 0 && v >= 0x00040000u) || (major >= 2 && v >= 0x02030000u); }
bool include_checksum(uint32_t v) { return (v >> 24) == 0 && v >= 0x00050000u; }

}  // namespace

// ---------------------------------------------------------------- device side
namespace vga {
namespace nwstm {

struct TrackK { int channel_count; uint8_t left, right, volume, panning; };

// everything the header kernel writes that is not per channel; passed by value (< 4 KiB of kernel arguments)
struct HeaderArgs {
    int target, big, nch, looping, sample_rate, loop_start, loop_end, sample_count;
    int interleave_count, interleave_size, samples_per_interleave, last_block_size_without_padding, last_block_samples;
    int last_block_size, samples_per_seek_table_entry, track_short, track_info, region_info, unaligned_loop, version_word;
    int head_offset, head_size, head1_size, head2_size, seek_offset, seek_size, data_offset, data_size, audio_offset;
    int file_size, track_count;
    int codec, bytes_per_seek_table_entry;                  // NwCodec: GC-ADPCM, or PCM8 / PCM16 (no seek block)
    TrackK tracks[VGA_NW_MAX_TRACKS];
};

// A positioned, endian-aware writer over one image, as the reference's BinaryWriter over MemoryStream(byte[FileSize])
// (Utilities/BinaryWriterBE.cs for big-endian files).
struct Cursor {
    uint8_t *buf;
    int pos;
    bool big;
    __device__ void put8(int v) { buf[pos++] = (uint8_t)v; }
    __device__ void put16(int v) { if (big) { put8(v >> 8); put8(v); } else { put8(v); put8(v >> 8); } }
    __device__ void put32(int v) { if (big) { put16(v >> 16); put16(v); } else { put16(v); put16(v >> 16); } }
    __device__ void tag(const char *t) { for (int k = 0; k < 4; k++) put8(t[k]); }   // WriteUTF8: bytes as they are
};

// One workgroup per image: the threads zero everything in front of the seek block (of the DATA block for PCM, which
// has none) and between the DATA header and the audio, then lane 0 writes the file header and HEAD
// (BrstmWriter.cs:130-260) or INFO (BCFstmWriter.cs:171-333).  PCM streams take the writers' Codec != GcAdpcm branches.
__global__ __launch_bounds__(64) void nw_header_kernel(HeaderArgs a, const uint8_t *__restrict__ adpcm, int64_t adpcm_pitch,
                                                       int adpcm_len, const int16_t *__restrict__ coefs,
                                                       const int16_t *__restrict__ gain, const int16_t *__restrict__ start_ctx,
                                                       const int16_t *__restrict__ loop_ctx, uint8_t *__restrict__ files,
                                                       int64_t file_pitch)
{
    uint8_t *img = files + (int64_t)blockIdx.x * file_pitch;
    const bool gc = a.codec == kCodecGcAdpcm;
    for (int k = threadIdx.x, end = gc ? a.seek_offset : a.data_offset; k < end; k += 64) img[k] = 0;
    for (int k = a.data_offset + threadIdx.x; k < a.audio_offset; k += 64) img[k] = 0;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int nch = a.nch, row0 = blockIdx.x * nch;
    // GcAdpcmChannel.StartContext: (Adpcm[0], 0, 0) for a fresh channel (GcAdpcmChannel.cs:45)
    auto ctx = [&](Cursor &c, int ch, bool loop) {
        const int r = row0 + ch;
        // the loop context written for a file that does not loop is the start context (BrstmWriter.cs:250, BCFstmWriter.cs:325)
        if (loop && a.looping) {
            for (int k = 0; k < 3; k++) c.put16(loop_ctx ? loop_ctx[r * 3 + k] : 0);
        } else if (start_ctx) {
            for (int k = 0; k < 3; k++) c.put16(start_ctx[r * 3 + k]);
        } else {
            c.put16(adpcm_len > 0 ? adpcm[(int64_t)r * adpcm_pitch] : 0);
            c.put16(0);
            c.put16(0);
        }
    };
    auto coef = [&](Cursor &c, int ch) { for (int k = 0; k < 16; k++) c.put16(coefs[(row0 + ch) * 16 + k]); };
    Cursor c{img, 0, a.big != 0};
    const int T = a.track_count;
    if (a.target == VGA_NW_RSTM) {
        c.tag("RSTM");                                      // WriteRstmHeader (:130-145)
        c.put16(0xfeff);
        c.put16(0x0100);
        c.put32(a.file_size);
        c.put16(0x40);
        c.put16(2);
        c.put32(a.head_offset); c.put32(a.head_size);
        c.put32(a.seek_offset); c.put32(a.seek_size);
        c.put32(a.data_offset); c.put32(a.data_size);
        c.pos = a.head_offset;                              // WriteHeadBlock (:147-162)
        c.tag("HEAD");
        c.put32(a.head_size);
        c.put32(kOffsetMarker); c.put32(24);
        c.put32(kOffsetMarker); c.put32(24 + a.head1_size);
        c.put32(kOffsetMarker); c.put32(24 + a.head1_size + a.head2_size);
        c.put8(a.codec);                                    // WriteHeadBlock1 (:164-183)
        c.put8(a.looping);
        c.put8(nch);                                        // (byte)ChannelCount
        c.put8(0);
        c.put16(a.sample_rate);                             // (ushort)SampleRate
        c.put16(0);
        c.put32(a.loop_start);
        c.put32(a.sample_count);
        c.put32(a.audio_offset);
        c.put32(a.interleave_count);
        c.put32(a.interleave_size);
        c.put32(a.samples_per_interleave);
        c.put32(a.last_block_size_without_padding);
        c.put32(a.last_block_samples);
        c.put32(a.last_block_size);
        c.put32(a.samples_per_seek_table_entry);
        c.put32(a.bytes_per_seek_table_entry);
        const int tinfo = a.track_short ? 4 : 0x0c;         // WriteHeadBlock2 (:185-216)
        c.put8(T);
        c.put8(a.track_short ? 0 : 1);
        c.put16(0);
        int base = 24 + 0x34 + 4;
        for (int i = 0; i < T; i++) { c.put32(a.track_short ? kOffsetMarker : kOffsetMarkerV2); c.put32(base + T * 8 + tinfo * i); }
        for (int i = 0; i < T; i++) {
            const TrackK &t = a.tracks[i];
            if (!a.track_short) { c.put8(t.volume); c.put8(t.panning); c.put16(0); c.put32(0); }
            c.put8(t.channel_count);
            c.put8(t.left);
            c.put8(t.right);
            c.put8(0);
        }
        c.put8(nch);                                        // WriteHeadBlock3 (:218-256)
        c.put8(0);
        c.put16(0);
        base = 24 + 0x34 + a.head2_size + 4;
        const int cinfo = gc ? 0x38 : 8;                    // ChannelInfoSize
        for (int i = 0; i < nch; i++) { c.put32(kOffsetMarker); c.put32(base + nch * 8 + cinfo * i); }
        for (int i = 0; i < nch; i++) {
            c.put32(kOffsetMarker);
            if (!gc) { c.put32(0); continue; }
            c.put32(base + nch * 8 + 0x38 * i + 8);
            coef(c, i);
            c.put16(gain ? gain[row0 + i] : 0);
            ctx(c, i, false);
            ctx(c, i, true);
            c.put16(0);
        }
        if (gc) {
            c.pos = a.seek_offset;                          // WriteAdpcBlock (:258-267)
            c.tag("ADPC");
            c.put32(a.seek_size);
        }
        c.pos = a.data_offset;                              // WriteDataBlock (:270-274)
        c.tag("DATA");
        c.put32(a.data_size);
        c.put32(0x18);
        return;
    }
    c.tag(a.target == VGA_NW_CSTM ? "CSTM" : "FSTM");       // WriteHeader (:171-197)
    c.put16(0xfeff);
    c.put16(0x40);
    c.put32(a.version_word);
    c.put32(a.file_size);
    c.put16(gc ? 3 : 2);
    c.put16(0);
    c.put16(kStreamInfoBlock); c.put16(0); c.put32(a.head_offset); c.put32(a.head_size);
    if (gc) { c.put16(kStreamSeekBlock); c.put16(0); c.put32(a.seek_offset); c.put32(a.seek_size); }
    c.put16(kStreamDataBlock); c.put16(0); c.put32(a.data_offset); c.put32(a.data_size);
    c.pos = a.head_offset;                                  // WriteInfoBlock (:199-223)
    c.tag("INFO");
    c.put32(a.head_size);
    c.put16(kStreamInfo); c.put16(0); c.put32(24);
    if (a.track_info) { c.put16(kReferenceTable); c.put16(0); c.put32(24 + a.head1_size); }
    else { c.put32(0); c.put32(-1); }
    c.put16(kReferenceTable); c.put16(0); c.put32(24 + a.head1_size + a.head2_size);
    c.put8(a.codec);                                        // WriteInfoBlock1 (:225-258)
    c.put8(a.looping);
    c.put8(nch);
    c.put8(0);
    c.put32(a.sample_rate);
    c.put32(a.loop_start);
    c.put32(a.sample_count);
    c.put32(a.interleave_count);
    c.put32(a.interleave_size);
    c.put32(a.samples_per_interleave);
    c.put32(a.last_block_size_without_padding);
    c.put32(a.last_block_samples);
    c.put32(a.last_block_size);
    c.put32(a.bytes_per_seek_table_entry);
    c.put32(a.samples_per_seek_table_entry);
    c.put16(kSampleData); c.put16(0); c.put32(0x18);
    if (a.region_info) { c.put16(kByteTable); c.put16(0); c.put32(0); c.put32(-1); }
    if (a.unaligned_loop) { c.put32(a.loop_start); c.put32(a.loop_end); }   // Adpcm.LoopStart / LoopEnd
    if (a.track_info) {                                     // WriteInfoBlock2 (:260-275)
        c.put32(T);
        for (int i = 0; i < T; i++) { c.put16(kTrackInfo); c.put16(0); c.put32(4 + 8 * T + 4 + 8 * nch + 0x14 * i); }
    }
    const int tts = a.track_info ? 0x14 * T : 0;            // WriteInfoBlock3 (:277-333)
    c.put32(nch);
    for (int i = 0; i < nch; i++) { c.put16(kChannelInfo); c.put16(0); c.put32(4 + 8 * nch + tts + 8 * i); }
    if (a.track_info)
        for (int i = 0; i < T; i++) {
            const TrackK &t = a.tracks[i];
            c.put8(t.volume); c.put8(t.panning); c.put16(0);
            c.put16(kByteTable); c.put16(0); c.put32(0xc);
            c.put32(t.channel_count);
            c.put8(t.left); c.put8(t.right); c.put16(0);
        }
    for (int i = 0; i < nch; i++) {
        if (gc) { c.put16(kGcAdpcmInfo); c.put16(0); c.put32(8 * nch - 8 * i + 0x2e * i); }
        else { c.put32(0); c.put32(-1); }                   // a null reference: PCM has no channel info body
    }
    if (gc) {
        for (int i = 0; i < nch; i++) {
            coef(c, i);
            ctx(c, i, false);
            ctx(c, i, true);
            c.put16(0);
        }
        c.pos = a.seek_offset;                              // WriteSeekBlock (:335-344)
        c.tag("SEEK");
        c.put32(a.seek_size);
    }
    c.pos = a.data_offset;                                  // WriteDataBlock (:346-352): bytes 8..0x20 stay zero
    c.tag("DATA");
    c.put32(a.data_size);
}

// GcAdpcmFormat.BuildSeekTable (GcAdpcmFormat.cs:100-113): the channels' tables interleaved by 2 shorts, resized to
// `entries` (zero fill / truncation), then written in one byte order -- big-endian in BRSTM (BrstmWriter.cs:267),
// little-endian in BCSTM and ALSO in a big-endian BFSTM (BCFstmWriter.cs:340).  One thread per short of the block
// body; the block's padding is written as zeros here.
__global__ __launch_bounds__(256) void nw_seek_kernel(const int16_t *__restrict__ seek, int64_t seek_pitch, int src_entries,
                                                      int nch, int entries, int big, int seek_offset, int seek_size,
                                                      uint8_t *__restrict__ files, int64_t file_pitch)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int body_shorts = (seek_size - 8) / 2;
    if (k >= body_shorts) return;
    const int f = blockIdx.y;
    int v = 0;
    if (k < entries * nch * 2) {
        const int e = k / (2 * nch), r = k - e * 2 * nch, ch = r >> 1, j = r & 1;
        if (e < src_entries) v = seek[(int64_t)(f * nch + ch) * seek_pitch + 2 * e + j];
    }
    uint8_t *d = files + (int64_t)f * file_pitch + seek_offset + 8 + 2 * k;
    d[0] = (uint8_t)(big ? v >> 8 : v);
    d[1] = (uint8_t)(big ? v : v >> 8);
}

using container::kMaxGridY;

}  // namespace nwstm
}  // namespace vga

// ---------------------------------------------------------------- host side
namespace {

// the layout has checked the track count
int check_track_list(const vga_nwstm_params *p, const vga_nw_track *tracks)
{
    if (p->track_count > 0 && !tracks) { set_error("track_count %d with a null track list", p->track_count); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

// AudioTrack.GetDefaultTrackList (Formats/AudioTrack.cs:69-82), or the caller's list
void fill_tracks(const vga_nwstm_layout &L, const vga_nw_track *tracks, nwstm::HeaderArgs *a)
{
    for (int i = 0; i < L.track_count; i++) {
        nwstm::TrackK &t = a->tracks[i];
        if (tracks) {
            t = {tracks[i].channel_count, (uint8_t)tracks[i].left, (uint8_t)tracks[i].right, (uint8_t)tracks[i].volume,
                 (uint8_t)tracks[i].panning};
        } else {
            const int cc = std::min(a->nch - i * 2, 2);
            t = {cc, (uint8_t)(i * 2), (uint8_t)(cc >= 2 ? i * 2 + 1 : 0), 0x7f, 0x40};
        }
    }
}

void header_args(const vga_nwstm_layout &L, const vga_nwstm_params *p, int nch, const vga_nw_track *tracks, nwstm::HeaderArgs *a,
                 int codec = kCodecGcAdpcm)
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
    fill_tracks(L, tracks, a);
}

struct Ref { int type, offset, base; int abs() const { return base + offset; } bool is(int t) const { return type == t && offset > 0; } };
Ref read_ref(ByteReader &r, int base) { Ref x; x.type = r.i16(); r.pos += 2; x.offset = r.i32(); x.base = base; return x; }

int pcm_codec_check(int codec)
{
    if (codec == kCodecPcm8 || codec == kCodecPcm16) return VGA_OK;
    if (codec == kCodecGcAdpcm) set_error("the stream is GC-ADPCM (codec 2): read it with vga_nwstm_parse");
    else set_error("stream codec %d is neither PCM8 (0) nor PCM16 (1)", codec);
    return VGA_ERR_INVALID_OP;
}

// the target's byte order and the version fields (BrstmWriter.cs:119, BCFstmWriter.cs:27,57-65,147-162)
int target_and_version(const vga_nwstm_params *p, vga_nwstm_layout *L)
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
int nw_layout(const vga_nwstm_params *p, int codec, int nch, vga_nwstm_layout *L)
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
        if (int rc = vga_gcadpcm_channel_layout_for(&L->channel, &cl)) return rc;
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

}  // namespace

extern "C" {

int vga_nwstm_layout_for(const vga_nwstm_params *p, int nch, vga_nwstm_layout *L)
{
    if (!p || !L) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    std::memset(L, 0, sizeof *L);
    return nw_layout(p, kCodecGcAdpcm, nch, L);
}

int vga_nwstm_write_device(const vga_nwstm_params *p, int nch, int nfiles, const vga_nw_track *tracks, const uint8_t *d_adpcm,
                           int64_t adpcm_pitch, int adpcm_len, const int16_t *d_coefs, const int16_t *d_gain,
                           const int16_t *d_start_context, const int16_t *d_loop_context, const int16_t *d_seek,
                           int64_t seek_pitch, int seek_entries, uint8_t *d_files, int64_t file_pitch, void *stream)
{
    vga_nwstm_layout L;
    if (int rc = vga_nwstm_layout_for(p, nch, &L)) return rc;
    if (int rc = check_track_list(p, tracks)) return rc;
    if (nfiles < 0 || adpcm_len < 0 || seek_entries < 0) { set_error("negative count / length"); return VGA_ERR_ARGUMENT; }
    if (nfiles == 0) return VGA_OK;
    if (!d_files || !d_coefs || (adpcm_len > 0 && !d_adpcm) || (seek_entries > 0 && !d_seek)) {
        set_error("null device pointer");
        return VGA_ERR_ARGUMENT;
    }
    if (adpcm_len > 0 && adpcm_pitch < adpcm_len) { set_error("adpcm pitch < length"); return VGA_ERR_ARGUMENT; }
    if (seek_entries > 0 && seek_pitch < 2 * (int64_t)seek_entries) { set_error("seek pitch < 2 * entries"); return VGA_ERR_ARGUMENT; }
    if (int rc = check_write_files(nfiles, nch, file_pitch, L.file_size)) return rc;
    hipStream_t s = (hipStream_t)stream;
    nwstm::HeaderArgs a;
    header_args(L, p, nch, tracks, &a);
    hipLaunchKernelGGL(nwstm::nw_header_kernel, dim3(nfiles), dim3(64), 0, s, a, d_adpcm, adpcm_pitch, adpcm_len, d_coefs,
                       d_gain, d_start_context, d_loop_context, d_files, file_pitch);
    VGA_HIP_TRY(hipGetLastError());
    const int body_shorts = (L.seek_block_size - 8) / 2;
    for (int f0 = 0; f0 < nfiles; f0 += nwstm::kMaxGridY) {
        const int nf = std::min(nfiles - f0, nwstm::kMaxGridY);
        hipLaunchKernelGGL(nwstm::nw_seek_kernel, dim3((body_shorts + 255) / 256, nf), dim3(256), 0, s,
                           d_seek ? d_seek + (int64_t)f0 * nch * seek_pitch : nullptr, seek_pitch, seek_entries, nch,
                           L.seek_table_entry_count, L.endianness == VGA_NW_BIG_ENDIAN && p->target == VGA_NW_RSTM,
                           L.seek_block_offset, L.seek_block_size, d_files + (int64_t)f0 * file_pitch, file_pitch);
        VGA_HIP_TRY(hipGetLastError());
    }
    return interleave_images(d_adpcm, adpcm_pitch, nch, nfiles, (uint32_t)adpcm_len, (uint32_t)L.interleave_size,
                             (uint32_t)L.audio_data_size, d_files + L.audio_data_offset, file_pitch, s);
}

int vga_nwstm_write(const vga_nwstm_params *p, int nch, const vga_nw_track *tracks, const uint8_t *const *adpcm, int adpcm_len,
                    const int16_t *coefs, const int16_t *gain, const int16_t *start_context, const int16_t *loop_context,
                    const int16_t *const *seek, int seek_entries, uint8_t *file_out)
{
    vga_nwstm_layout L;
    if (int rc = vga_nwstm_layout_for(p, nch, &L)) return rc;
    if (int rc = check_track_list(p, tracks)) return rc;
    if (adpcm_len < 0 || seek_entries < 0) { set_error("negative length"); return VGA_ERR_ARGUMENT; }
    if (!coefs || !file_out || (adpcm_len > 0 && !adpcm) || (seek_entries > 0 && !seek)) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    for (int c = 0; c < nch; c++)
        if ((adpcm_len > 0 && !adpcm[c]) || (seek_entries > 0 && !seek[c])) { set_error("channel %d: null pointer", c); return VGA_ERR_ARGUMENT; }
    HostStage h;
    uint8_t *d_adpcm = nullptr;
    int16_t *d_seek = nullptr;
    const int16_t *d_coefs = nullptr, *d_gain = nullptr, *d_sc = nullptr, *d_lc = nullptr;
    int64_t apitch = 0, spitch = 0;
    if (int rc = h.open()) return rc;
    if (int rc = h.rows(adpcm, nch, adpcm_len, &d_adpcm, &apitch)) return rc;
    if (int rc = h.rows(seek, nch, 2 * seek_entries, &d_seek, &spitch)) return rc;
    if (int rc = h.table(coefs, (size_t)nch * 16, &d_coefs)) return rc;
    if (int rc = h.table(gain, (size_t)nch, &d_gain)) return rc;
    if (int rc = h.table(start_context, (size_t)nch * 3, &d_sc)) return rc;
    if (int rc = h.table(loop_context, (size_t)nch * 3, &d_lc)) return rc;
    return h.write_image(file_out, (size_t)L.file_size, [&](uint8_t *d_file, hipStream_t s) {
        return vga_nwstm_write_device(p, nch, 1, tracks, d_adpcm, apitch, adpcm_len, d_coefs, d_gain, d_sc, d_lc, d_seek, spitch,
                                      seek_entries, d_file, L.file_size, s);
    });
}

// BrstmReader.ReadFile / BCFstmReader.ReadFile up to the audio (host only): the checks of the reference readers,
// then what Common.ToAdpcmStream (Common.cs:67-97) needs.
// pcm: the PCM8 / PCM16 streams vga_nwstm_pcm_parse reads; else the GC-ADPCM ones of vga_nwstm_parse
static int parse_nw(const uint8_t *file, size_t size, vga_nwstm_info *out, bool pcm)
{
    if (!file || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    std::memset(out, 0, sizeof *out);
    const int64_t len = (int64_t)size;
    if (len < 4) return invalid("file is too short for a NintendoWare header");
    ByteReader r{file, len, 0, true};
    vga_nwstm_info &I = *out;
    if (!std::memcmp(file, "RSTM", 4)) {                    // BrstmReader.cs
        I.target = VGA_NW_RSTM;
        I.endianness = VGA_NW_BIG_ENDIAN;
        r.pos = 4;
        if (r.u16() != 0xfeff) return invalid("Expected byte order mark 0xFEFF");
        const int major = r.u8(), minor = r.u8();
        I.version = (uint32_t)major << 24 | (uint32_t)minor << 16;
        I.file_size = r.i32();
        if (r.eof) return invalid("file ends inside the RSTM header");
        if (len < I.file_size) return invalid("Actual file length is less than stated length");
        r.i16();
        r.i16();
        I.head_block_offset = r.i32(); I.head_block_size = r.i32();
        I.seek_block_offset = r.i32(); I.seek_block_size = r.i32();
        I.data_block_offset = r.i32(); I.data_block_size = r.i32();
        if (r.eof) return invalid("file ends inside the RSTM header");
        r.pos = I.head_block_offset;
        if (!r.magic("HEAD", 4)) return invalid("Unknown or invalid HEAD block");
        if (r.i32() != I.head_block_size) return invalid("HEAD block size in RSTM header doesn't match size in HEAD header");
        const int base = (int)r.pos;
        const Ref si = read_ref(r, base), ti = read_ref(r, base), ci = read_ref(r, base);
        if (r.eof) return invalid("file ends inside the HEAD block");
        if (!si.is(kByteTable)) return invalid("Could not read stream info.");
        r.pos = si.abs();                                   // StreamInfo.ReadBrstm
        I.codec = r.u8();
        I.looping = r.u8() != 0;
        I.channel_count = r.u8();
        r.pos += 1;
        I.sample_rate = r.u16();
        r.pos += 2;
        I.loop_start = r.i32();
        I.sample_count = r.i32();
        I.audio_data_offset = r.i32();
        I.interleave_count = r.i32();
        I.interleave_size = r.i32();
        I.samples_per_interleave = r.i32();
        I.last_block_size_without_padding = r.i32();
        I.last_block_samples = r.i32();
        I.last_block_size = r.i32();
        I.samples_per_seek_table_entry = r.i32();
        I.bytes_per_seek_table_entry = r.i32();
        if (r.eof) return invalid("file ends inside the stream info");
        if (!pcm && I.codec != kCodecGcAdpcm) { set_error("BRSTM codec %d (PCM8 = 0, PCM16 = 1) is not GC-ADPCM", I.codec); return VGA_ERR_INVALID_OP; }
        if (pcm) { if (int rc = pcm_codec_check(I.codec)) return rc; }
        if (!ti.is(kByteTable)) return invalid("Could not read track info.");
        r.pos = ti.abs();                                   // TrackInfo.ReadBrstm
        I.track_count = r.u8();
        I.track_type = r.u8() == 0 ? VGA_NW_TRACK_SHORT : VGA_NW_TRACK_STANDARD;
        r.pos += 2;
        Ref tr[256];
        for (int i = 0; i < I.track_count; i++) tr[i] = read_ref(r, ti.base);
        for (int i = 0; i < I.track_count; i++) {
            vga_nw_track &t = I.tracks[i];
            r.pos = tr[i].abs();
            t.volume = 0x7f; t.panning = 0x40;
            if ((tr[i].type & 0xff) == 1) { t.volume = r.u8(); t.panning = r.u8(); r.pos += 6; }
            t.channel_count = r.u8();
            t.left = r.u8();
            t.right = r.u8();
        }
        if (r.eof) return invalid("file ends inside the track info");
        if (!ci.is(kByteTable)) return invalid("Could not read channel info.");
        r.pos = ci.abs();                                   // ChannelInfo.ReadBrstm
        const int cc = r.u8();
        r.pos += 3;
        Ref ch[256];
        for (int i = 0; i < cc; i++) ch[i] = read_ref(r, ci.base);
        int found = 0;
        for (int i = 0; i < cc; i++) {
            r.pos = ch[i].abs();
            const Ref ad = read_ref(r, ci.base);
            if (ad.offset <= 0) continue;
            r.pos = ad.abs();
            for (int k = 0; k < 16; k++) I.coefs[found][k] = (int16_t)r.i16();
            I.gain[found] = (int16_t)r.i16();
            for (int k = 0; k < 3; k++) I.start_context[found][k] = (int16_t)r.i16();
            for (int k = 0; k < 3; k++) I.loop_context[found][k] = (int16_t)r.i16();
            found++;
        }
        if (r.eof) return invalid("file ends inside the channel info");
        if (!pcm && found < I.channel_count) return invalid("fewer channel infos than channels");
        if (I.seek_block_offset != 0) {                     // ReadAdpcBlock
            r.pos = I.seek_block_offset;
            if (!r.magic("ADPC", 4)) return invalid("Unknown or invalid ADPC block");
            if (r.i32() != I.seek_block_size) return invalid("ADPC block size in RSTM header doesn't match size in ADPC header");
            if (I.samples_per_seek_table_entry <= 0) return invalid("samples per seek table entry must be positive");
            const bool full = I.sample_count % I.samples_per_seek_table_entry == 0 && I.sample_count > 0;
            const int per = 4 * I.channel_count;
            const int n_short = bytes_of(I.sample_count) / I.samples_per_seek_table_entry + 1;
            const int n_std = I.sample_count / I.samples_per_seek_table_entry + (full ? 0 : 1);
            if (I.seek_block_size == (int)next_multiple(8 + (int64_t)n_std * per, 0x20)) {
                I.seek_table_type = VGA_NW_SEEK_STANDARD;
                I.seek_entries = n_std;
            } else if (I.seek_block_size == (int)next_multiple(8 + (int64_t)n_short * per, 0x20)) {
                I.seek_table_type = VGA_NW_SEEK_SHORT;
                I.seek_entries = n_short;
            }                                               // else: unknown layout, the table is not read
            I.seek_table_offset = I.seek_block_offset + 8;
        }
        r.pos = I.data_block_offset;                        // ReadDataBlock
        if (!r.magic("DATA", 4)) return invalid("Unknown or invalid DATA block");
        if (r.i32() != I.data_block_size) return invalid("DATA block size in main header doesn't match size in DATA header");
        I.audio_data_length = I.data_block_size - (I.audio_data_offset - I.data_block_offset);
    } else {                                                // BCFstmReader.cs
        const bool known = !std::memcmp(file, "CSTM", 4) || !std::memcmp(file, "FSTM", 4);
        if (!known) {
            if (!std::memcmp(file, "CWAV", 4) || !std::memcmp(file, "FWAV", 4) || !std::memcmp(file, "CSTP", 4) ||
                !std::memcmp(file, "FSTP", 4)) {
                set_error("%.4s files (wave / prefetch) are not read here: only CSTM, FSTM and RSTM streams", (const char *)file);
                return VGA_ERR_INVALID_OP;
            }
            return invalid("File has no CSTM or FSTM header");
        }
        I.target = file[0] == 'C' ? VGA_NW_CSTM : VGA_NW_FSTM;
        if (len < 6) return invalid("File has no byte order mark");
        const int bom = file[4] | file[5] << 8;
        if (bom == 0xFEFF) I.endianness = VGA_NW_LITTLE_ENDIAN;
        else if (bom == 0xFFFE) I.endianness = VGA_NW_BIG_ENDIAN;
        else return invalid("File has no byte order mark");
        r.big = I.endianness == VGA_NW_BIG_ENDIAN;
        r.pos = 6;
        r.i16();                                            // HeaderSize
        I.version = (uint32_t)r.i32();
        I.file_size = r.i32();
        if (r.eof) return invalid("file ends inside the header");
        if (len < I.file_size) return invalid("Actual file length is less than stated length");
        const int nblocks = r.i16();
        r.pos += 2;
        Ref info{}, seek{}, data{};
        int info_size = 0, seek_size = 0, data_size = 0;
        bool have_info = false, have_seek = false, have_data = false, prefetch = false;
        for (int i = 0; i < nblocks && !r.eof; i++) {
            const Ref b = read_ref(r, 0);
            const int bs = r.i32();
            if (!have_info && (b.type == kStreamInfoBlock || b.type == 0x7000)) { info = b; info_size = bs; have_info = true; }
            if (!have_seek && b.type == kStreamSeekBlock) { seek = b; seek_size = bs; have_seek = true; }
            if (!have_data && (b.type == kStreamDataBlock || b.type == kStreamPrefetchDataBlock || b.type == 0x7001)) {
                data = b; data_size = bs; have_data = true; prefetch = b.type != kStreamDataBlock;
            }
        }
        if (r.eof) return invalid("file ends inside the block table");
        if (!have_info) return invalid("File has no INFO block");
        if (info.type != kStreamInfoBlock || prefetch) { set_error("wave / prefetch blocks are not read here"); return VGA_ERR_INVALID_OP; }
        r.pos = info.abs();
        if (!r.magic("INFO", 4)) return invalid("Unknown or invalid INFO block");
        if (r.i32() != info_size) return invalid("INFO block size in main header doesn't match size in INFO header");
        const int base = (int)r.pos;
        const Ref si = read_ref(r, base), ti = read_ref(r, base), ci = read_ref(r, base);
        if (r.eof) return invalid("file ends inside the INFO block");
        if (!si.is(kStreamInfo)) return invalid("Could not read stream info.");
        r.pos = si.abs();                                   // StreamInfo.ReadBfstm
        I.codec = r.u8();
        I.looping = r.u8() != 0;
        I.channel_count = r.u8();
        r.u8();                                             // RegionCount
        I.sample_rate = r.i32();
        I.loop_start = r.i32();
        I.sample_count = r.i32();
        I.interleave_count = r.i32();
        I.interleave_size = r.i32();
        I.samples_per_interleave = r.i32();
        I.last_block_size_without_padding = r.i32();
        I.last_block_samples = r.i32();
        I.last_block_size = r.i32();
        I.bytes_per_seek_table_entry = r.i32();
        I.samples_per_seek_table_entry = r.i32();
        const Ref audio = read_ref(r, 0);
        if (include_region_info(I.version)) { r.i16(); r.pos += 2; read_ref(r, 0); }
        if (include_unaligned_loop(I.version)) { I.loop_start_unaligned = r.i32(); I.loop_end_unaligned = r.i32(); I.has_unaligned_loop = 1; }
        if (include_checksum(I.version)) r.i32();
        if (r.eof) return invalid("file ends inside the stream info");
        if (!pcm && I.codec != kCodecGcAdpcm) { set_error("stream codec %d (PCM8 = 0, PCM16 = 1) is not GC-ADPCM", I.codec); return VGA_ERR_INVALID_OP; }
        if (pcm) { if (int rc = pcm_codec_check(I.codec)) return rc; }
        I.track_type = VGA_NW_TRACK_STANDARD;
        if (ti.is(kReferenceTable)) {                       // TrackInfo.ReadBfstm
            r.pos = ti.abs();
            const int tbase = (int)r.pos;
            const int n = r.i32();
            if (n < 0 || n > VGA_NW_MAX_TRACKS) return invalid("track count out of range");
            Ref tr[VGA_NW_MAX_TRACKS];
            for (int i = 0; i < n; i++) tr[i] = read_ref(r, tbase);
            for (int i = 0; i < n; i++) {
                vga_nw_track &t = I.tracks[i];
                r.pos = tr[i].abs();
                t.volume = r.u8();
                t.panning = r.u8();
                r.u8();
                r.u8();
                const Ref cref = read_ref(r, tr[i].abs());
                r.pos = cref.abs();
                t.channel_count = r.i32();
                t.left = r.u8();
                t.right = r.u8();
            }
            I.track_count = n;
            I.has_track_info = 1;
        }
        if (r.eof) return invalid("file ends inside the track info");
        if (ci.is(kReferenceTable)) {                       // ChannelInfo.ReadBfstm
            r.pos = ci.abs();
            const int cbase = (int)r.pos;
            const int n = r.i32();
            if (n < 0 || n > VGA_NW_MAX_CHANNELS) return invalid("channel count out of range");
            Ref ch[VGA_NW_MAX_CHANNELS];
            for (int i = 0; i < n; i++) ch[i] = read_ref(r, cbase);
            int found = 0;
            for (int i = 0; i < n; i++) {
                r.pos = ch[i].abs();
                const Ref ad = read_ref(r, ch[i].abs());
                if (!ad.is(kGcAdpcmInfo)) continue;
                r.pos = ad.abs();
                for (int k = 0; k < 16; k++) I.coefs[found][k] = (int16_t)r.i16();
                for (int k = 0; k < 3; k++) I.start_context[found][k] = (int16_t)r.i16();
                for (int k = 0; k < 3; k++) I.loop_context[found][k] = (int16_t)r.i16();
                found++;
            }
            if (!pcm && found < I.channel_count) return invalid("fewer channel infos than channels");
        } else {
            return invalid("Could not read channel info.");
        }
        if (r.eof) return invalid("file ends inside the channel info");
        I.head_block_offset = info.abs();
        I.head_block_size = info_size;
        if (have_seek) {                                    // ReadSeekBlock
            r.pos = seek.abs();
            if (!r.magic("SEEK", 4)) return invalid("Unknown or invalid SEEK block");
            if (r.i32() != seek_size) return invalid("SEEK block size in main header doesn't match size in SEEK header");
            if (I.samples_per_seek_table_entry <= 0) return invalid("samples per seek table entry must be positive");
            I.seek_block_offset = seek.abs();
            I.seek_block_size = seek_size;
            I.seek_table_offset = seek.abs() + 8;
            I.seek_entries = div_round_up(I.sample_count, I.samples_per_seek_table_entry);
        }
        if (!have_data) return invalid("File has no DATA block");
        r.pos = data.abs();                                 // ReadDataBlock
        if (!r.magic("DATA", 4)) return invalid("Unknown or invalid DATA block");
        if (r.i32() != data_size) return invalid("DATA block size in main header doesn't match size in DATA header");
        I.data_block_offset = data.abs();
        I.data_block_size = data_size;
        I.audio_data_offset = data.abs() + audio.offset + 8;
        I.audio_data_length = data_size - (I.audio_data_offset - data.abs());
    }
    if (I.channel_count < 1) return invalid("the stream has no channels");
    if (I.sample_count < 0 || I.loop_start < 0) return invalid("negative sample count / loop start");
    if (I.looping && I.loop_start > I.sample_count) return invalid("loop start past the end of the stream");
    if (I.seek_entries > 0) {                               // ReadBytes(seekTableSize) stops at the end of the file
        const int64_t avail = std::max<int64_t>(0, len - I.seek_table_offset) / (4 * I.channel_count);
        if (avail < I.seek_entries) I.seek_entries = (int)avail;
    }
    I.seek_big_endian = I.target == VGA_NW_RSTM;             // the SEEK table is little-endian in every BCSTM / BFSTM
    // DeInterleave (Interleave.cs:118-133): the block must hold `length` bytes, equally split over the channels
    if (I.interleave_size <= 0) return invalid("interleave size must be positive");
    if (I.audio_data_length < 0 || I.audio_data_offset < 0 || I.audio_data_offset + (int64_t)I.audio_data_length > len)
        return invalid("Specified length is greater than the number of bytes remaining in the Stream");
    if (I.audio_data_length % I.channel_count != 0) return invalid("The input length must be divisible by the number of outputs.");
    if (pcm) {                                              // Common.SamplesToBytes(SampleCount, Codec)
        const int64_t row = (int64_t)I.sample_count * (I.codec == kCodecPcm16 ? 2 : 1);
        if (row > 0x7FFFFFFF) return invalid("sample count too large for one channel's bytes");
        std::memset(I.coefs, 0, sizeof I.coefs);
        std::memset(I.gain, 0, sizeof I.gain);
        std::memset(I.start_context, 0, sizeof I.start_context);
        std::memset(I.loop_context, 0, sizeof I.loop_context);
        I.adpcm_bytes = (int)row;
        return VGA_OK;
    }
    I.adpcm_bytes = bytes_of(I.sample_count);
    return VGA_OK;
}

int vga_nwstm_parse(const uint8_t *file, size_t size, vga_nwstm_info *out) { return parse_nw(file, size, out, false); }

int vga_nwstm_read_device(const vga_nwstm_info *I, const uint8_t *d_files, int64_t file_pitch, int nfiles, uint8_t *d_adpcm,
                          int64_t adpcm_pitch, void *stream)
{
    if (!I || nfiles < 0) { set_error("null / negative argument"); return VGA_ERR_ARGUMENT; }
    if (nfiles == 0 || I->adpcm_bytes == 0) return VGA_OK;
    const int nch = I->channel_count;
    if (nch < 1 || I->interleave_size <= 0 || I->audio_data_length < 0 || I->audio_data_length % nch) { set_error("info does not describe a stream"); return VGA_ERR_ARGUMENT; }
    if (int rc = check_read_batch(d_files, d_adpcm, adpcm_pitch, I->adpcm_bytes, nfiles, file_pitch,
                                  (int64_t)I->audio_data_offset + I->audio_data_length))
        return rc;
    return deinterleave_images(d_files, file_pitch, nfiles, I->audio_data_offset, nch, (uint32_t)(I->audio_data_length / nch),
                               (uint32_t)I->interleave_size, (uint32_t)I->adpcm_bytes, d_adpcm, adpcm_pitch, (hipStream_t)stream);
}

int vga_nwstm_read(const uint8_t *file, size_t size, const vga_nwstm_info *I, uint8_t *const *adpcm_out, int16_t *const *seek_out)
{
    if (!file || !I || !adpcm_out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    const int nch = I->channel_count;
    if ((int64_t)I->audio_data_offset + I->audio_data_length > (int64_t)size) { set_error("info does not describe this file"); return VGA_ERR_ARGUMENT; }
    for (int c = 0; c < nch; c++)
        if (!adpcm_out[c] || (seek_out && I->seek_entries > 0 && !seek_out[c])) { set_error("channel %d: null pointer", c); return VGA_ERR_ARGUMENT; }
    if (seek_out && I->seek_entries > 0) {                  // tableBytes.ToShortArray(endianness).DeInterleave(2, ChannelCount)
        const uint8_t *t = file + I->seek_table_offset;
        for (int e = 0; e < I->seek_entries; e++)
            for (int c = 0; c < nch; c++)
                for (int j = 0; j < 2; j++) {
                    const uint8_t *b = t + ((int64_t)e * nch + c) * 4 + 2 * j;
                    seek_out[c][2 * e + j] = (int16_t)(I->seek_big_endian ? (b[0] << 8 | b[1]) : (b[0] | b[1] << 8));
                }
    }
    if (I->adpcm_bytes == 0) return VGA_OK;
    const size_t bytes = (size_t)I->audio_data_offset + (size_t)I->audio_data_length;
    HostStage h;
    return h.read_rows(file, bytes, adpcm_out, nch, I->adpcm_bytes, 1, [&](const uint8_t *f, void *d, int64_t dp, hipStream_t s) {
        return vga_nwstm_read_device(I, f, (int64_t)bytes, 1, static_cast<uint8_t *>(d), dp, s);
    });
}


// ---------------------------------------------------------------- PCM8 / PCM16 streams (the writers' Codec != GcAdpcm)

// BxstmConfiguration with Codec = Pcm16Bit / Pcm8Bit and the size math of BrstmWriter.cs:22-74 / BCFstmWriter.cs:23-83
int vga_nwstm_pcm_layout_for(const vga_nwstm_params *p, int codec, int nch, vga_nwstm_layout *L)
{
    if (!p || !L) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    std::memset(L, 0, sizeof *L);
    if (codec != kCodecPcm8 && codec != kCodecPcm16) {
        set_error("codec %d: this call writes PCM8 (0) or PCM16 (1) streams (vga_nwstm_layout_for for GC-ADPCM)", codec);
        return VGA_ERR_ARGUMENT;
    }
    return nw_layout(p, codec, nch, L);
}

int vga_nwstm_pcm_write_device(const vga_nwstm_params *p, int codec, int nch, int nfiles, const vga_nw_track *tracks,
                               const void *d_samples, int sample_kind, int64_t pitch, uint8_t *d_files, int64_t file_pitch,
                               void *stream)
{
    vga_nwstm_layout L;
    if (int rc = vga_nwstm_pcm_layout_for(p, codec, nch, &L)) return rc;
    if (int rc = check_track_list(p, tracks)) return rc;
    if (int rc = check_sample_kind(sample_kind)) return rc;
    if (codec == kCodecPcm16 && sample_kind != VGA_SAMPLES_S16) { set_error("a PCM16 stream is written from VGA_SAMPLES_S16 rows"); return VGA_ERR_ARGUMENT; }
    if (nfiles < 0) { set_error("negative file count"); return VGA_ERR_ARGUMENT; }
    if (nfiles == 0) return VGA_OK;
    if (!d_files || (p->sample_count > 0 && !d_samples)) { set_error("null device pointer"); return VGA_ERR_ARGUMENT; }
    if (p->sample_count > 0 && pitch < p->sample_count) { set_error("pitch < sample count"); return VGA_ERR_ARGUMENT; }
    if (int rc = check_write_files(nfiles, nch, file_pitch, L.file_size)) return rc;
    hipStream_t s = (hipStream_t)stream;
    nwstm::HeaderArgs a;
    header_args(L, p, nch, tracks, &a, codec);
    hipLaunchKernelGGL(nwstm::nw_header_kernel, dim3(nfiles), dim3(64), 0, s, a, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr,
                       d_files, file_pitch);
    VGA_HIP_TRY(hipGetLastError());
    const uint32_t in = (uint32_t)L.channel_adpcm_bytes, il = (uint32_t)L.interleave_size, out = (uint32_t)L.audio_data_size;
    uint8_t *audio = d_files + L.audio_data_offset;
    if (out == 0) return VGA_OK;
    if (sample_kind == VGA_SAMPLES_8BIT || (codec == kCodecPcm16 && L.endianness == VGA_NW_LITTLE_ENDIAN))   // the rows' bytes are the file's
        return interleave_images(static_cast<const uint8_t *>(d_samples), sample_kind == VGA_SAMPLES_S16 ? pitch * 2 : pitch, nch, nfiles,
                                 in, il, out, audio, file_pitch, s);
    return pcm::launch_interleave_files(codec == kCodecPcm16 ? pcm::kSwap16 : pcm::kPcm8, static_cast<const int16_t *>(d_samples),
                                        pitch, nch, nfiles, in, il, out, audio, file_pitch, s);
}

int vga_nwstm_pcm_write(const vga_nwstm_params *p, int codec, int nch, const vga_nw_track *tracks, const void *const *samples,
                        int sample_kind, uint8_t *file_out)
{
    vga_nwstm_layout L;
    if (int rc = vga_nwstm_pcm_layout_for(p, codec, nch, &L)) return rc;
    if (int rc = check_track_list(p, tracks)) return rc;
    if (int rc = check_sample_kind(sample_kind)) return rc;
    if (!file_out || (p->sample_count > 0 && !samples)) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    for (int c = 0; c < nch && p->sample_count > 0; c++)
        if (!samples[c]) { set_error("channel %d: null pointer", c); return VGA_ERR_ARGUMENT; }
    HostStage h;
    void *d_in = nullptr;
    int64_t pitch = 0;
    if (int rc = h.open()) return rc;
    if (int rc = h.rows(samples, nch, p->sample_count, sample_kind == VGA_SAMPLES_S16 ? 2 : 1, &d_in, &pitch)) return rc;
    return h.write_image(file_out, (size_t)L.file_size, [&](uint8_t *d_file, hipStream_t s) {
        return vga_nwstm_pcm_write_device(p, codec, nch, 1, tracks, d_in, sample_kind, pitch, d_file, L.file_size, s);
    });
}

// BrstmReader / BCFstmReader up to the audio for PCM8 / PCM16 streams (Common.ToPcm16Stream / ToPcm8Stream)
int vga_nwstm_pcm_parse(const uint8_t *file, size_t size, vga_nwstm_info *out) { return parse_nw(file, size, out, true); }

int vga_nwstm_pcm_read_device(const vga_nwstm_info *I, const uint8_t *d_files, int64_t file_pitch, int nfiles, void *d_samples,
                              int sample_kind, int64_t pitch, void *stream)
{
    if (!I || nfiles < 0) { set_error("null / negative argument"); return VGA_ERR_ARGUMENT; }
    if (I->codec != kCodecPcm8 && I->codec != kCodecPcm16) { set_error("info is not a PCM8 / PCM16 stream (vga_nwstm_pcm_parse)"); return VGA_ERR_ARGUMENT; }
    if (int rc = check_sample_kind(sample_kind)) return rc;
    if (I->codec == kCodecPcm16 && sample_kind != VGA_SAMPLES_S16) { set_error("a PCM16 stream is read to VGA_SAMPLES_S16 rows"); return VGA_ERR_ARGUMENT; }
    const int bps = I->codec == kCodecPcm16 ? 2 : 1;
    if (nfiles == 0 || I->adpcm_bytes == 0) return VGA_OK;
    const int nch = I->channel_count;
    if (nch < 1 || I->interleave_size <= 0 || I->audio_data_length < 0 || I->audio_data_length % nch || I->adpcm_bytes != I->sample_count * bps) {
        set_error("info does not describe a stream");
        return VGA_ERR_ARGUMENT;
    }
    if (int rc = check_read_batch(d_files, d_samples, pitch, I->sample_count, nfiles, file_pitch,
                                  (int64_t)I->audio_data_offset + I->audio_data_length))
        return rc;
    const uint32_t in = (uint32_t)(I->audio_data_length / nch), il = (uint32_t)I->interleave_size, out = (uint32_t)I->adpcm_bytes;
    hipStream_t s = (hipStream_t)stream;
    if (sample_kind == VGA_SAMPLES_8BIT || (I->codec == kCodecPcm16 && I->endianness == VGA_NW_LITTLE_ENDIAN))   // the file's bytes are the rows'
        return deinterleave_images(d_files, file_pitch, nfiles, I->audio_data_offset, nch, in, il, out, static_cast<uint8_t *>(d_samples),
                                   sample_kind == VGA_SAMPLES_S16 ? pitch * 2 : pitch, s);
    return pcm::launch_deinterleave(I->codec == kCodecPcm16 ? pcm::kSwap16 : pcm::kPcm8, d_files, file_pitch, I->audio_data_offset, nch,
                                    nfiles * nch, in, il, out, static_cast<int16_t *>(d_samples), pitch, s);
}

int vga_nwstm_pcm_read(const uint8_t *file, size_t size, const vga_nwstm_info *I, void *const *out, int sample_kind)
{
    if (!file || !I || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (int rc = check_sample_kind(sample_kind)) return rc;
    const int nch = I->channel_count;
    if (I->audio_data_offset < 0 || (int64_t)I->audio_data_offset + I->audio_data_length > (int64_t)size) { set_error("info does not describe this file"); return VGA_ERR_ARGUMENT; }
    for (int c = 0; c < nch; c++)
        if (!out[c]) { set_error("channel %d: null pointer", c); return VGA_ERR_ARGUMENT; }
    if (I->sample_count == 0) return VGA_OK;
    const size_t bytes = (size_t)I->audio_data_offset + (size_t)I->audio_data_length;
    HostStage h;
    return h.read_rows(file, bytes, out, nch, I->sample_count, sample_kind == VGA_SAMPLES_S16 ? 2 : 1,
                       [&](const uint8_t *f, void *d, int64_t dp, hipStream_t s) {
                           return vga_nwstm_pcm_read_device(I, f, (int64_t)bytes, 1, d, sample_kind, dp, s);
                       });
}

}  // extern "C"
