// nw_header_body.hpp -- what one workgroup writes in front of the audio of one NintendoWare stream image: the file header,
// HEAD (BrstmWriter.cs:130-260) or INFO (BCFstmWriter.cs:171-333), the 8-byte headers of the ADPC / SEEK and DATA blocks and
// the zeros between them.  One body for the equally shaped files of nwstm.hip (pitched rows, the caller's track list as a
// kernel argument) and for the sets of nw_files_kernels.hip (packed rows, the default track list computed in place): the
// caller's policy P says where a channel's row of the per-channel arrays is, what its first ADPCM byte is and what track
// i is.
//   struct P { __device__ int row(int ch) const;            // index into coefs / gain / the contexts (int or int64_t)
//              __device__ int first_byte(int ch) const;     // Adpcm[0] of the channel, 0 for a channel without bytes
//              __device__ nw::TrackK track(int i) const; };
#pragma once
#include "common.hpp"
#include "nw_host.hpp"

namespace vga {
namespace nw {

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

// AudioTrack.GetDefaultTrackList (Formats/AudioTrack.cs:69-82): track i of nch channels
__device__ inline TrackK default_track(int nch, int i)
{
    const int cc = nch - i * 2 < 2 ? nch - i * 2 : 2;
    return {cc, (uint8_t)(i * 2), (uint8_t)(cc >= 2 ? i * 2 + 1 : 0), 0x7f, 0x40};
}

// Called by all 64 threads of a workgroup: they zero everything in front of the seek block (of the DATA block for PCM, which
// has none) and between the DATA header and the audio, then lane 0 writes the headers.  PCM streams take the writers'
// Codec != GcAdpcm branches.
template <class P>
__device__ void write_header(const HeaderGeom &a, const P &p, const int16_t *__restrict__ coefs, const int16_t *__restrict__ gain,
                             const int16_t *__restrict__ start_ctx, const int16_t *__restrict__ loop_ctx, uint8_t *__restrict__ img)
{
    const bool gc = a.codec == kCodecGcAdpcm;
    for (int k = threadIdx.x, end = gc ? a.seek_offset : a.data_offset; k < end; k += 64) img[k] = 0;
    for (int k = a.data_offset + threadIdx.x; k < a.audio_offset; k += 64) img[k] = 0;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int nch = a.nch;
    // GcAdpcmChannel.StartContext: (Adpcm[0], 0, 0) for a fresh channel (GcAdpcmChannel.cs:45)
    auto ctx = [&](Cursor &c, int ch, bool loop) {
        const auto r = p.row(ch);
        // the loop context written for a file that does not loop is the start context (BrstmWriter.cs:250, BCFstmWriter.cs:325)
        if (loop && a.looping) {
            for (int k = 0; k < 3; k++) c.put16(loop_ctx ? loop_ctx[r * 3 + k] : 0);
        } else if (start_ctx) {
            for (int k = 0; k < 3; k++) c.put16(start_ctx[r * 3 + k]);
        } else {
            c.put16(p.first_byte(ch));
            c.put16(0);
            c.put16(0);
        }
    };
    auto coef = [&](Cursor &c, int ch) { for (int k = 0; k < 16; k++) c.put16(coefs[p.row(ch) * 16 + k]); };
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
            const TrackK t = p.track(i);
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
            c.put16(gain ? gain[p.row(i)] : 0);
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
            const TrackK t = p.track(i);
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

}  // namespace nw
}  // namespace vga
