// nwwav_parse.hpp -- BrwavReader.ReadFile and the wave / prefetch branches of BCFstmReader.ReadFile up to the audio,
// then what Common.ToAudioStream needs.  Plain C++ over byte_reader.hpp (no HIP): nwwav.hip wraps it as
// vga_nwwav_parse, and tests/host/nwwav_parse_fuzz.cpp runs it under AddressSanitizer.
#pragma once
#include "byte_reader.hpp"
#include "../../include/vgaudio_hip_nwwav.h"

#include <cstdio>

namespace vga {
namespace nwwav {

using container::ByteReader;

// Structures/ReferenceType.cs
enum : int {
    kReferenceTable = 0x0101, kGcAdpcmInfo = 0x0300, kStreamInfoBlock = 0x4000, kStreamSeekBlock = 0x4001, kStreamDataBlock = 0x4002,
    kStreamRegionBlock = 0x4003, kStreamPrefetchDataBlock = 0x4004, kStreamInfo = 0x4100, kWaveInfoBlock = 0x7000,
    kWaveDataBlock = 0x7001, kWaveChannelInfo = 0x7100
};

struct Ref { int type, offset, base; int64_t abs() const { return (int64_t)base + offset; } bool is(int t) const { return type == t && offset > 0; } };
inline Ref read_ref(ByteReader &r, int64_t base) { Ref x; x.type = r.i16(); r.pos += 2; x.offset = r.i32(); x.base = (int)base; return x; }

// Common.cs:130-157 on a packed NwVersion
inline bool include_region_info(uint32_t v) { const int major = v >> 24; return (major >= 2 && v >= 0x02010000u) || major == 0; }
inline bool include_unaligned_loop(uint32_t v) { const int major = v >> 24; return (major == 0 && v >= 0x00040000u) || (major >= 2 && v >= 0x02030000u); }
inline bool include_checksum(uint32_t v) { return (v >> 24) == 0 && v >= 0x00050000u; }
inline bool include_unaligned_loop_wave(uint32_t v) { const int major = v >> 24; return (major == 0 && v >= 0x00010200u) || (major >= 2 && v >= 0x02010100u); }

// GcAdpcmMath.cs (C# division: towards zero)
inline int nibble_to_sample(int n) { return 14 * (n / 16) + n % 16 - 2; }
inline int nibbles_to_samples(int64_t n) { const int64_t extra = n % 16; return (int)(14 * (n / 16) + (extra < 2 ? 0 : extra - 2)); }
inline int64_t samples_to_bytes(int64_t samples, int codec)   // Common.SamplesToBytes
{
    if (codec == VGA_NW_CODEC_PCM16) return samples * 2;
    if (codec == VGA_NW_CODEC_PCM8) return samples;
    const int64_t extra = samples % 14, nibbles = 16 * (samples / 14) + (extra ? extra + 2 : 0);
    return (nibbles + 1) / 2;
}
inline int bytes_to_samples(int bytes, int codec)             // Common.BytesToSamples
{
    return codec == VGA_NW_CODEC_PCM16 ? bytes / 2 : codec == VGA_NW_CODEC_PCM8 ? bytes : nibbles_to_samples((int64_t)bytes * 2);
}

struct Failure { int code = VGA_OK; char msg[200] = {0}; };

struct Parser {
    const uint8_t *file;
    int64_t len;
    vga_nwwav_info &I;
    Failure &f;
    ByteReader r;

    Parser(const uint8_t *p, size_t size, vga_nwwav_info *out, Failure *fail) : file(p), len((int64_t)size), I(*out), f(*fail), r{p, (int64_t)size, 0, true} {}

    int fail(int code, const char *msg) { f.code = code; std::snprintf(f.msg, sizeof f.msg, "%s", msg); return code; }
    int invalid(const char *msg) { return fail(VGA_ERR_INVALID_DATA, msg); }

    // GcAdpcmChannelInfo: Coefs, (Gain,) Start, Loop
    void adpcm_info(int c, bool with_gain)
    {
        for (int k = 0; k < 16; k++) I.coefs[c][k] = (int16_t)r.i16();
        if (with_gain) I.gain[c] = (int16_t)r.i16();
        for (int k = 0; k < 3; k++) I.start_context[c][k] = (int16_t)r.i16();
        for (int k = 0; k < 3; k++) I.loop_context[c][k] = (int16_t)r.i16();
    }

    // what every kind ends with: the counts ToAudioStream's builders take and where ReadBytes(audioDataLength) reads
    int finish(bool prefetch)
    {
        if (I.codec != VGA_NW_CODEC_PCM8 && I.codec != VGA_NW_CODEC_PCM16 && I.codec != VGA_NW_CODEC_GCADPCM) return invalid("unknown codec");
        if (I.sample_count < 0) return invalid("negative sample count");
        if (I.looping && (I.loop_start < 0 || I.loop_start > I.sample_count)) return invalid("loop start outside the audio");
        const int64_t bytes = samples_to_bytes(I.sample_count, I.codec);
        if (bytes > 0x7FFFFFFF) return invalid("sample count too large for one channel's bytes");
        I.channel_bytes = (int)bytes;
        if (I.codec != VGA_NW_CODEC_GCADPCM) {
            std::memset(I.coefs, 0, sizeof I.coefs);
            std::memset(I.gain, 0, sizeof I.gain);
            std::memset(I.start_context, 0, sizeof I.start_context);
            std::memset(I.loop_context, 0, sizeof I.loop_context);
        }
        if (prefetch) return VGA_OK;                        // the region was checked as a whole
        for (int c = 0; c < I.channel_count; c++)
            if (I.audio_offset[c] < 0 || (int64_t)I.audio_offset[c] + bytes > len) return invalid("channel audio runs past the end of the file");
        return VGA_OK;
    }

    int rwav()                                              // BrwavReader.cs
    {
        I.kind = VGA_NWWAV_RWAV;
        I.endianness = VGA_NW_BIG_ENDIAN;
        r.pos = 4;
        if (len < 6) return invalid("file ends inside the RWAV header");
        const int bom = r.u16();
        if (bom != 0xfeff) {                                // reader.Expect((ushort)0xfeff), Extensions.cs:107-117
            f.code = VGA_ERR_INVALID_DATA;
            std::snprintf(f.msg, sizeof f.msg, "Expected 65279, but got %d at offset 0x4", bom);
            return f.code;
        }
        const int major = r.u8(), minor = r.u8();
        I.version = (uint32_t)major << 24 | (uint32_t)minor << 16;
        I.file_size = r.i32();
        if (r.eof) return invalid("file ends inside the RWAV header");
        if (len < I.file_size) return invalid("Actual file length is less than stated length");
        r.i16();                                            // HeaderSize
        r.i16();                                            // BlockCount
        const int head_offset = r.i32(), head_size = r.i32(), data_offset = r.i32(), data_size = r.i32();   // BrstmHeader.ReadBrwav
        if (r.eof) return invalid("file ends inside the RWAV header");
        r.pos = head_offset;
        if (!r.magic("INFO", 4)) return invalid("Unknown or invalid INFO block");
        if (r.i32() != head_size) return invalid("HEAD block size in RWAV header doesn't match size in HEAD header");
        const int64_t base = r.pos;                         // RwavWaveInfo.ReadBrwav
        I.codec = r.u8();
        I.looping = r.u8() != 0;
        I.channel_count = r.u8();
        r.pos += 1;
        I.sample_rate = r.u16();
        r.pos += 2;
        I.loop_start = nibble_to_sample(r.i32());
        I.sample_count = nibble_to_sample(r.i32());
        const int channel_info_offset = r.i32();
        r.i32();                                            // InfoStructureLength
        if (r.eof) return invalid("file ends inside the wave info");
        if (I.channel_count < 1) return invalid("the file has no channels");
        int offsets[VGA_NW_MAX_CHANNELS];
        r.pos = base + channel_info_offset;
        for (int c = 0; c < I.channel_count; c++) offsets[c] = r.i32();
        int audio[VGA_NW_MAX_CHANNELS];
        for (int c = 0; c < I.channel_count; c++) {         // RwavChannelInfo.Read
            r.pos = base + offsets[c];
            audio[c] = r.i32();
            const int adpcm_info_offset = r.i32();
            r.pos += 16;                                    // the four volumes
            r.pos = base + adpcm_info_offset;
            adpcm_info(c, true);
        }
        if (r.eof) return invalid("file ends inside the channel info");
        r.pos = data_offset;                                // ReadDataBlock
        if (!r.magic("DATA", 4)) return invalid("Unknown or invalid DATA block");
        if (r.i32() != data_size) return invalid("DATA block size in main header doesn't match size in DATA header");
        for (int c = 0; c < I.channel_count; c++) {
            const int64_t at = r.pos + audio[c];
            if (at < 0 || at > len) return invalid("channel audio runs past the end of the file");
            I.audio_offset[c] = (int)at;
        }
        return finish(false);
    }

    // ChannelInfo.ReadBfstm: the table's references, wave audio offsets where they are WaveChannelInfo, and the GC-ADPCM
    // infos of those that have one (compacted, as the reference's list is)
    int channel_table(int *count, int *waves, int *infos)
    {
        const int64_t base = r.pos;
        const int n = r.i32();
        if (r.eof) return invalid("file ends inside the channel info");
        if (n < 1 || n > VGA_NW_MAX_CHANNELS) return invalid("channel count out of range");
        Ref ch[VGA_NW_MAX_CHANNELS];
        for (int i = 0; i < n; i++) ch[i] = read_ref(r, base);
        *waves = *infos = 0;
        for (int i = 0; i < n; i++) {
            r.pos = ch[i].abs();
            if (ch[i].is(kWaveChannelInfo)) I.audio_offset[(*waves)++] = read_ref(r, 0).offset;
            const Ref ad = read_ref(r, ch[i].abs());
            if (!ad.is(kGcAdpcmInfo)) continue;
            r.pos = ad.abs();
            adpcm_info((*infos)++, false);
        }
        if (r.eof) return invalid("file ends inside the channel info");
        *count = n;
        return VGA_OK;
    }

    int bcf()                                               // BCFstmReader.cs
    {
        if (len < 6) return invalid("File has no byte order mark");
        const int bom = file[4] | file[5] << 8;
        if (bom == 0xFEFF) I.endianness = VGA_NW_LITTLE_ENDIAN;
        else if (bom == 0xFFFE) I.endianness = VGA_NW_BIG_ENDIAN;
        else return invalid("File has no byte order mark");
        r.big = I.endianness == VGA_NW_BIG_ENDIAN;
        r.pos = 6;                                          // ReadHeader
        r.i16();                                            // HeaderSize
        I.version = (uint32_t)r.i32();
        I.file_size = r.i32();
        if (r.eof) return invalid("file ends inside the header");
        if (len < I.file_size) return invalid("Actual file length is less than stated length");
        const int nblocks = r.i16();
        r.pos += 2;
        Ref info{}, seek{}, region{}, data{};
        int info_size = 0, seek_size = 0, region_size = 0, data_size = 0;
        bool have_info = false, have_seek = false, have_region = false, have_data = false;
        for (int i = 0; i < nblocks && !r.eof; i++) {       // SizedReference, FirstOrDefault of each kind
            const Ref b = read_ref(r, 0);
            const int bs = r.i32();
            if (!have_info && (b.type == kStreamInfoBlock || b.type == kWaveInfoBlock)) { info = b; info_size = bs; have_info = true; }
            if (!have_seek && b.type == kStreamSeekBlock) { seek = b; seek_size = bs; have_seek = true; }
            if (!have_region && b.type == kStreamRegionBlock) { region = b; region_size = bs; have_region = true; }
            if (!have_data && (b.type == kStreamDataBlock || b.type == kStreamPrefetchDataBlock || b.type == kWaveDataBlock)) {
                data = b; data_size = bs; have_data = true;
            }
        }
        if (r.eof) return invalid("file ends inside the block table");
        if (!have_info) return invalid("File has no INFO block");
        r.pos = info.abs();                                 // ReadInfoBlock
        if (!r.magic("INFO", 4)) return invalid("Unknown or invalid INFO block");
        if (r.i32() != info_size) return invalid("INFO block size in main header doesn't match size in INFO header");
        const bool wave = info.type == kWaveInfoBlock;
        int waves = 0, infos = 0;
        if (wave) {                                         // StreamInfo.ReadBfwav, ChannelInfo.ReadBfstm
            I.codec = r.u8();
            I.looping = r.u8() != 0;
            r.pos += 2;
            I.sample_rate = r.i32();
            I.loop_start = r.i32();
            I.sample_count = r.i32();
            if (include_unaligned_loop_wave(I.version)) { I.loop_start_unaligned = r.i32(); I.has_loop_start_unaligned = 1; }
            else r.pos += 4;
            if (r.eof) return invalid("file ends inside the wave info");
            if (int rc = channel_table(&I.channel_count, &waves, &infos)) return rc;
            if (waves < I.channel_count) return invalid("fewer wave audio offsets than channels");
        } else {                                            // the StreamInfoBlock case
            const int64_t base = r.pos;
            const Ref si = read_ref(r, base);
            read_ref(r, base);                              // track info: not part of what a prefetch file reads as
            const Ref ci = read_ref(r, base);
            if (r.eof) return invalid("file ends inside the INFO block");
            if (!si.is(kStreamInfo)) return invalid("Could not read stream info.");
            r.pos = si.abs();                               // StreamInfo.ReadBfstm
            I.codec = r.u8();
            I.stream_looping = r.u8() != 0;
            I.channel_count = r.u8();
            r.u8();                                         // RegionCount
            I.sample_rate = r.i32();
            I.loop_start = r.i32();
            I.stream_sample_count = r.i32();
            I.interleave_count = r.i32();
            I.interleave_size = r.i32();
            I.samples_per_interleave = r.i32();
            I.last_block_size_without_padding = r.i32();
            I.last_block_samples = r.i32();
            I.last_block_size = r.i32();
            r.pos += 8 + 8;                                 // seek table entry sizes, the audio reference
            if (include_region_info(I.version)) r.pos += 12;
            if (include_unaligned_loop(I.version)) r.pos += 8;
            if (include_checksum(I.version)) r.pos += 4;
            if (!r.has(0)) return invalid("file ends inside the stream info");
            if (I.channel_count < 1) return invalid("the file has no channels");
            if (!ci.is(kReferenceTable)) return invalid("Could not read channel info.");
            r.pos = ci.abs();
            int n = 0;
            if (int rc = channel_table(&n, &waves, &infos)) return rc;
        }
        if (I.codec == VGA_NW_CODEC_GCADPCM && infos < I.channel_count) return invalid("fewer channel infos than channels");
        if (have_seek) {                                    // ReadSeekBlock, ReadRegionBlock: their headers
            r.pos = seek.abs();
            if (!r.magic("SEEK", 4)) return invalid("Unknown or invalid SEEK block");
            if (r.i32() != seek_size) return invalid("SEEK block size in main header doesn't match size in SEEK header");
        }
        if (have_region) {
            r.pos = region.abs();
            if (!r.magic("REGN", 4)) return invalid("Unknown or invalid REGN block");
            if (r.i32() != region_size) return invalid("REGN block size in main header doesn't match size in REGN header");
        }
        if (!have_data) return invalid("File has no DATA block");
        r.pos = data.abs();                                 // ReadDataBlock
        const bool is_data = r.magic("DATA", 4);
        if (!is_data && (r.eof || std::memcmp(file + r.pos - 4, "PDAT", 4) != 0)) return invalid("Unknown or invalid DATA block");
        if (r.i32() != data_size) return invalid("DATA block size in main header doesn't match size in DATA header");
        if (r.eof) return invalid("file ends inside the DATA block");
        if (wave != (data.type == kWaveDataBlock) || (!wave && data.type != kStreamPrefetchDataBlock))
            return invalid("the info and data blocks are not those of one wave or prefetch file");
        I.kind = wave ? (file[0] == 'C' ? VGA_NWWAV_CWAV : VGA_NWWAV_FWAV) : (file[0] == 'C' ? VGA_NWWAV_CSTP : VGA_NWWAV_FSTP);
        if (wave) {
            for (int c = 0; c < I.channel_count; c++) {
                const int64_t at = r.pos + I.audio_offset[c];
                if (at < 0 || at > len) return invalid("channel audio runs past the end of the file");
                I.audio_offset[c] = (int)at;
            }
            return finish(false);
        }
        I.prefetch_count = r.i32();                         // PrefetchData.ReadPrefetchData, all read, the first used
        if (r.eof || I.prefetch_count < 1) return invalid("the prefetch block holds no region");
        if (r.pos + (int64_t)I.prefetch_count * 20 > len) return invalid("file ends inside the prefetch regions");
        const int64_t base = r.pos;
        I.prefetch_start_sample = r.i32();
        I.prefetch_size = r.i32();
        r.i32();
        const Ref audio = read_ref(r, base);
        const int nch = I.channel_count, size = I.prefetch_size;
        // DeInterleave(Size, InterleaveSize, ChannelCount, Size) from the reference's position (Interleave.cs:118-133)
        if (size < 0 || audio.abs() < 0 || audio.abs() + size > len)
            return invalid("Specified length is greater than the number of bytes remaining in the Stream");
        if (size % nch != 0) return invalid("The input length must be divisible by the number of outputs.");
        if (I.interleave_size <= 0) return invalid("interleave size must be positive");
        I.prefetch_audio_offset = (int)audio.abs();
        I.looping = 0;                                      // Common.cs:51-52
        I.sample_count = bytes_to_samples(size / nch, I.codec);
        const int first = std::min(I.interleave_size, size / nch);
        for (int c = 0; c < nch; c++) I.audio_offset[c] = I.prefetch_audio_offset + c * first;
        return finish(true);
    }

    int run()
    {
        std::memset(&I, 0, sizeof I);
        if (len < 4) return invalid("file is too short for a NintendoWare header");
        if (!std::memcmp(file, "RSTM", 4) || !std::memcmp(file, "CSTM", 4) || !std::memcmp(file, "FSTM", 4)) {
            f.code = VGA_ERR_INVALID_OP;
            std::snprintf(f.msg, sizeof f.msg, "%.4s files are streams: read them with vga_nwstm_parse", (const char *)file);
            return f.code;
        }
        if (!std::memcmp(file, "RWAV", 4)) return rwav();
        if (!std::memcmp(file, "CWAV", 4) || !std::memcmp(file, "FWAV", 4) || !std::memcmp(file, "CSTP", 4) || !std::memcmp(file, "FSTP", 4))
            return bcf();
        return invalid(file[0] == 'R' ? "File has no RWAV header" : "File has no CSTM or FSTM header");
    }
};

inline int parse(const uint8_t *file, size_t size, vga_nwwav_info *out, Failure *fail)
{
    return Parser(file, size, out, fail).run();
}

// One channel's stored bytes (info->channel_bytes of them) from the image in host memory: a plain copy for wave files,
// the block de-interleave of the first region for prefetch files.
inline int read_channel(const uint8_t *file, size_t size, const vga_nwwav_info *I, int c, uint8_t *out)
{
    const int64_t n = I->channel_bytes, len = (int64_t)size;
    if (I->kind < VGA_NWWAV_CSTP) {
        if (I->audio_offset[c] < 0 || I->audio_offset[c] + n > len) return VGA_ERR_ARGUMENT;
        std::memcpy(out, file + I->audio_offset[c], (size_t)n);
        return VGA_OK;
    }
    const int64_t il = I->interleave_size, nch = I->channel_count, in = I->prefetch_size / std::max<int64_t>(nch, 1);
    if (il <= 0 || nch < 1 || n > in || I->prefetch_audio_offset < 0 || (int64_t)I->prefetch_audio_offset + I->prefetch_size > len) return VGA_ERR_ARGUMENT;
    const int64_t blocks = (in + il - 1) / il, last = in - (blocks - 1) * il;
    for (int64_t p = 0; p < n;) {
        const int64_t b = p / il, cur = b == blocks - 1 ? last : il, within = p - b * il, k = std::min(cur - within, n - p);
        std::memcpy(out + p, file + I->prefetch_audio_offset + b * il * nch + c * cur + within, (size_t)k);
        p += k;
    }
    return VGA_OK;
}

}  // namespace nwwav
}  // namespace vga
