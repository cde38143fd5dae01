// container_readers.hip -- the DSP, ADX and HCA file readers (Containers/Dsp/DspReader.cs, Containers/Adx/AdxReader.cs,
// Containers/Hca/HcaReader.cs).  Parsing is host code; the audio is taken out of nfiles equally shaped images per launch
// in HBM, in the row layouts the decoders take.  Keys and decryption stay with the caller, who composes them from the
// existing key-search and crypt calls exactly as the reference's ToAudioStream does.
#include "container_host.hpp"
#include "adx_span.hpp"
#include "hca_capi.hpp"
#include "hca_frame_crc.hpp"

using namespace vga;
using namespace vga::container;

// ---------------------------------------------------------------- device side
namespace vga {
namespace readers {

// ADX frames of 18 bytes, interleaved one frame per channel (AdxReader.ReadData :116-124 -> DeInterleave(audioSize,
// FrameSize, ChannelCount)): a workgroup takes a span of frame groups of one file through LDS with 16-byte vectors both
// ways.  The body is adx_span.hpp's, shared with the reader of a set of files (adx_files_kernels.hip).
constexpr int kAdxFrame = adxspan::kFrame;
constexpr int kAdxSpanBytes = adxspan::kSpanBytes;
constexpr int kAdxMaxFastChannels = adxspan::kMaxChannels;

__global__ __launch_bounds__(256) void adx18_deinterleave_kernel(const uint8_t *__restrict__ files, int64_t file_pitch,
                                                                 int audio_offset, int nch, int frame_count, int span_frames,
                                                                 uint8_t *__restrict__ dst, int64_t dst_pitch, int file0)
{
    __shared__ __align__(16) uint8_t lds[adxspan::kLdsBytes];
    const int f = file0 + blockIdx.y;
    adxspan::deinterleave_span(lds, files + (int64_t)f * file_pitch + audio_offset, nch, frame_count, blockIdx.x * span_frames, span_frames,
                               [&](int c) { return dst + (int64_t)(f * nch + c) * dst_pitch; });
}

// ReadHcaData (HcaReader.cs:123-138): one wave per frame copies it from the image to the frames layout and checks its
// CRC-16.  The copy is by output dword (the frames layout is 4-byte aligned; a dword belongs to the frame that holds its
// first byte), each from two aligned source dwords.  The CRC is the crypt pass's (hca_frame_crc.hpp): every lane reads
// its contiguous chunk of the frame from the image a second time, byte by byte (mostly cache hits: the copy has just
// loaded those lines).  A frame whose CRC does not match is counted, not rejected (:131-134).  Measured on the configs[3]
// shape: the copy alone takes 5.73 of the kernel's 6.24 ms, so the per-frame dword copy bounds it, not the CRC.
constexpr int kHcaWaves = 4;

__device__ __forceinline__ uint32_t load_u32_any(const uint8_t *s, int64_t i, int64_t n)
{
    // bytes s[i .. i+4) of an n-byte region at any alignment; bytes at or past n read as 0
    const uint8_t *p = s + i;
    const int off = (int)((uintptr_t)p & 3);
    const uint8_t *a = p - off;
    if (i + 4 <= n && off == 0) return *reinterpret_cast<const uint32_t *>(p);
    if (i + 4 <= n && a >= s && a + 8 <= s + n) {
        const uint32_t lo = reinterpret_cast<const uint32_t *>(a)[0], hi = reinterpret_cast<const uint32_t *>(a)[1];
        return __builtin_amdgcn_alignbyte(hi, lo, off);
    }
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) v |= (uint32_t)(i + k < n ? p[k] : 0) << (8 * k);
    return v;
}

__global__ __launch_bounds__(64 * kHcaWaves) void hca_read_frames_kernel(const uint8_t *__restrict__ files, int64_t file_pitch,
                                                                        int frames_offset, int frame_count, int frame_size,
                                                                        int64_t total_frames, uint8_t *__restrict__ frames,
                                                                        int64_t frames_pitch, const uint16_t *__restrict__ crc_pow,
                                                                        int *__restrict__ bad_crc)
{
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * kHcaWaves + (threadIdx.x >> 6);
    if (g >= total_frames) return;
    const int f = (int)(g / frame_count), k = (int)(g - (int64_t)f * frame_count);
    const uint8_t *src = files + (int64_t)f * file_pitch + frames_offset;       // the file's frames, back to back
    uint8_t *dst = frames + (int64_t)f * frames_pitch;
    const int64_t n = (int64_t)frame_count * frame_size;
    const int64_t b0 = (int64_t)k * frame_size, b1 = b0 + frame_size;
    // dwords whose first byte lies in [b0, b1); the last frame's also cover the 8 bytes of slack (zeros)
    const int64_t d0 = (b0 + 3) >> 2, d1 = k == frame_count - 1 ? (n + 8 + 3) >> 2 : (b1 + 3) >> 2;
    for (int64_t d = d0 + lane; d < d1; d += 64)
        reinterpret_cast<uint32_t *>(dst)[d] = load_u32_any(src, 4 * d, n);
    const int nbytes = frame_size - 2;
    const hca_crc::Chunk ch = hca_crc::lane_chunk(lane, nbytes);
    const uint8_t *a = src + b0;
    unsigned crc = 0;
    for (int i = ch.begin; i < ch.end; i++) crc = hca_crc::step(crc, a[i]);
    const unsigned part = hca_crc::wave_combine(crc, ch, nbytes, crc_pow);
    if (lane == 0 && bad_crc && part != ((unsigned)a[nbytes] << 8 | a[nbytes + 1])) atomicAdd(bad_crc + f, 1);
}

}  // namespace readers
}  // namespace vga

// ---------------------------------------------------------------- host side
namespace {

thread_local int g_adx_read_general = 0;     // vga_testing_adx_read_general_this_thread (its own file: the codec kernels'
                                             // headers, which stamp the committed profiles, stay untouched)

constexpr int kDspHeader = 0x60;             // DspReader.cs:13

}  // namespace

extern "C" {

int vga_testing_adx_read_general_this_thread(int on)
{
    const int old = g_adx_read_general;
    g_adx_read_general = on ? 1 : 0;
    return old;
}

// ---------------------------------------------------------------- DSP
int vga_dsp_parse(const uint8_t *file, size_t size, vga_dsp_info *out)
{
    if (!file || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    std::memset(out, 0, sizeof *out);
    vga_dsp_info &I = *out;
    ByteReader r{file, (int64_t)size, 0, true};
    I.sample_count = r.i32();                               // ReadHeader (:57-101)
    I.nibble_count = r.i32();
    I.sample_rate = r.i32();
    I.looping = r.i16() == 1;
    I.format = r.i16();
    I.start_addr = r.i32();
    I.end_addr = r.i32();
    I.cur_addr = r.i32();
    r.pos = 0x4a;
    int nch = r.i16();
    I.frames_per_interleave = r.i16();
    if (r.eof) return invalid("file ends inside the DSP header");
    nch = nch == 0 ? 1 : nch;                               // :71
    if (nch < 0) return invalid("negative channel count");
    if (nch > VGA_DSP_MAX_CHANNELS) {
        set_error("DSP file with %d channels: at most %d are read here", nch, VGA_DSP_MAX_CHANNELS);
        return VGA_ERR_INVALID_OP;
    }
    I.channel_count = nch;
    for (int i = 0; i < nch; i++) {
        r.pos = (int64_t)kDspHeader * i + 0x1c;
        for (int k = 0; k < 16; k++) I.coefs[i][k] = (int16_t)r.i16();
        I.gain[i] = (int16_t)r.i16();
        for (int k = 0; k < 3; k++) I.start_context[i][k] = (int16_t)r.i16();   // GcAdpcmContext(reader)
        for (int k = 0; k < 3; k++) I.loop_context[i][k] = (int16_t)r.i16();
    }
    if (r.eof) return invalid("file ends inside a channel header");
    I.loop_start = vga_gcadpcm_nibble_to_sample(I.start_addr);              // DspStructure.cs:68-72
    I.loop_end = vga_gcadpcm_nibble_to_sample(I.end_addr);
    if (I.sample_count < 0) return invalid("negative sample count");
    const int bytes = vga_gcadpcm_sample_count_to_byte_count(I.sample_count);
    if ((int64_t)size < kDspHeader + (int64_t)bytes) {      // :87-90 (one header, whatever the channel count)
        set_error("File doesn't contain enough data for %d samples", I.sample_count);
        return VGA_ERR_INVALID_DATA;
    }
    if (vga_gcadpcm_sample_count_to_nibble_count(I.sample_count) != I.nibble_count) return invalid("Sample count and nibble count do not match");
    if (I.format != 0) { set_error("File does not contain ADPCM audio. Specified format is %d", I.format); return VGA_ERR_INVALID_DATA; }
    I.audio_offset = kDspHeader * nch;                      // ReadFile (:25)
    I.adpcm_bytes = bytes;
    if (nch == 1) {                                         // ReadData (:103-115): ReadBytes, the length checked above
        I.interleave_size = 0;
        I.data_length = bytes;
        return VGA_OK;
    }
    I.interleave_size = I.frames_per_interleave * 8;        // FramesPerInterleave * BytesPerFrame
    if (I.interleave_size <= 0) return invalid("frames per interleave must be positive");   // DivideByRoundUp by 0
    const int64_t length = next_multiple(bytes, 8) * nch;
    if (length > 0x7FFFFFFF) return invalid("audio data length exceeds 2 GiB");
    I.data_length = (int)length;
    if ((int64_t)size - I.audio_offset < length) return invalid("Specified length is greater than the number of bytes remaining in the Stream");
    return VGA_OK;
}

int vga_dsp_read_device(const vga_dsp_info *I, const uint8_t *d_files, int64_t file_pitch, int nfiles, uint8_t *d_adpcm,
                        int64_t adpcm_pitch, void *stream)
{
    if (!I || nfiles < 0) { set_error("null / negative argument"); return VGA_ERR_ARGUMENT; }
    if (nfiles == 0 || I->adpcm_bytes == 0) return VGA_OK;
    const int nch = I->channel_count;
    if (nch < 1 || nch > VGA_DSP_MAX_CHANNELS || I->adpcm_bytes < 0 || I->data_length % nch ||
        (nch > 1 && (I->interleave_size <= 0 || I->data_length / nch < I->adpcm_bytes))) {
        set_error("info does not describe a DSP file");
        return VGA_ERR_ARGUMENT;
    }
    if (int rc = check_read_batch(d_files, d_adpcm, adpcm_pitch, I->adpcm_bytes, nfiles, file_pitch, (int64_t)I->audio_offset + I->data_length))
        return rc;
    const uint32_t out = (uint32_t)I->adpcm_bytes;
    // mono: the bytes verbatim, one block; several channels: DeInterleave(length, interleave, nch, bytes)
    const uint32_t in = nch == 1 ? out : (uint32_t)(I->data_length / nch), il = nch == 1 ? out : (uint32_t)I->interleave_size;
    return deinterleave_images(d_files, file_pitch, nfiles, I->audio_offset, nch, in, il, out, d_adpcm, adpcm_pitch, (hipStream_t)stream);
}

int vga_dsp_read(const uint8_t *file, size_t size, const vga_dsp_info *I, uint8_t *const *adpcm_out)
{
    if (!file || !I || !adpcm_out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    const int nch = I->channel_count;
    if (nch < 1 || nch > VGA_DSP_MAX_CHANNELS || (int64_t)I->audio_offset + I->data_length > (int64_t)size) {
        set_error("info does not describe this file");
        return VGA_ERR_ARGUMENT;
    }
    for (int c = 0; c < nch; c++)
        if (!adpcm_out[c]) { set_error("channel %d: null pointer", c); return VGA_ERR_ARGUMENT; }
    if (I->adpcm_bytes == 0) return VGA_OK;
    const size_t bytes = (size_t)I->audio_offset + (size_t)I->data_length;
    HostStage h;
    return h.read_rows(file, bytes, adpcm_out, nch, I->adpcm_bytes, 1, [&](const uint8_t *f, void *d, int64_t dp, hipStream_t s) {
        return vga_dsp_read_device(I, f, (int64_t)bytes, 1, static_cast<uint8_t *>(d), dp, s);
    });
}

// ---------------------------------------------------------------- ADX
int vga_adx_parse(const uint8_t *file, size_t size, vga_adx_file_info *out)
{
    if (!file || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    std::memset(out, 0, sizeof *out);
    vga_adx_file_info &I = *out;
    ByteReader r{file, (int64_t)size, 0, true};
    const int sig = r.u16();                                // ReadFile (:18-21)
    if (r.eof || sig != 0x8000) return invalid("File doesn't have ADX signature (0x80 0x00)");
    I.header_size = r.i16();                                // ReadHeader (:71-114)
    I.type = r.u8();
    I.frame_size = r.u8();
    I.bit_depth = r.u8();
    I.channel_count = r.u8();
    I.sample_rate = r.i32();
    I.sample_count = r.i32();
    I.highpass_frequency = r.i16();
    I.version = r.u8();
    I.revision = r.u8();
    if (r.eof) return invalid("file ends inside the ADX header");
    if (I.version >= 4) {
        r.pos += 4;
        for (int c = 0; c < I.channel_count; c++) {
            I.history[c][0] = (int16_t)r.i16();
            I.history[c][1] = (int16_t)r.i16();
        }
        if (I.channel_count == 1) r.pos += 4;               // room for two channels' histories at least
        if (r.eof) return invalid("file ends inside the history samples");
    }
    if (r.pos + 24 <= I.header_size) {
        I.inserted_samples = r.i16();
        I.loop_count = r.i16();
        if (I.loop_count > 0) {
            I.looping = 1;
            I.loop_type = r.i32();
            I.loop_start_sample = r.i32();
            I.loop_start_byte = r.i32();
            I.loop_end_sample = r.i32();
            I.loop_end_byte = r.i32();
        }
        if (r.eof) return invalid("file ends inside the loop block");
    }
    // ReadData (:116-124)
    I.audio_offset = I.header_size + 4;
    if (I.audio_offset < 0) return invalid("the audio offset (HeaderSize + 4) is negative");
    I.samples_per_frame = I.frame_size < 1 ? 0 : vga_adx_nibble_count_to_sample_count(I.frame_size * 2, I.frame_size);
    if (I.samples_per_frame <= 0) { set_error("frame size %d holds no samples", I.frame_size); return VGA_ERR_INVALID_DATA; }
    if (I.channel_count < 1) return invalid("the file has no channels");
    if (I.sample_count < 0) return invalid("negative sample count");
    I.frame_count = div_round_up(I.sample_count, I.samples_per_frame);
    const int64_t per = (int64_t)I.frame_count * I.frame_size, audio = per * I.channel_count;
    if (audio > 0x7FFFFFFF) return invalid("audio size exceeds 2 GiB");
    I.audio_bytes = (int)per;
    if ((int64_t)size - I.audio_offset < audio) return invalid("Specified length is greater than the number of bytes remaining in the Stream");
    return VGA_OK;
}

int vga_adx_read_device(const vga_adx_file_info *I, const uint8_t *d_files, int64_t file_pitch, int nfiles, uint8_t *d_audio,
                        int64_t audio_pitch, void *stream)
{
    if (!I || nfiles < 0) { set_error("null / negative argument"); return VGA_ERR_ARGUMENT; }
    if (nfiles == 0 || I->audio_bytes == 0) return VGA_OK;
    const int nch = I->channel_count, fs = I->frame_size;
    if (nch < 1 || nch > 255 || fs < 1 || I->frame_count < 0 || I->audio_bytes != I->frame_count * fs || I->audio_offset < 0) {
        set_error("info does not describe an ADX file");
        return VGA_ERR_ARGUMENT;
    }
    if (int rc = check_read_batch(d_files, d_audio, audio_pitch, I->audio_bytes, nfiles, file_pitch,
                                  (int64_t)I->audio_offset + (int64_t)I->audio_bytes * nch))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool fast = fs == readers::kAdxFrame && nch <= readers::kAdxMaxFastChannels && !g_adx_read_general &&
                      !(((uint64_t)(uintptr_t)d_audio | (uint64_t)audio_pitch) & 15);
    if (!fast) {
        const uint32_t row = (uint32_t)I->audio_bytes;
        return deinterleave_images(d_files, file_pitch, nfiles, I->audio_offset, nch, row, (uint32_t)fs, row, d_audio, audio_pitch, s);
    }
    const int span = readers::kAdxSpanBytes / (readers::kAdxFrame * nch) / 8 * 8;
    const unsigned spans = (unsigned)((I->frame_count + span - 1) / span);
    for (int f0 = 0; f0 < nfiles; f0 += container::kMaxGridY) {
        const int nf = std::min(nfiles - f0, container::kMaxGridY);
        hipLaunchKernelGGL(readers::adx18_deinterleave_kernel, dim3(spans, nf), dim3(256), 0, s, d_files, file_pitch, I->audio_offset,
                           nch, I->frame_count, span, d_audio, audio_pitch, f0);
        VGA_HIP_TRY(hipGetLastError());
    }
    return VGA_OK;
}

int vga_adx_read(const uint8_t *file, size_t size, const vga_adx_file_info *I, uint8_t *const *audio_out)
{
    if (!file || !I || !audio_out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    const int nch = I->channel_count;
    const int64_t bytes = (int64_t)I->audio_offset + (int64_t)I->audio_bytes * nch;
    if (nch < 1 || nch > 255 || I->audio_offset < 0 || bytes > (int64_t)size) { set_error("info does not describe this file"); return VGA_ERR_ARGUMENT; }
    for (int c = 0; c < nch; c++)
        if (!audio_out[c]) { set_error("channel %d: null pointer", c); return VGA_ERR_ARGUMENT; }
    if (I->audio_bytes == 0) return VGA_OK;
    HostStage h;
    return h.read_rows(file, (size_t)bytes, audio_out, nch, I->audio_bytes, 1, [&](const uint8_t *f, void *d, int64_t dp, hipStream_t s) {
        return vga_adx_read_device(I, f, bytes, 1, static_cast<uint8_t *>(d), dp, s);
    });
}

// ---------------------------------------------------------------- HCA
int vga_hca_parse(const uint8_t *file, size_t size, vga_hca_file_info *out)
{
    if (!file || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    std::memset(out, 0, sizeof *out);
    vga_hca_file_info &I = *out;
    vga_hca_info &H = I.hca;
    I.volume = 1.0f;                                        // HcaInfo.Volume's default (HcaInfo.cs:45)
    ByteReader r{file, (int64_t)size, 0, true};
    char id[5] = {0};
    auto chunk_id = [&]() {                                 // ReadChunkId (:226-236): top bits cleared
        if (!r.bytes(id, 4)) return false;
        for (int k = 0; k < 4; k++) id[k] &= 0x7f;
        return true;
    };
    const bool have_sig = chunk_id();                       // ReadHcaHeader (:59-121)
    I.version = r.i16();
    const int header_size = r.i16();
    if (!have_sig || r.eof) return invalid("file ends inside the HCA header");
    H.header_size = header_size;
    if (std::memcmp(id, "HCA\0", 4) != 0) return invalid("Not a valid HCA file");
    bool too_long_comment = false;
    while (r.pos < header_size) {
        if (!chunk_id()) return invalid("file ends inside a chunk id");
        if (!std::memcmp(id, "fmt\0", 4)) {                 // :140-149
            H.channel_count = r.u8();
            H.sample_rate = r.u8() << 16;
            H.sample_rate |= r.u16();
            H.frame_count = r.i32();
            H.inserted_samples = r.i16();
            H.appended_samples = r.i16();
            H.sample_count = (int)((uint32_t)H.frame_count * 1024u - (uint32_t)H.inserted_samples - (uint32_t)H.appended_samples);
        } else if (!std::memcmp(id, "comp", 4)) {           // :151-164
            H.frame_size = r.i16();
            H.min_resolution = r.u8();
            H.max_resolution = r.u8();
            H.track_count = r.u8();
            H.channel_config = r.u8();
            H.total_band_count = r.u8();
            H.base_band_count = r.u8();
            H.stereo_band_count = r.u8();
            H.bands_per_hfr_group = r.u8();
            I.reserved1 = r.u8();
            I.reserved2 = r.u8();
        } else if (!std::memcmp(id, "dec\0", 4)) {          // :166-187
            H.frame_size = r.i16();
            H.min_resolution = r.u8();
            H.max_resolution = r.u8();
            H.total_band_count = r.u8() + 1;
            H.base_band_count = r.u8() + 1;
            const int a = r.u8();
            H.track_count = a >> 4;
            H.channel_config = a & 0xf;
            I.dec_stereo_type = r.u8();
            if (I.dec_stereo_type == 0) H.base_band_count = H.total_band_count;
            else H.stereo_band_count = H.total_band_count - H.base_band_count;
        } else if (!std::memcmp(id, "loop", 4)) {           // :189-197
            H.looping = 1;
            H.loop_start_frame = r.i32();
            H.loop_end_frame = r.i32();
            H.pre_loop_samples = r.i16();
            H.post_loop_samples = r.i16();
            const int loop_end = (int)((uint32_t)(H.loop_end_frame + 1) * 1024u - (uint32_t)H.post_loop_samples - (uint32_t)H.inserted_samples);
            H.sample_count = std::min(H.sample_count, loop_end);       // HcaInfo.LoopEndSample (HcaInfo.cs:36)
        } else if (!std::memcmp(id, "ath\0", 4)) {          // :199-202
            H.use_ath_curve = r.i16() == 1;
            I.has_ath_chunk = 1;
        } else if (!std::memcmp(id, "ciph", 4)) {           // :210-213
            I.encryption_type = r.i16();
        } else if (!std::memcmp(id, "rva\0", 4)) {          // :215-218 (ReadSingle, big-endian)
            const uint32_t bits = (uint32_t)r.i32();
            std::memcpy(&I.volume, &bits, 4);
        } else if (!std::memcmp(id, "vbr\0", 4)) {          // :204-208
            I.vbr_max_frame_size = r.i16();
            I.vbr_noise_level = r.i16();
        } else if (!std::memcmp(id, "comm", 4)) {           // :220-224, then Position = HeaderSize (:104-107)
            r.pos++;
            // ReadUTF8Z (Utilities/Extensions.cs:60-73): up to the first byte below 2, or to the end of the stream, where
            // the reference drops the last byte
            const int64_t start = r.pos;
            int64_t k = start;
            while (k < r.len && file[k] > 1) k++;
            const int64_t n = k < r.len ? k - start : r.len - start - 1;
            if (n < 0) return invalid("file ends inside the comment");
            if (n > 255) too_long_comment = true;
            else std::memcpy(I.comment, file + start, (size_t)n);
            I.has_comment = 1;
            H.comment_length = (int)std::min<int64_t>(n, 255);
            r.pos = header_size;
        } else if (!std::memcmp(id, "pad\0", 4)) {          // :108-110
            r.pos = header_size;
        } else {
            set_error("Chunk %.4s is not supported.", id);  // NotSupportedException (:111-112)
            return VGA_ERR_INVALID_OP;
        }
        if (r.eof) { set_error("file ends inside the %.4s chunk", id); return VGA_ERR_INVALID_DATA; }
    }
    if (I.version < 0x0200 && !I.has_ath_chunk) H.use_ath_curve = 1;    // :116
    if (H.track_count < 1) H.track_count = 1;                            // :118
    if (H.bands_per_hfr_group > 0) {                                     // CalculateHfrValues (HcaInfo.cs:50-56)
        H.hfr_band_count = H.total_band_count - H.base_band_count - H.stereo_band_count;
        H.hfr_group_count = div_round_up(H.hfr_band_count, H.bands_per_hfr_group);
    }
    // ReadFile (:27): Position = HeaderSize; ReadHcaData (:123-138): FrameCount frames of FrameSize bytes
    if (header_size < 0) return invalid("negative header size");
    I.frames_offset = header_size;
    if (H.frame_count < 0) return invalid("negative frame count");
    if (H.frame_count > 0 && H.frame_size < 2) return invalid("frames shorter than their CRC");
    if ((int64_t)size - header_size < (int64_t)H.frame_count * std::max(H.frame_size, 0)) return invalid("file ends inside the frames");
    if (too_long_comment) { set_error("comment longer than 255 bytes"); return VGA_ERR_INVALID_OP; }
    // A negative stereo band count (dec chunk, base > total) or HFR group count (comp bands past the total) decodes in the
    // reference and is kept; a secondary channel's base band count above 128 is refused by the decoder
    // (VGA_ERR_OUT_OF_RANGE, where the reference throws), as are stereo bands with more than one track.
    if (H.channel_count < 1 || H.channel_count > 8 || H.frame_size < 8 || H.frame_size > 0xFFFF || H.total_band_count > 128 ||
        H.base_band_count < 0 || H.base_band_count + H.stereo_band_count > 128 || H.hfr_group_count > 8) {
        set_error("HCA stream the decoder cannot take (channels %d, frame size %d, bands %d/%d/%d, hfr groups %d)", H.channel_count,
                  H.frame_size, H.total_band_count, H.base_band_count, H.stereo_band_count, H.hfr_group_count);
        return VGA_ERR_INVALID_OP;
    }
    return VGA_OK;
}

int vga_hca_read_device(const vga_hca_file_info *I, const uint8_t *d_files, int64_t file_pitch, int nfiles, uint8_t *d_frames,
                        int64_t frames_pitch, int *d_bad_crc, void *stream)
{
    if (!I || nfiles < 0) { set_error("null / negative argument"); return VGA_ERR_ARGUMENT; }
    const vga_hca_info &H = I->hca;
    hipStream_t s = (hipStream_t)stream;
    if (nfiles == 0) return VGA_OK;
    if (H.frame_count < 0 || H.frame_size < 8 || H.frame_size > 0xFFFF || I->frames_offset < 0) { set_error("info does not describe an HCA file"); return VGA_ERR_ARGUMENT; }
    const int64_t bytes = (int64_t)H.frame_count * H.frame_size;
    if (!d_files || !d_frames || frames_pitch < bytes + 8 || (frames_pitch & 3) || ((uintptr_t)d_frames & 3)) {
        set_error("null pointer / frames pitch not a multiple of 4 of at least frame_count * frame_size + 8 (%lld)", (long long)(bytes + 8));
        return VGA_ERR_ARGUMENT;
    }
    if (nfiles > 1 && file_pitch < I->frames_offset + bytes) { set_error("file pitch smaller than the file"); return VGA_ERR_ARGUMENT; }
    if (d_bad_crc) VGA_HIP_TRY(hipMemsetAsync(d_bad_crc, 0, sizeof(int) * (size_t)nfiles, s));
    if (H.frame_count == 0) {                               // only the slack to clear
        for (int f = 0; f < nfiles; f++) VGA_HIP_TRY(hipMemsetAsync(d_frames + f * frames_pitch, 0, 8, s));
        return VGA_OK;
    }
    static_assert(hca_crc::kPowEntries > 0xFFFF - 2, "wave_combine reads crc_pow[nbytes - end] for frames of up to 0xFFFF bytes");
    const uint16_t *pow = nullptr;
    if (int rc = hca::crc_pow_table(&pow)) return rc;
    const int64_t total = (int64_t)nfiles * H.frame_count;
    const int64_t blocks = (total + readers::kHcaWaves - 1) / readers::kHcaWaves;
    if (blocks > 0x7FFFFFFF) { set_error("too many frames for one launch"); return VGA_ERR_ARGUMENT; }
    hipLaunchKernelGGL(readers::hca_read_frames_kernel, dim3((unsigned)blocks), dim3(64 * readers::kHcaWaves), 0, s, d_files, file_pitch,
                       I->frames_offset, H.frame_count, H.frame_size, total, d_frames, frames_pitch, pow, d_bad_crc);
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

int vga_hca_read(const uint8_t *file, size_t size, const vga_hca_file_info *I, uint8_t *frames_out, int *bad_crc_out)
{
    if (!file || !I || !frames_out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    const vga_hca_info &H = I->hca;
    const int64_t bytes = (int64_t)H.frame_count * std::max(H.frame_size, 0);
    if (H.frame_count < 0 || I->frames_offset < 0 || I->frames_offset + bytes > (int64_t)size) { set_error("info does not describe this file"); return VGA_ERR_ARGUMENT; }
    if (bad_crc_out) *bad_crc_out = 0;
    if (bytes == 0) return VGA_OK;
    HostStage h;
    const uint8_t *d_file = nullptr;
    void *d_out = nullptr, *d_bad = nullptr;
    const int64_t pitch = hca::frames_pitch_for(H);
    int bad = 0;
    if (int rc = h.open()) return rc;
    if (int rc = h.image(file, (size_t)(I->frames_offset + bytes), &d_file)) return rc;
    if (int rc = h.alloc((size_t)pitch, &d_out)) return rc;
    if (int rc = h.alloc(sizeof(int), &d_bad)) return rc;
    if (int rc = vga_hca_read_device(I, d_file, I->frames_offset + bytes, 1, static_cast<uint8_t *>(d_out), pitch, static_cast<int *>(d_bad),
                                     h.stream()))
        return rc;
    if (int rc = h.back(frames_out, d_out, (size_t)bytes)) return rc;
    if (int rc = h.back(&bad, d_bad, sizeof bad)) return rc;
    if (int rc = h.finish()) return rc;
    if (bad_crc_out) *bad_crc_out = bad;
    return VGA_OK;
}

}  // extern "C"
