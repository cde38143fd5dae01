// capi_containers.hip -- C ABI of the ADX and HCA container writers (DSP lives next to the
// GC-ADPCM entry points).  Images are assembled in HBM; the host-pointer forms stage through the device.
#include "container_host.hpp"
#include "wave_file_host.hpp"

#include <vector>

using namespace vga;
using namespace vga::container;

namespace {

// Utilities/Crc16.cs:12-18 with polynomial 0x8005 (HcaWriter.cs:18), MSB first, initial value 0
uint16_t crc16(const uint8_t *data, int size)
{
    uint16_t crc = 0;
    for (int i = 0; i < size; i++) {
        crc ^= (uint16_t)(data[i] << 8);
        for (int k = 0; k < 8; k++) crc = (crc & 0x8000) ? (uint16_t)((crc << 1) ^ 0x8005) : (uint16_t)(crc << 1);
    }
    return crc;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- ADX (Containers/Adx/AdxWriter.cs:14-139)
int vga_adx_file_layout_for(const vga_adx_file_params *p, int nch, vga_adx_file_layout *L)
{
    return adx_file_layout(p, nch, L);                      // (adx_file_host.hpp: one copy for this call and for sets of files)
}

int vga_adx_write_device(const uint8_t *d_audio, int64_t audio_pitch, int audio_len, const int16_t *d_history, int nch,
                         const vga_adx_file_params *p, uint8_t *d_file, void *stream)
{
    vga_adx_file_layout L;
    container::AdxHeaderArgs a;
    if (audio_len < 0 || !d_file || (audio_len > 0 && !d_audio)) { set_error("null / negative argument"); return VGA_ERR_ARGUMENT; }
    if (int rc = adx_args(p, nch, audio_len, &L, &a)) return rc;
    if (p->version == 4 && !d_history) { set_error("version 4 headers carry the channel histories"); return VGA_ERR_ARGUMENT; }
    if (audio_len > 0 && audio_pitch < audio_len) { set_error("audio pitch %lld < length %d", (long long)audio_pitch, audio_len); return VGA_ERR_ARGUMENT; }
    hipStream_t s = (hipStream_t)stream;
    VGA_HIP_TRY(hipMemsetAsync(d_file, 0, (size_t)L.file_size, s));
    if (int rc = container::launch_adx_header(a, d_history, d_file, s)) return rc;
    // WriteData (:119-131): frames of all channels in turn, FrameCount frames each
    if (int rc = container::launch_interleave(d_audio, audio_pitch, audio_len, nch, p->frame_size, L.frame_count * p->frame_size,
                                              d_file + L.audio_offset, s))
        return rc;
    return container::launch_adx_footer(a, d_file, s);
}

int vga_adx_write(const uint8_t *const *audio, int audio_len, const int16_t *history, int nch, const vga_adx_file_params *p,
                  uint8_t *file_out)
{
    vga_adx_file_layout L;
    container::AdxHeaderArgs a;
    if (audio_len < 0 || !file_out || !audio) { set_error("null / negative argument"); return VGA_ERR_ARGUMENT; }
    if (int rc = adx_args(p, nch, audio_len, &L, &a)) return rc;
    for (int c = 0; c < nch; c++)
        if (audio_len > 0 && !audio[c]) { set_error("audio[%d] is null", c); return VGA_ERR_ARGUMENT; }
    if (p->version == 4 && !history) { set_error("version 4 headers carry the channel histories"); return VGA_ERR_ARGUMENT; }
    HostStage h;
    uint8_t *d_audio = nullptr;
    const int16_t *d_hist = nullptr;
    int64_t pitch = 0;
    if (int rc = h.open()) return rc;
    if (int rc = h.rows(audio, nch, audio_len, &d_audio, &pitch)) return rc;
    if (int rc = h.table(history, (size_t)nch, &d_hist)) return rc;
    return h.write_image(file_out, (size_t)L.file_size, [&](uint8_t *d_file, hipStream_t s) {
        return vga_adx_write_device(d_audio, pitch, audio_len, d_hist, nch, p, d_file, s);
    });
}

// ---------------------------------------------------------------- HCA (Containers/Hca/HcaWriter.cs:12-185)
int vga_hca_file_size(const vga_hca_info *h)
{
    if (!h) { set_error("null HcaInfo"); return VGA_ERR_ARGUMENT; }
    const int64_t n = (int64_t)h->header_size + (int64_t)h->frame_size * h->frame_count;                // :22
    if (h->header_size < 0 || h->frame_size < 0 || h->frame_count < 0 || n > 0x7FFFFFFF) {
        set_error("HCA file size out of range");
        return VGA_ERR_OUT_OF_RANGE;
    }
    return (int)n;
}

// WriteHeader (:57-82): the chunks, zero padding, CRC-16 of everything before it.  header_out: h->header_size bytes.
int vga_hca_file_header(const vga_hca_info *h, const char *comment, float volume, int encryption_type, int encrypted_ids,
                        uint8_t *header_out)
{
    if (!h || !header_out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (h->header_size < 8 || h->header_size > 0x7FFF) { set_error("HCA header size %d out of range", h->header_size); return VGA_ERR_OUT_OF_RANGE; }
    std::memset(header_out, 0, (size_t)h->header_size);
    ByteWriter c{header_out, h->header_size - 2, 0, true};
    // WriteChunkId (:158-171): with an encryption key every non-zero id byte gets its top bit set
    auto chunk = [&](const char *id, int n) { for (int i = 0; i < n; i++) c.put8(id[i] && encrypted_ids ? (id[i] | 0x80) : id[i]); };
    chunk("HCA\0", 4);                                      // :84-89
    c.put16(0x0200);
    c.put16(h->header_size);
    chunk("fmt\0", 4);                                     // :91-103
    c.put8(h->channel_count);
    c.put8(h->sample_rate >> 16);
    c.put16(h->sample_rate);
    c.put32(h->frame_count);
    c.put16(h->inserted_samples);
    c.put16(h->appended_samples);
    chunk("comp", 4);                                      // :105-118
    c.put16(h->frame_size);
    c.put8(h->min_resolution);
    c.put8(h->max_resolution);
    c.put8(h->track_count);
    c.put8(h->channel_config);
    c.put8(h->total_band_count);
    c.put8(h->base_band_count);
    c.put8(h->stereo_band_count);
    c.put8(h->bands_per_hfr_group);
    c.put16(0);
    if (h->looping) {                                       // :120-129
        chunk("loop", 4);
        c.put32(h->loop_start_frame);
        c.put32(h->loop_end_frame);
        c.put16(h->pre_loop_samples);
        c.put16(h->post_loop_samples);
    }
    chunk("ciph", 4);                                      // :131-135
    c.put16(encryption_type);
    if (volume != 1.0f) {                                   // :137-146
        uint32_t bits;
        std::memcpy(&bits, &volume, 4);
        chunk("rva\0", 4);
        c.put32((int)bits);
    }
    bool blank = true;                                      // string.IsNullOrWhiteSpace (:66)
    if (comment)
        for (const char *s = comment; *s; s++)
            if (!(*s == ' ' || (*s >= 9 && *s <= 13))) blank = false;
    if (blank) {
        chunk("pad", 3);                                   // :154-157: three bytes
    } else {
        chunk("comm\0", 5);                                // :148-152
        c.bytes(comment, (int)std::strlen(comment) + 1);
    }
    if (c.overflow) {
        set_error("HCA header chunks (%d bytes) do not fit HeaderSize %d", (int)c.pos, h->header_size);
        return VGA_ERR_INVALID_OP;
    }
    const uint16_t crc = crc16(header_out, h->header_size - 2);   // :75-79
    header_out[h->header_size - 2] = (uint8_t)(crc >> 8);
    header_out[h->header_size - 1] = (uint8_t)crc;
    return VGA_OK;
}

// nstreams equally shaped streams (one HcaInfo): image s = header + stream s's frames, file_pitch bytes apart
int vga_hca_write_device(const vga_hca_info *h, const uint8_t *d_frames, int64_t frames_pitch, int nstreams, const char *comment,
                         float volume, int encryption_type, int encrypted_ids, uint8_t *d_files, int64_t file_pitch, void *stream)
{
    const int size = vga_hca_file_size(h);
    if (size < 0) return size;
    if (nstreams < 0 || !d_files || (!d_frames && h->frame_count > 0)) { set_error("null / negative argument"); return VGA_ERR_ARGUMENT; }
    const int64_t audio = (int64_t)h->frame_size * h->frame_count;
    if (file_pitch < size || frames_pitch < audio) { set_error("pitch smaller than the data"); return VGA_ERR_ARGUMENT; }
    if (nstreams == 0) return VGA_OK;
    std::vector<uint8_t> header((size_t)h->header_size);
    if (int rc = vga_hca_file_header(h, comment, volume, encryption_type, encrypted_ids, header.data())) return rc;
    hipStream_t s = (hipStream_t)stream;
    // the header goes into image 0 as kernel arguments, the other images copy it on the device
    if (int rc = container::upload_bytes(header.data(), h->header_size, d_files, s)) return rc;
    if (nstreams > 1)
        if (int rc = container::launch_replicate(d_files, h->header_size, d_files + file_pitch, file_pitch, nstreams - 1, s)) return rc;
    if (audio > 0)                                          // WriteData (:173-179): the frames, back to back
        VGA_HIP_TRY(hipMemcpy2DAsync(d_files + h->header_size, (size_t)file_pitch, d_frames, (size_t)frames_pitch, (size_t)audio,
                                     (size_t)nstreams, hipMemcpyDeviceToDevice, s));
    return VGA_OK;
}

// One stream held in host memory (CriHcaFormat.AudioData flattened): header + frames.  No device work is needed
// for a 96-byte header and a copy, so this form stays on the host.
int vga_hca_write(const vga_hca_info *h, const uint8_t *frames, const char *comment, float volume, int encryption_type,
                  int encrypted_ids, uint8_t *file_out)
{
    const int size = vga_hca_file_size(h);
    if (size < 0) return size;
    if (!file_out || (!frames && h->frame_count > 0)) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (int rc = vga_hca_file_header(h, comment, volume, encryption_type, encrypted_ids, file_out)) return rc;
    std::memcpy(file_out + h->header_size, frames, (size_t)h->frame_size * h->frame_count);
    return VGA_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- WAVE, 16-bit PCM
// The writers' size and header math and the readers' checks are wave_file_host.hpp's: one copy for these calls and for sets
// of files (include/vgaudio_hip_files/wave_files.h).
extern "C" {

// WaveReader.ReadFile + ToAudioStream up to the audio itself (WaveReader.cs:13-68, RiffParser.cs:36-78): host only.
int vga_wave_parse(const uint8_t *file, int64_t file_len, vga_wave_info *w)
{
    if (!file || !w || file_len < 0) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    std::memset(w, 0, sizeof *w);
    ByteReader r{file, file_len};
    char id[4], type[4];
    if (!r.bytes(id, 4)) return invalid("file ends inside the RIFF header");
    const int64_t riff_size = r.i32();
    if (!r.bytes(type, 4) || r.eof) return invalid("file ends inside the RIFF header");
    if (std::memcmp(id, "RIFF", 4) != 0) return invalid("Not a valid RIFF file");                    // RiffChunk.cs:21-24
    const int64_t riff_end = 8 + riff_size;                                                            // RiffParser.cs:44-45
    bool have_fmt = false, have_data = false, have_smpl = false, have_ext = false, ext_pcm = false;
    int format_tag = 0, block_align = 0, smpl_loops = 0, smpl_start = 0, smpl_end = 0;
    while (r.pos + 8 < riff_end) {
        if (!r.bytes(id, 4)) return invalid("RIFF size runs past the end of the file");
        const int64_t size = r.i32();
        if (r.eof) return invalid("file ends inside a chunk header");
        if (size < 0) return invalid("negative chunk size");
        const int64_t body = r.pos;
        if (!std::memcmp(id, "fmt ", 4)) {                                                             // WaveFmtChunk.cs:16-34
            format_tag = r.u16();
            w->channel_count = r.i16();
            w->sample_rate = r.i32();
            r.i32();
            block_align = r.i16();
            w->bits_per_sample = r.i16();
            have_fmt = true;
            have_ext = false;
            if (format_tag == 0xFFFE) {                                                                // WaveFormatExtensible.cs:20-27
                const int64_t ext_body = r.pos + 2;
                const int ext_size = r.i16();
                r.i16();
                r.i32();
                if (r.has(16)) { ext_pcm = std::memcmp(file + r.pos, kWaveSubtypePcm, 16) == 0; r.pos += 16; }
                have_ext = true;
                r.skip_to(ext_body + ext_size);
            }
        } else if (!std::memcmp(id, "data", 4)) {                                                      // WaveDataChunk.cs:9-15
            have_data = true;
            w->data_offset = r.pos;
            w->data_size_declared = (int)size;
            w->data_size = (int)std::min<int64_t>(size, file_len - r.pos);
            r.pos += w->data_size;
        } else if (!std::memcmp(id, "smpl", 4)) {                                                      // WaveSmplChunk.cs:19-45
            for (int i = 0; i < 7; i++) r.i32();
            smpl_loops = r.i32();
            r.i32();
            if (smpl_loops < 0) return invalid("negative loop count in the smpl chunk");
            for (int i = 0; i < smpl_loops && !r.eof; i++) {
                r.i32(); r.i32();
                const int start = r.i32(), end = r.i32();
                r.i32(); r.i32();
                if (i == 0) { smpl_start = start; smpl_end = end; }
            }
            have_smpl = true;
        } else if (!std::memcmp(id, "fact", 4)) {
            r.i32();
        }
        if (r.eof) return invalid("file ends inside a chunk");
        r.skip_to(body + size);
        r.pos = body + size + ((body + size) & 1);                                                     // chunks are 2-byte aligned
    }
    // ValidateWaveFile (WaveReader.cs:70-98)
    if (std::memcmp(type, "WAVE", 4) != 0) return invalid("Not a valid WAVE file");
    if (!have_fmt) return invalid("File must have a valid fmt chunk");
    if (!have_data) return invalid("File must have a valid data chunk");
    const int bytes_per_sample = (w->bits_per_sample + 7) / 8;
    if (format_tag != 1 && format_tag != 0xFFFE) return invalid("Must contain PCM data. Has unsupported format");
    if (w->bits_per_sample != 16 && w->bits_per_sample != 8) return invalid("Must have 8 or 16 bits per sample");
    if (w->channel_count == 0) return invalid("Channel count must not be zero");
    if (block_align != bytes_per_sample * w->channel_count) return invalid("File has invalid block alignment");
    if (have_ext && !ext_pcm) return invalid("Must contain PCM data. Has unsupported SubFormat");
    if (w->channel_count < 0) return invalid("negative channel count");
    w->sample_count_declared = w->data_size_declared / bytes_per_sample / w->channel_count;            // :27
    w->sample_count = w->data_size / bytes_per_sample / w->channel_count;                              // Interleave.cs:190
    if (have_smpl && smpl_loops > 0) {                                                                 // :32-37
        w->loop_start = smpl_start;
        w->loop_end = smpl_end;
        w->looping = smpl_end > smpl_start;
    }
    if (w->looping) {                                                                                  // AudioFormatBaseBuilder.cs:30-43
        if (w->loop_start < 0 || w->loop_start > w->sample_count || w->loop_end < 0 || w->loop_end > w->sample_count) {
            set_error("Loop points must be less than the number of samples and non-negative.");
            return VGA_ERR_OUT_OF_RANGE;
        }
    } else {
        w->loop_start = w->loop_end = 0;
    }
    return VGA_OK;
}

// InterleavedByteToShort (Interleave.cs:188-207) on the device: d_data = the data chunk's bytes (any alignment)
int vga_wave_deinterleave_pcm16_device(const uint8_t *d_data, int sample_count, int nch, int16_t *d_pcm, int64_t pcm_pitch,
                                       void *stream)
{
    if (sample_count < 0 || nch < 0) { set_error("negative size"); return VGA_ERR_ARGUMENT; }
    if (sample_count == 0 || nch == 0) return VGA_OK;
    if (!d_data || !d_pcm || pcm_pitch < sample_count) { set_error("null pointer / pitch < sample count"); return VGA_ERR_ARGUMENT; }
    return container::launch_pcm16_deinterleave(d_data, sample_count, nch, d_pcm, pcm_pitch, (hipStream_t)stream);
}

// WaveReader for a 16-bit file in host memory: pcm_out[c] = info->sample_count shorts
int vga_wave_read_pcm16(const uint8_t *file, int64_t file_len, const vga_wave_info *w, int16_t *const *pcm_out)
{
    if (!file || !w || !pcm_out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (int rc = wave_read16_check(w, file_len)) return rc;
    const int64_t bytes = (int64_t)w->sample_count * w->channel_count * 2;
    if (bytes == 0) return VGA_OK;
    for (int c = 0; c < w->channel_count; c++)
        if (!pcm_out[c]) { set_error("pcm_out[%d] is null", c); return VGA_ERR_ARGUMENT; }
    HostStage h;
    return h.read_rows(file + w->data_offset, (size_t)bytes, pcm_out, w->channel_count, w->sample_count, 2,
                       [&](const uint8_t *d_data, void *d, int64_t dp, hipStream_t s) {
                           return container::launch_pcm16_deinterleave(d_data, w->sample_count, w->channel_count, static_cast<int16_t *>(d), dp, s);
                       });
}

// WaveWriter.FileSize (WaveWriter.cs:25-30), 16-bit
int64_t vga_wave_file_size(const vga_wave_params *p, int nch)
{
    return wave_file_size(p, nch, 2);
}

int vga_wave_write_pcm16_device(const int16_t *d_pcm, int64_t pcm_pitch, int nch, const vga_wave_params *p, uint8_t *d_file,
                                void *stream)
{
    const int64_t size = vga_wave_file_size(p, nch);
    if (size < 0) return (int)size;
    if (!d_file || (p->sample_count > 0 && (!d_pcm || pcm_pitch < p->sample_count))) { set_error("null pointer / pitch < sample count"); return VGA_ERR_ARGUMENT; }
    uint8_t header[160];
    const int hs = wave_header_size(p, nch);
    wave_header(p, nch, size, header);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = container::upload_bytes(header, hs, d_file, s)) return rc;
    return container::launch_pcm16_interleave(d_pcm, pcm_pitch, p->sample_count, nch, d_file + hs, s);
}

int vga_wave_write_pcm16(const int16_t *const *pcm, int nch, const vga_wave_params *p, uint8_t *file_out)
{
    const int64_t size = vga_wave_file_size(p, nch);
    if (size < 0) return (int)size;
    if (!pcm || !file_out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (p->sample_count == 0) { wave_header(p, nch, size, file_out); return VGA_OK; }
    HostStage h;
    int16_t *d_in = nullptr;
    int64_t pitch = 0;
    if (int rc = h.open()) return rc;
    for (int c = 0; c < nch; c++)
        if (!pcm[c]) { set_error("pcm[%d] is null", c); return VGA_ERR_ARGUMENT; }
    if (int rc = h.rows(pcm, nch, p->sample_count, &d_in, &pitch)) return rc;
    return h.write_image(file_out, (size_t)size, [&](uint8_t *d_file, hipStream_t s) {
        return vga_wave_write_pcm16_device(d_in, pitch, nch, p, d_file, s);
    });
}

}  // extern "C"

// ---------------------------------------------------------------- WAVE, 8-bit (WaveWriter.cs with WaveCodec.Pcm8Bit)
namespace {

int elem_size(int kind) { return kind == VGA_SAMPLES_S16 ? 2 : 1; }

}  // namespace

extern "C" {

// WaveWriter.FileSize (WaveWriter.cs:25-30) with BytesPerSample 1: DataChunkSize = nch * samples, odd sizes included
int64_t vga_wave_pcm8_file_size(const vga_wave_params *p, int nch)
{
    return wave_file_size(p, nch, 1);
}

int vga_wave_write_pcm8_device(const void *d_samples, int sample_kind, int64_t pitch, int nch, const vga_wave_params *p,
                               uint8_t *d_file, void *stream)
{
    const int64_t size = vga_wave_pcm8_file_size(p, nch);
    if (size < 0) return (int)size;
    if (int rc = check_sample_kind(sample_kind)) return rc;
    if (!d_file || (p->sample_count > 0 && (!d_samples || pitch < p->sample_count))) { set_error("null pointer / pitch < sample count"); return VGA_ERR_ARGUMENT; }
    uint8_t header[160];
    const int hs = wave_header_size(p, nch);
    wave_header(p, nch, size, header, 1);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = container::upload_bytes(header, hs, d_file, s)) return rc;
    return container::launch_pcm8_interleave(d_samples, sample_kind == VGA_SAMPLES_S16, pitch, p->sample_count, nch, d_file + hs, s);
}

int vga_wave_write_pcm8(const void *const *samples, int sample_kind, int nch, const vga_wave_params *p, uint8_t *file_out)
{
    const int64_t size = vga_wave_pcm8_file_size(p, nch);
    if (size < 0) return (int)size;
    if (int rc = check_sample_kind(sample_kind)) return rc;
    if (!samples || !file_out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (p->sample_count == 0) { wave_header(p, nch, size, file_out, 1); return VGA_OK; }
    for (int c = 0; c < nch; c++)
        if (!samples[c]) { set_error("samples[%d] is null", c); return VGA_ERR_ARGUMENT; }
    HostStage h;
    void *d_in = nullptr;
    int64_t pitch = 0;
    if (int rc = h.open()) return rc;
    if (int rc = h.rows(samples, nch, p->sample_count, elem_size(sample_kind), &d_in, &pitch)) return rc;
    return h.write_image(file_out, (size_t)size, [&](uint8_t *d_file, hipStream_t s) {
        return vga_wave_write_pcm8_device(d_in, sample_kind, pitch, nch, p, d_file, s);
    });
}

// DeInterleave(1, nch) (WaveReader.cs:47) on the device, through Pcm8Codec.Decode for int16 rows
int vga_wave_deinterleave_pcm8_device(const uint8_t *d_data, int sample_count, int nch, void *d_samples, int sample_kind,
                                      int64_t pitch, void *stream)
{
    if (sample_count < 0 || nch < 0) { set_error("negative size"); return VGA_ERR_ARGUMENT; }
    if (int rc = check_sample_kind(sample_kind)) return rc;
    if (sample_count == 0 || nch == 0) return VGA_OK;
    if (!d_data || !d_samples || pitch < sample_count) { set_error("null pointer / pitch < sample count"); return VGA_ERR_ARGUMENT; }
    return container::launch_pcm8_deinterleave(d_data, sample_count, nch, d_samples, sample_kind == VGA_SAMPLES_S16, pitch,
                                               (hipStream_t)stream);
}

// WaveReader for an 8-bit file in host memory: out[c] = info->sample_count elements of sample_kind
int vga_wave_read_pcm8(const uint8_t *file, int64_t file_len, const vga_wave_info *w, void *const *out, int sample_kind)
{
    if (!file || !w || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (int rc = check_sample_kind(sample_kind)) return rc;
    if (int rc = wave_read8_check(w, file_len)) return rc;
    const int64_t bytes = (int64_t)w->sample_count * w->channel_count;
    for (int c = 0; c < w->channel_count; c++)
        if (!out[c]) { set_error("out[%d] is null", c); return VGA_ERR_ARGUMENT; }
    if (bytes == 0) return VGA_OK;
    HostStage h;
    return h.read_rows(file + w->data_offset, (size_t)bytes, out, w->channel_count, w->sample_count, elem_size(sample_kind),
                       [&](const uint8_t *d_data, void *d, int64_t dp, hipStream_t s) {
                           return vga_wave_deinterleave_pcm8_device(d_data, w->sample_count, w->channel_count, d, sample_kind, dp, s);
                       });
}

}  // extern "C"
