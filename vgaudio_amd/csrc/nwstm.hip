// nwstm.hip -- NintendoWare streams for GC-ADPCM: BRSTM (Containers/NintendoWare/BrstmWriter.cs, BrstmReader.cs) and
// BCSTM / BFSTM (BCFstmWriter.cs, BCFstmReader.cs).  Size math and parsing are host code; the images are assembled
// and taken apart in HBM, nfiles equally shaped files per launch.  Everything on the device is byte movement:
// HBM-bound, every byte of an image read or written once.
#include "container_host.hpp"
#include "nw_header_body.hpp"
#include "pcm_kernels.hpp"

using namespace vga;
using namespace vga::container;
using namespace vga::nw;                                    // the formats' constants, the size math (nw_host.hpp)

// ---------------------------------------------------------------- device side
namespace vga {
namespace nwstm {

using nw::TrackK;

// everything the header kernel writes that is not per channel; passed by value (< 4 KiB of kernel arguments)
struct HeaderArgs : nw::HeaderGeom {
    TrackK tracks[VGA_NW_MAX_TRACKS];
};

// equally shaped files: file f's channel c is row f * nch + c of the pitched inputs, the tracks are the launch's
struct PitchedRows {
    const HeaderArgs &a;
    const uint8_t *adpcm;
    int64_t adpcm_pitch;
    int adpcm_len, row0;
    __device__ int row(int ch) const { return row0 + ch; }
    __device__ int first_byte(int ch) const { return adpcm_len > 0 ? adpcm[(int64_t)(row0 + ch) * adpcm_pitch] : 0; }
    __device__ TrackK track(int i) const { return a.tracks[i]; }
};

// One workgroup per image (nw_header_body.hpp)
__global__ __launch_bounds__(64) void nw_header_kernel(HeaderArgs a, const uint8_t *__restrict__ adpcm, int64_t adpcm_pitch,
                                                       int adpcm_len, const int16_t *__restrict__ coefs,
                                                       const int16_t *__restrict__ gain, const int16_t *__restrict__ start_ctx,
                                                       const int16_t *__restrict__ loop_ctx, uint8_t *__restrict__ files,
                                                       int64_t file_pitch)
{
    const PitchedRows rows{a, adpcm, adpcm_pitch, adpcm_len, (int)blockIdx.x * a.nch};
    nw::write_header(a, rows, coefs, gain, start_ctx, loop_ctx, files + (int64_t)blockIdx.x * file_pitch);
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
    nw::header_geom(L, p, nch, codec, a);
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
    if (int rc = nw::pcm_read_info_check(I, sample_kind, nfiles > 0)) return rc;
    if (nfiles == 0 || I->adpcm_bytes == 0) return VGA_OK;
    const int nch = I->channel_count;
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
