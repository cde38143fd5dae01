// gc_containers.hip -- the remaining GC-ADPCM containers: HPS (Containers/Hps/HpsWriter.cs, HpsReader.cs), IDSP
// (Containers/Idsp/IdspWriter.cs, IdspReader.cs) and GENH (Containers/Genh/GenhReader.cs; the reference has no
// writer).  Size math (gc_stream_host.hpp) and parsing are host code; the images are assembled and taken apart in HBM, nfiles equally
// shaped files per launch.  Everything on the device is byte movement: HBM-bound, every image byte written once.
#include "container_host.hpp"
#include "gc_stream_host.hpp"

#include <vector>

using namespace vga;
using namespace vga::container;

using gcs::check_channels;            // the channel-count check, hps_layout and idsp_layout live in gc_stream_host.hpp
using gcs::hps_layout;
using gcs::idsp_layout;
using gcs::kHpsMaxBlockSize;
using gcs::kIdspChannelInfoSize;
using gcs::kIdspStreamInfoSize;
using gcs::kMaxChannels;

// ---------------------------------------------------------------- device side
namespace vga {
namespace gcc {

using container::Granule;
using container::kMaxGridY;
using container::pick_granule;

// byte `pos` of a big-endian field of `n` bytes holding v
__device__ __forceinline__ uint8_t be(int v, int n, int pos) { return (uint8_t)((uint32_t)v >> (8 * (n - 1 - pos))); }

struct HpsArgs {
    int nch, sample_rate, end_address, header_size, block_header_size;
    int64_t adpcm_pitch, pcm_pitch;
};

// GcAdpcmChannel.StartContext (GcAdpcmChannel.cs:45): the caller's, or (adpcm[0], 0, 0)
__device__ __forceinline__ int start_ctx(const int16_t *ctx, const uint8_t *adpcm, int64_t pitch, int row, int t)
{
    if (ctx) return ctx[row * 3 + t];
    return t == 0 ? adpcm[(int64_t)row * pitch] : 0;
}

// One thread per header byte, each byte written once.  blockIdx.y == 0: the stream header and channel infos
// (HpsWriter.cs:59-83), zero up to HeaderSize; blockIdx.y == b + 1: block b's header (:91-106) -- WrittenSize, EndNibble,
// NextOffset, then per channel (short)pred/scale of the aligned ADPCM, hist1, hist2 from the Pcm rows and a zero short
// -- zero up to 0x20.  blockIdx.z is the file.
__global__ __launch_bounds__(256) void hps_header_kernel(HpsArgs a, const vga_hps_block *__restrict__ map,
                                                         const uint8_t *__restrict__ adpcm, const int16_t *__restrict__ coefs,
                                                         const int16_t *__restrict__ gain, const int16_t *__restrict__ start,
                                                         const int16_t *__restrict__ pcm, uint8_t *__restrict__ files,
                                                         int64_t file_pitch)
{
    const int k = blockIdx.x * 256 + threadIdx.x, f = blockIdx.z, nch = a.nch;
    uint8_t *img = files + (int64_t)f * file_pitch;
    if (blockIdx.y == 0) {
        if (k >= a.header_size) return;
        uint8_t v = 0;
        if (k < 8) {
            v = " HALPST"[k];                               // the literal's terminating zero is byte 7
        } else if (k < 12) {
            v = be(a.sample_rate, 4, k - 8);
        } else if (k < 16) {
            v = be(nch, 4, k - 12);
        } else if (k < 16 + 0x38 * nch) {                   // WriteChannelInfo (:70-83)
            const int c = (k - 16) / 0x38, q = (k - 16) % 0x38, row = f * nch + c;
            if (q < 4) v = be(kHpsMaxBlockSize, 4, q);
            else if (q < 8) v = be(2, 4, q - 4);            // SampleToNibble(0)
            else if (q < 12) v = be(a.end_address, 4, q - 8);
            else if (q < 16) v = be(2, 4, q - 12);
            else if (q < 48) v = be(coefs[row * 16 + (q - 16) / 2], 2, q & 1);
            else if (q < 50) v = be(gain ? gain[row] : 0, 2, q & 1);
            else v = be(start_ctx(start, adpcm, a.adpcm_pitch, row, (q - 50) / 2), 2, q & 1);
        }
        img[k] = v;
        return;
    }
    if (k >= a.block_header_size) return;
    const vga_hps_block B = map[blockIdx.y - 1];
    uint8_t v = 0;
    if (k < 4) {
        v = be(B.written_size, 4, k);
    } else if (k < 8) {
        v = be(B.end_nibble, 4, k - 4);
    } else if (k < 12) {
        v = be(B.next_offset, 4, k - 8);
    } else if (k < 12 + 8 * nch) {
        const int c = (k - 12) >> 3, q = (k - 12) & 7, t = q >> 1, row = f * nch + c;
        int x = 0;
        if (t == 0) {
            x = adpcm[(int64_t)row * a.adpcm_pitch + B.start_sample / 14 * 8];      // GetPredScale(StartSample)
        } else if (t < 3) {                                 // GcAdpcmLoopContext.GetHist1 / GetHist2 over the Pcm field
            const int i = B.start_sample - t;
            x = i < 0 || !pcm ? 0 : pcm[(int64_t)row * a.pcm_pitch + i];
        }
        v = be(x, 2, q & 1);
    }
    img[B.offset + k] = v;
}

// The block bodies (HpsWriter.cs:108-112): channel c's ChannelSize bytes from ByteInIndex of its row, zero-padded to
// 0x20, one after the other.  One thread per G-byte granule of the body; blockIdx.y is the block, blockIdx.z the file.
// Every padded channel size is a multiple of 0x20, so a granule never straddles two channels.
template <int G>
__global__ __launch_bounds__(256) void hps_body_kernel(const vga_hps_block *__restrict__ map, int nch, int block_header_size,
                                                       const uint8_t *__restrict__ adpcm, int64_t adpcm_pitch,
                                                       uint8_t *__restrict__ files, int64_t file_pitch)
{
    using T = typename Granule<G>::type;
    const vga_hps_block B = map[blockIdx.y];
    const uint32_t o = ((uint32_t)blockIdx.x * 256 + threadIdx.x) * G;
    if (o >= (uint32_t)B.written_size) return;
    const int f = blockIdx.z;
    const uint32_t padded = (uint32_t)B.written_size / nch, c = o / padded, within = o - c * padded;
    const uint32_t n = (uint32_t)B.channel_size;
    const uint8_t *s = adpcm + (int64_t)(f * nch + (int)c) * adpcm_pitch + B.byte_in_index + within;
    T v;
    if (within + G <= n) {
        v = *reinterpret_cast<const T *>(s);
    } else {
        uint8_t tmp[G];
        for (int k = 0; k < G; k++) tmp[k] = within + k < n ? s[k] : 0;
        memcpy(&v, tmp, G);
    }
    *reinterpret_cast<T *>(files + (int64_t)f * file_pitch + B.offset + block_header_size + o) = v;
}

// HpsReader.ReadData (:89-128) -> ToAudioStream (:37-50): block b's AudioSizeBytes of channel c, at
// audioStart + Size / nch * c, to out_offset of the channel's row.  One thread per G-byte granule; blockIdx.y is the
// block, blockIdx.z the row (file * nch + channel).  The ragged end of a block goes byte by byte.
template <int G>
__global__ __launch_bounds__(256) void hps_gather_kernel(const vga_hps_block_info *__restrict__ map, int nch,
                                                         const uint8_t *__restrict__ files, int64_t file_pitch,
                                                         uint8_t *__restrict__ dst, int64_t dst_pitch, int row0)
{
    using T = typename Granule<G>::type;
    const vga_hps_block_info B = map[blockIdx.y];
    const uint32_t within = ((uint32_t)blockIdx.x * 256 + threadIdx.x) * G;
    if (within >= (uint32_t)B.audio_bytes) return;
    const int row = row0 + blockIdx.z, f = row / nch, c = row - f * nch;
    const uint8_t *s = files + (int64_t)f * file_pitch + B.audio_offset + (int64_t)(B.size / nch) * c + within;
    uint8_t *d = dst + (int64_t)row * dst_pitch + B.out_offset + within;
    if (within + G <= (uint32_t)B.audio_bytes) {
        *reinterpret_cast<T *>(d) = *reinterpret_cast<const T *>(s);
        return;
    }
    for (uint32_t k = 0; within + k < (uint32_t)B.audio_bytes; k++) d[k] = s[k];
}

struct IdspArgs {
    int nch, sample_rate, sample_count, loop_start, loop_end, block_size, header_size, audio_data_size;
    int channel_sample_count, channel_nibble_count, looping, start_addr, end_addr, cur_addr;
    int64_t adpcm_pitch;
};

// IdspWriter.WriteHeader (:63-96): one thread per byte of the 0x40 + 0x60 * nch header, each written once; blockIdx.y
// is the file.
__global__ __launch_bounds__(256) void idsp_header_kernel(IdspArgs a, const uint8_t *__restrict__ adpcm,
                                                          const int16_t *__restrict__ coefs, const int16_t *__restrict__ gain,
                                                          const int16_t *__restrict__ start, const int16_t *__restrict__ loop,
                                                          uint8_t *__restrict__ files, int64_t file_pitch)
{
    const int k = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y, nch = a.nch;
    if (k >= a.header_size) return;
    uint8_t v = 0;
    if (k < kIdspStreamInfoSize) {
        const int w = k >> 2, q = k & 3;
        const int fields[12] = {0, 0, nch, a.sample_rate, a.sample_count, a.loop_start, a.loop_end, a.block_size,
                                kIdspStreamInfoSize, kIdspChannelInfoSize, a.header_size, a.audio_data_size};
        if (w == 0) v = "IDSP"[q];
        else if (w < 12) v = be(fields[w], 4, q);
    } else {
        const int c = (k - kIdspStreamInfoSize) / kIdspChannelInfoSize, q = (k - kIdspStreamInfoSize) % kIdspChannelInfoSize;
        const int row = f * nch + c;
        if (q < 12) {
            const int fields[3] = {a.channel_sample_count, a.channel_nibble_count, a.sample_rate};
            v = be(fields[q >> 2], 4, q & 3);
        } else if (q < 16) {
            v = q < 14 ? be(a.looping, 2, q - 12) : 0;      // (short)Looping, (short)0
        } else if (q < 28) {
            const int fields[3] = {a.start_addr, a.end_addr, a.cur_addr};
            v = be(fields[(q - 16) >> 2], 4, q & 3);
        } else if (q < 60) {
            v = be(coefs[row * 16 + (q - 28) / 2], 2, q & 1);
        } else if (q < 62) {
            v = be(gain ? gain[row] : 0, 2, q & 1);
        } else if (q < 68) {
            v = be(start_ctx(start, adpcm, a.adpcm_pitch, row, (q - 62) / 2), 2, q & 1);
        } else if (q < 74) {
            v = be(loop ? loop[row * 3 + (q - 68) / 2] : 0, 2, q & 1);
        }
    }
    files[(int64_t)f * file_pitch + k] = v;
}

}  // namespace gcc
}  // namespace vga

// ---------------------------------------------------------------- host side
namespace {

using container::kMaxGridY;

int check_write(int nfiles, int nch, const uint8_t *d_adpcm, int64_t adpcm_pitch, int adpcm_len, int need, const int16_t *d_coefs,
                uint8_t *d_files, int64_t file_pitch, int file_size)
{
    if (nfiles < 0 || adpcm_len < 0) { set_error("negative count / length"); return VGA_ERR_ARGUMENT; }
    if (nfiles == 0) return VGA_OK;
    if (!d_files || !d_coefs || (adpcm_len > 0 && !d_adpcm)) { set_error("null device pointer"); return VGA_ERR_ARGUMENT; }
    if (adpcm_len < need) { set_error("adpcm rows of %d bytes: the layout needs %d", adpcm_len, need); return VGA_ERR_ARGUMENT; }
    if (adpcm_len > 0 && adpcm_pitch < adpcm_len) { set_error("adpcm pitch < length"); return VGA_ERR_ARGUMENT; }
    return check_write_files(nfiles, nch, file_pitch, file_size);
}

// the HPS and IDSP writers' host forms: the rows and tables go up
struct StagedAdpcm {
    uint8_t *adpcm = nullptr;
    const int16_t *coefs = nullptr, *gain = nullptr, *start = nullptr, *loop = nullptr;
    int64_t apitch = 0;
    int up(HostStage &h, int nch, const uint8_t *const *rows, int len, const int16_t *c, const int16_t *g, const int16_t *sc,
           const int16_t *lc)
    {
        if (int rc = h.open()) return rc;
        if (int rc = h.rows(rows, nch, len, &adpcm, &apitch)) return rc;
        if (int rc = h.table(c, (size_t)nch * 16, &coefs)) return rc;
        if (int rc = h.table(g, (size_t)nch, &gain)) return rc;
        if (int rc = h.table(sc, (size_t)nch * 3, &start)) return rc;
        return h.table(lc, (size_t)nch * 3, &loop);
    }
};

int check_host_rows(const uint8_t *const *adpcm, int adpcm_len, int nch, const int16_t *coefs, const uint8_t *file_out)
{
    if (adpcm_len < 0) { set_error("negative length"); return VGA_ERR_ARGUMENT; }
    if (!coefs || !file_out || (adpcm_len > 0 && !adpcm)) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    for (int c = 0; c < nch && adpcm_len > 0; c++)
        if (!adpcm[c]) { set_error("channel %d: null pointer", c); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

int check_out_rows(uint8_t *const *out, int nch)
{
    if (!out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    for (int c = 0; c < nch; c++)
        if (!out[c]) { set_error("channel %d: null pointer", c); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- HPS
int vga_hps_layout_for(const vga_hps_params *p, int nch, vga_hps_layout *out) { return hps_layout(p, nch, out, nullptr); }

int vga_hps_block_map(const vga_hps_params *p, int nch, vga_hps_block *blocks, int capacity)
{
    vga_hps_layout L;
    std::vector<vga_hps_block> m;
    if (int rc = hps_layout(p, nch, &L, &m)) return rc;
    if (!blocks || capacity < L.block_count) { set_error("block map of %d entries: capacity %d", L.block_count, capacity); return VGA_ERR_ARGUMENT; }
    std::copy(m.begin(), m.end(), blocks);
    return VGA_OK;
}

int vga_hps_write_device(const vga_hps_params *p, int nch, int nfiles, const uint8_t *d_adpcm, int64_t adpcm_pitch,
                         int adpcm_len, const int16_t *d_coefs, const int16_t *d_gain, const int16_t *d_start_context,
                         const int16_t *d_pcm, int64_t pcm_pitch, int pcm_len, uint8_t *d_files, int64_t file_pitch,
                         void *stream)
{
    vga_hps_layout L;
    std::vector<vga_hps_block> m;
    if (int rc = hps_layout(p, nch, &L, &m)) return rc;
    if (int rc = check_write(nfiles, nch, d_adpcm, adpcm_pitch, adpcm_len, L.channel_adpcm_bytes, d_coefs, d_files, file_pitch,
                             L.file_size))
        return rc;
    if (d_pcm && (pcm_len < 0 || pcm_pitch < pcm_len)) { set_error("pcm pitch < length"); return VGA_ERR_ARGUMENT; }
    if (d_pcm)                                              // GetHist1 / GetHist2 index Pcm[StartSample - 1 / - 2]
        if (int rc = gcs::hps_check_pcm(m, pcm_len)) return rc;
    if (nfiles == 0) return VGA_OK;
    if (L.block_count >= kMaxGridY) { set_error("%d blocks: at most %d per call", L.block_count, kMaxGridY - 1); return VGA_ERR_ARGUMENT; }
    hipStream_t s = (hipStream_t)stream;
    AsyncBuf d_map;
    if (int rc = container::upload_table(m.data(), L.block_count, d_map, s)) return rc;
    gcc::HpsArgs a{nch, p->sample_rate, vga_gcadpcm_sample_to_nibble(L.sample_count - 1), L.header_size, L.block_header_size,
                   adpcm_pitch, pcm_pitch};
    int max_written = 0;
    for (const vga_hps_block &b : m) max_written = std::max(max_written, b.written_size);
    const uint64_t align = (uint64_t)(uintptr_t)d_adpcm | (uint64_t)adpcm_pitch | (uint64_t)(uintptr_t)d_files |
                           (uint64_t)(nfiles > 1 ? file_pitch : 0) | (uint64_t)L.header_size | (uint64_t)L.block_header_size;
    const unsigned header_x = (unsigned)((std::max(L.header_size, L.block_header_size) + 255) / 256);
    for (int f0 = 0; f0 < nfiles; f0 += kMaxGridY) {
        const int nf = std::min(nfiles - f0, kMaxGridY);
        const int64_t r0 = (int64_t)f0 * nch;
        uint8_t *files = d_files + (int64_t)f0 * file_pitch;
        const uint8_t *adpcm = d_adpcm + r0 * adpcm_pitch;
        hipLaunchKernelGGL(gcc::hps_header_kernel, dim3(header_x, L.block_count + 1, nf), dim3(256), 0, s, a,
                           d_map.as<vga_hps_block>(), adpcm, d_coefs + r0 * 16, d_gain ? d_gain + r0 : nullptr,
                           d_start_context ? d_start_context + r0 * 3 : nullptr, d_pcm ? d_pcm + r0 * pcm_pitch : nullptr,
                           files, file_pitch);
        VGA_HIP_TRY(hipGetLastError());
        if (int rc = container::pick_granule(align, [&](auto g) {
                constexpr int G = decltype(g)::value;
                hipLaunchKernelGGL(gcc::hps_body_kernel<G>, dim3((unsigned)((max_written / G + 255) / 256), L.block_count, nf),
                                   dim3(256), 0, s, d_map.as<vga_hps_block>(), nch, L.block_header_size, adpcm, adpcm_pitch,
                                   files, file_pitch);
            }))
            return rc;
    }
    return VGA_OK;
}

int vga_hps_write(const vga_hps_params *p, int nch, const uint8_t *const *adpcm, int adpcm_len, const int16_t *coefs,
                  const int16_t *gain, const int16_t *start_context, const int16_t *const *pcm, int pcm_len, uint8_t *file_out)
{
    vga_hps_layout L;
    if (int rc = vga_hps_layout_for(p, nch, &L)) return rc;
    if (int rc = check_host_rows(adpcm, adpcm_len, nch, coefs, file_out)) return rc;
    if (pcm && pcm_len < 0) { set_error("negative pcm length"); return VGA_ERR_ARGUMENT; }
    for (int c = 0; pcm && c < nch && pcm_len > 0; c++)
        if (!pcm[c]) { set_error("channel %d: null pcm pointer", c); return VGA_ERR_ARGUMENT; }
    HostStage h;
    StagedAdpcm w;
    int16_t *d_pcm = nullptr;
    int64_t ppitch = 0;
    if (int rc = w.up(h, nch, adpcm, adpcm_len, coefs, gain, start_context, nullptr)) return rc;
    if (pcm)
        if (int rc = h.rows(pcm, nch, pcm_len, &d_pcm, &ppitch)) return rc;
    return h.write_image(file_out, (size_t)L.file_size, [&](uint8_t *d_file, hipStream_t s) {
        return vga_hps_write_device(p, nch, 1, w.adpcm, w.apitch, adpcm_len, w.coefs, w.gain, w.start, d_pcm, ppitch, pcm_len, d_file,
                                    L.file_size, s);
    });
}

// HpsReader.ReadFile (:14-31) and what ToAudioStream (:33-65) checks
int vga_hps_parse(const uint8_t *file, size_t size, vga_hps_info *out, vga_hps_block_info *blocks, int capacity)
{
    if (!file || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    std::memset(out, 0, sizeof *out);
    vga_hps_info &I = *out;
    ByteReader r{file, (int64_t)size, 0, true};
    if (!r.magic(" HALPST\0", 8)) return invalid("File has no HALPST header");
    I.sample_rate = r.i32();                                // ReadHeader (:67-87)
    const int nch = r.i32();
    if (r.eof) return invalid("file ends inside the HPS header");
    if (nch > kMaxChannels) { set_error("HPS file with %d channels: at most %d are read here", nch, kMaxChannels); return VGA_ERR_INVALID_OP; }
    if (nch < 1) return invalid("the HPS file has no channels");
    I.channel_count = nch;
    for (int c = 0; c < nch; c++) {
        I.max_block_size[c] = r.i32();
        r.i32();
        I.end_address[c] = r.i32();
        r.i32();
        for (int k = 0; k < 16; k++) I.coefs[c][k] = (int16_t)r.i16();
        I.gain[c] = (int16_t)r.i16();
        for (int k = 0; k < 3; k++) I.start_context[c][k] = (int16_t)r.i16();
    }
    if (r.eof) return invalid("file ends inside the channel infos");
    // ReadData (:89-128): follow NextOffset while it moves forward
    int64_t current = 0, next = next_multiple(std::max<int64_t>(0x80, r.pos), 0x20), out_offset = 0;
    int count = 0;
    vga_hps_block_info last{};
    while (next > current) {
        r.pos = current = next;
        vga_hps_block_info b{};
        b.offset = (int)current;
        b.size = r.i32();
        b.final_nibble = r.i32();
        b.next_offset = r.i32();
        r.pos += 8 * (int64_t)nch;                          // the contexts; the loop block's are read again below
        if (r.eof || r.pos > r.len) return invalid("file ends inside a block header");
        const int64_t audio_start = next_multiple(r.pos, 0x20);
        const int64_t nibbles = (int64_t)b.final_nibble + 1;
        if (nibbles < 0) return invalid("negative block audio size");
        b.audio_offset = (int)audio_start;
        b.audio_bytes = (int)(nibbles / 2 + (nibbles & 1));  // AudioSizeBytes: DivideBy2RoundUp
        for (int c = 0; c < nch; c++) {
            const int64_t at = audio_start + (int64_t)(b.size / nch) * c;
            if (at < 0 || at + b.audio_bytes > r.len) return invalid("block audio runs past the end of the file");
        }
        b.out_offset = (int)out_offset;
        out_offset += b.audio_bytes;
        if (out_offset > 0x7FFFFFFF) return invalid("channel audio exceeds 2 GiB");
        if (blocks && count < capacity) blocks[count] = b;
        count++;
        last = b;
        next = b.next_offset;
    }
    I.block_count = count;
    I.adpcm_bytes = (int)out_offset;
    // VerifyData (:130-157)
    I.sample_count = vga_gcadpcm_nibble_to_sample(I.end_address[0]) + 1;
    for (int c = 1; c < nch; c++)
        if (vga_gcadpcm_nibble_to_sample(I.end_address[c]) + 1 != I.sample_count) return invalid("Channels have differing sample counts");
    if (last.next_offset != -1) {
        // the loop start block: walk the chain again (blocks may be NULL); its header carries the loop context
        ByteReader w{file, (int64_t)size, 0, true};
        int64_t cur = 0, nxt = next_multiple(std::max<int64_t>(0x80, 0x10 + 0x38 * (int64_t)nch), 0x20);
        int64_t nibble = 0;
        while (nxt > cur) {
            w.pos = cur = nxt;
            w.i32();
            const int final_nibble = w.i32();
            const int next_offset = w.i32();
            if (cur == last.next_offset) {
                I.looping = 1;
                I.loop_start = vga_gcadpcm_nibble_count_to_sample_count((int)nibble);
                for (int c = 0; c < nch; c++, w.pos += 2)
                    for (int k = 0; k < 3; k++) I.loop_context[c][k] = (int16_t)w.i16();
            }
            nibble += (int64_t)final_nibble + 1;
            nxt = next_offset;
        }
    }
    // ToAudioStream: GcAdpcmChannel(builder) and WithLoop(Looping, LoopStart, SampleCount)
    if (I.sample_count < 0) return invalid("negative sample count");
    if (I.adpcm_bytes < bytes_of(I.sample_count)) return invalid("Audio array length is too short for the specified number of samples.");
    if (I.looping && (I.loop_start < 0 || I.loop_start > I.sample_count)) return invalid("loop start outside the stream");
    if (blocks && count > capacity) { set_error("%d blocks: capacity %d", count, capacity); return VGA_ERR_ARGUMENT; }
    return VGA_OK;
}

int vga_hps_read_device(const vga_hps_info *I, const vga_hps_block_info *blocks, const uint8_t *d_files, int64_t file_pitch,
                        int nfiles, uint8_t *d_adpcm, int64_t adpcm_pitch, void *stream)
{
    if (!I || !blocks || nfiles < 0) { set_error("null / negative argument"); return VGA_ERR_ARGUMENT; }
    const int nch = I->channel_count;
    if (int rc = gcs::hps_check_info(I)) return rc;
    if (nfiles == 0 || I->adpcm_bytes == 0) return VGA_OK;
    if (!d_files || !d_adpcm || adpcm_pitch < I->adpcm_bytes) { set_error("null pointer / adpcm pitch < %d", I->adpcm_bytes); return VGA_ERR_ARGUMENT; }
    if ((int64_t)nfiles * nch > 0x7FFFFFFF) { set_error("too many files in one call"); return VGA_ERR_ARGUMENT; }
    uint64_t align = (uint64_t)(uintptr_t)d_files | (uint64_t)(nfiles > 1 ? file_pitch : 0) | (uint64_t)(uintptr_t)d_adpcm |
                     (uint64_t)adpcm_pitch;
    int max_bytes = 0;
    int64_t end = 0;
    for (int i = 0; i < I->block_count; i++) {
        const vga_hps_block_info &b = blocks[i];
        if (int rc = gcs::hps_check_block(I, b, i)) return rc;
        end = std::max(end, (int64_t)b.audio_offset + (int64_t)(b.size / nch) * (nch - 1) + b.audio_bytes);
        align |= (uint64_t)(uint32_t)b.audio_offset | (uint64_t)(uint32_t)(b.size / nch) | (uint64_t)(uint32_t)b.out_offset;
        max_bytes = std::max(max_bytes, b.audio_bytes);
    }
    if (nfiles > 1 && file_pitch < end) { set_error("file pitch smaller than the file"); return VGA_ERR_ARGUMENT; }
    if (max_bytes == 0) return VGA_OK;
    hipStream_t s = (hipStream_t)stream;
    AsyncBuf d_map;
    if (int rc = container::upload_table(blocks, I->block_count, d_map, s)) return rc;
    const int rows = nfiles * nch;
    for (int b0 = 0; b0 < I->block_count; b0 += kMaxGridY)
        for (int r0 = 0; r0 < rows; r0 += kMaxGridY) {
            const int nb = std::min(I->block_count - b0, kMaxGridY), nr = std::min(rows - r0, kMaxGridY);
            if (int rc = container::pick_granule(align, [&](auto g) {
                    constexpr int G = decltype(g)::value;
                    hipLaunchKernelGGL(gcc::hps_gather_kernel<G>, dim3((unsigned)(((max_bytes + G - 1) / G + 255) / 256), nb, nr),
                                       dim3(256), 0, s, d_map.as<vga_hps_block_info>() + b0, nch, d_files, file_pitch, d_adpcm,
                                       adpcm_pitch, r0);
                }))
                return rc;
        }
    return VGA_OK;
}

int vga_hps_read(const uint8_t *file, size_t size, const vga_hps_info *I, const vga_hps_block_info *blocks,
                 uint8_t *const *adpcm_out)
{
    if (!file || !I || !blocks) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (I->channel_count < 1 || I->channel_count > kMaxChannels) { set_error("info does not describe an HPS file"); return VGA_ERR_ARGUMENT; }
    if (int rc = check_out_rows(adpcm_out, I->channel_count)) return rc;
    for (int i = 0; i < I->block_count; i++) {
        const vga_hps_block_info &b = blocks[i];
        for (int c = 0; c < I->channel_count; c++) {
            const int64_t at = b.audio_offset + (int64_t)(b.size / I->channel_count) * c;
            if (at < 0 || at + b.audio_bytes > (int64_t)size) { set_error("info does not describe this file"); return VGA_ERR_ARGUMENT; }
        }
    }
    if (I->adpcm_bytes == 0) return VGA_OK;
    HostStage h;
    return h.read_rows(file, size, adpcm_out, I->channel_count, I->adpcm_bytes, 1,
                       [&](const uint8_t *f, void *d, int64_t dp, hipStream_t s) {
                           return vga_hps_read_device(I, blocks, f, (int64_t)size, 1, static_cast<uint8_t *>(d), dp, s);
                       });
}

// ---------------------------------------------------------------- IDSP
int vga_idsp_layout_for(const vga_idsp_params *p, int nch, vga_idsp_layout *out) { return idsp_layout(p, nch, out); }

int vga_idsp_write_device(const vga_idsp_params *p, int nch, int nfiles, const uint8_t *d_adpcm, int64_t adpcm_pitch,
                          int adpcm_len, const int16_t *d_coefs, const int16_t *d_gain, const int16_t *d_start_context,
                          const int16_t *d_loop_context, uint8_t *d_files, int64_t file_pitch, void *stream)
{
    vga_idsp_layout L;
    if (int rc = idsp_layout(p, nch, &L)) return rc;
    if (int rc = check_write(nfiles, nch, d_adpcm, adpcm_pitch, adpcm_len, 0, d_coefs, d_files, file_pitch, L.file_size)) return rc;
    if (nfiles == 0) return VGA_OK;
    if (adpcm_len == 0 && !d_start_context) { set_error("no audio: the start context reads Adpcm[0]"); return VGA_ERR_ARGUMENT; }
    hipStream_t s = (hipStream_t)stream;
    gcc::IdspArgs a{nch, p->sample_rate, L.sample_count, L.loop_start, L.loop_end, p->block_size, L.header_size,
                    L.audio_data_size, L.channel_sample_count, vga_gcadpcm_sample_count_to_nibble_count(L.channel_sample_count),
                    L.looping, L.start_addr, L.end_addr, L.cur_addr, adpcm_pitch};
    for (int f0 = 0; f0 < nfiles; f0 += kMaxGridY) {
        const int nf = std::min(nfiles - f0, kMaxGridY);
        const int64_t r0 = (int64_t)f0 * nch;
        hipLaunchKernelGGL(gcc::idsp_header_kernel, dim3((L.header_size + 255) / 256, nf), dim3(256), 0, s, a,
                           d_adpcm ? d_adpcm + r0 * adpcm_pitch : nullptr, d_coefs + r0 * 16, d_gain ? d_gain + r0 : nullptr,
                           d_start_context ? d_start_context + r0 * 3 : nullptr, d_loop_context ? d_loop_context + r0 * 3 : nullptr,
                           d_files + (int64_t)f0 * file_pitch, file_pitch);
        VGA_HIP_TRY(hipGetLastError());
    }
    // WriteData (:98-104): Interleave(channels, InterleaveSize, AudioDataSize)
    return interleave_images(d_adpcm, adpcm_pitch, nch, nfiles, (uint32_t)adpcm_len, (uint32_t)L.interleave_size,
                             (uint32_t)L.audio_data_size, d_files + L.header_size, file_pitch, s);
}

int vga_idsp_write(const vga_idsp_params *p, int nch, const uint8_t *const *adpcm, int adpcm_len, const int16_t *coefs,
                   const int16_t *gain, const int16_t *start_context, const int16_t *loop_context, uint8_t *file_out)
{
    vga_idsp_layout L;
    if (int rc = vga_idsp_layout_for(p, nch, &L)) return rc;
    if (int rc = check_host_rows(adpcm, adpcm_len, nch, coefs, file_out)) return rc;
    HostStage h;
    StagedAdpcm w;
    if (int rc = w.up(h, nch, adpcm, adpcm_len, coefs, gain, start_context, loop_context)) return rc;
    return h.write_image(file_out, (size_t)L.file_size, [&](uint8_t *d_file, hipStream_t s) {
        return vga_idsp_write_device(p, nch, 1, w.adpcm, w.apitch, adpcm_len, w.coefs, w.gain, w.start, w.loop, d_file, L.file_size, s);
    });
}

// IdspReader.ReadFile (:13-31)
int vga_idsp_parse(const uint8_t *file, size_t size, vga_idsp_info *out)
{
    if (!file || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    std::memset(out, 0, sizeof *out);
    vga_idsp_info &I = *out;
    ByteReader r{file, (int64_t)size, 0, true};
    if (!r.magic("IDSP", 4)) return invalid("File has no IDSP header");
    r.pos += 4;                                             // ReadIdspHeader (:72-103)
    I.channel_count = r.i32();
    I.sample_rate = r.i32();
    I.sample_count = r.i32();
    I.loop_start = r.i32();
    I.loop_end = r.i32();
    I.interleave_size = r.i32();
    I.header_size = r.i32();
    I.channel_info_size = r.i32();
    I.audio_data_offset = r.i32();
    I.audio_data_length = r.i32();
    if (r.eof) return invalid("file ends inside the IDSP header");
    const int nch = I.channel_count;
    if (nch > kMaxChannels) { set_error("IDSP file with %d channels: at most %d are read here", nch, kMaxChannels); return VGA_ERR_INVALID_OP; }
    if (nch < 1) return invalid("the IDSP file has no channels (DeInterleave divides by the channel count)");
    for (int c = 0; c < nch; c++) {
        r.pos = (int64_t)I.header_size + (int64_t)c * I.channel_info_size;
        I.channel_sample_count[c] = r.i32();
        r.i32();                                            // NibbleCount
        r.i32();                                            // SampleRate
        I.channel_looping[c] = r.i16() == 1;
        r.pos += 2;
        I.start_address[c] = r.i32();
        I.end_address[c] = r.i32();
        r.i32();                                            // CurrentAddress
        for (int k = 0; k < 16; k++) I.coefs[c][k] = (int16_t)r.i16();
        I.gain[c] = (int16_t)r.i16();
        for (int k = 0; k < 3; k++) I.start_context[c][k] = (int16_t)r.i16();
        for (int k = 0; k < 3; k++) I.loop_context[c][k] = (int16_t)r.i16();
        if (r.eof) return invalid("file ends inside a channel info");
        I.looping |= I.channel_looping[c];                  // no file-wide loop flag: any channel's
    }
    // ReadIdspData (:105-112): DeInterleave(ChannelCount * AudioDataLength, interleave, ChannelCount,
    // SampleCountToByteCount(SampleCount)) from AudioDataOffset
    I.interleave = I.interleave_size == 0 ? I.audio_data_length : I.interleave_size;
    if (I.interleave <= 0) return invalid("interleave size must be positive (DeInterleave divides by it)");
    if (I.audio_data_length < 0 || I.sample_count < 0) return invalid("negative audio length / sample count");
    const int64_t length = (int64_t)nch * I.audio_data_length;
    if (length > 0x7FFFFFFF) return invalid("audio data length exceeds 2 GiB");
    if (I.audio_data_offset < 0 || (int64_t)size - I.audio_data_offset < length)
        return invalid("Specified length is greater than the number of bytes remaining in the Stream");
    I.adpcm_bytes = bytes_of(I.sample_count);
    return VGA_OK;
}

int vga_idsp_read_device(const vga_idsp_info *I, const uint8_t *d_files, int64_t file_pitch, int nfiles, uint8_t *d_adpcm,
                         int64_t adpcm_pitch, void *stream)
{
    if (!I || nfiles < 0) { set_error("null / negative argument"); return VGA_ERR_ARGUMENT; }
    const int nch = I->channel_count;
    if (int rc = gcs::idsp_check_info(I)) return rc;
    if (nfiles == 0 || I->adpcm_bytes == 0) return VGA_OK;
    if (int rc = check_read_batch(d_files, d_adpcm, adpcm_pitch, I->adpcm_bytes, nfiles, file_pitch,
                                  I->audio_data_offset + (int64_t)nch * I->audio_data_length))
        return rc;
    return deinterleave_images(d_files, file_pitch, nfiles, I->audio_data_offset, nch, (uint32_t)I->audio_data_length,
                               (uint32_t)I->interleave, (uint32_t)I->adpcm_bytes, d_adpcm, adpcm_pitch, (hipStream_t)stream);
}

int vga_idsp_read(const uint8_t *file, size_t size, const vga_idsp_info *I, uint8_t *const *adpcm_out)
{
    if (!file || !I) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    const int nch = I->channel_count;
    const int64_t bytes = I->audio_data_offset + (int64_t)nch * I->audio_data_length;
    if (nch < 1 || nch > kMaxChannels || I->audio_data_offset < 0 || bytes > (int64_t)size) { set_error("info does not describe this file"); return VGA_ERR_ARGUMENT; }
    if (int rc = check_out_rows(adpcm_out, nch)) return rc;
    if (I->adpcm_bytes == 0) return VGA_OK;
    HostStage h;
    return h.read_rows(file, (size_t)bytes, adpcm_out, nch, I->adpcm_bytes, 1, [&](const uint8_t *f, void *d, int64_t dp, hipStream_t s) {
        return vga_idsp_read_device(I, f, bytes, 1, static_cast<uint8_t *>(d), dp, s);
    });
}

// ---------------------------------------------------------------- GENH
// GenhReader.ReadHeader (:50-97) and ReadCoefs (:99-121); the audio as ReadData (:123-127) takes it
int vga_genh_parse(const uint8_t *file, size_t size, vga_genh_info *out)
{
    if (!file || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    std::memset(out, 0, sizeof *out);
    vga_genh_info &I = *out;
    ByteReader r{file, (int64_t)size, 0, false};
    if (!r.magic("GENH", 4)) return invalid("File has no GENH header");
    I.channel_count = r.i32();
    I.interleave = r.i32();
    I.sample_rate = r.i32();
    I.loop_start = r.i32();
    I.loop_end = r.i32();
    I.codec = r.i32();
    I.audio_data_offset = r.i32();
    I.header_size = r.i32();
    I.coef_offset[0] = r.i32();
    I.coef_offset[1] = r.i32();
    I.interleave_type = r.i32();
    I.coef_type = r.i32();
    I.coef_split_offset[0] = r.i32();
    I.coef_split_offset[1] = r.i32();
    if (r.eof) return invalid("file ends inside the GENH header");
    if (I.channel_count < 1) return invalid("File must have at least one channel.");
    if (I.channel_count > 2) return invalid("GENH does not support more than 2 channels with NGC DSP files.");
    if (I.header_size > I.audio_data_offset) return invalid("Audio data must come after the GENH header.");
    ByteReader c{file, (int64_t)size, 0, (I.coef_type & 2) == 0};   // GenhCoefType.LittleEndian = 2, else big-endian
    for (int ch = 0; ch < I.channel_count; ch++) {
        c.pos = I.coef_offset[ch];
        if (I.coef_type & 1) {                              // GenhCoefType.Split
            for (int k = 0; k < 8; k++) I.coefs[ch][k * 2] = (int16_t)c.i16();
            c.pos = I.coef_split_offset[ch];
            for (int k = 0; k < 8; k++) I.coefs[ch][k * 2 + 1] = (int16_t)c.i16();
        } else {
            for (int k = 0; k < 16; k++) I.coefs[ch][k] = (int16_t)c.i16();
        }
        if (c.eof) return invalid("file ends inside the coefficients");
    }
    I.sample_count = I.loop_end;                            // GenhStructure.cs:25-26
    I.looping = I.loop_start != -1;
    // DeInterleave(stream, SampleCountToByteCount(SampleCount) * ChannelCount, Interleave, ChannelCount)
    if (I.sample_count < 0) return invalid("negative sample count");
    if (I.interleave <= 0) return invalid("interleave must be positive (DeInterleave divides by it)");
    I.adpcm_bytes = bytes_of(I.sample_count);
    const int64_t length = (int64_t)I.adpcm_bytes * I.channel_count;
    if (I.audio_data_offset < 0 || (int64_t)size - I.audio_data_offset < length)
        return invalid("Specified length is greater than the number of bytes remaining in the Stream");
    return VGA_OK;
}

int vga_genh_read_device(const vga_genh_info *I, const uint8_t *d_files, int64_t file_pitch, int nfiles, uint8_t *d_adpcm,
                         int64_t adpcm_pitch, void *stream)
{
    if (!I || nfiles < 0) { set_error("null / negative argument"); return VGA_ERR_ARGUMENT; }
    const int nch = I->channel_count;
    if (nch < 1 || nch > 2 || I->interleave <= 0 || I->adpcm_bytes < 0) { set_error("info does not describe a GENH file"); return VGA_ERR_ARGUMENT; }
    if (nfiles == 0 || I->adpcm_bytes == 0) return VGA_OK;
    if (int rc = check_read_batch(d_files, d_adpcm, adpcm_pitch, I->adpcm_bytes, nfiles, file_pitch,
                                  I->audio_data_offset + (int64_t)nch * I->adpcm_bytes))
        return rc;
    // no output size: every channel's row is its whole input (inputSize = length / ChannelCount)
    return deinterleave_images(d_files, file_pitch, nfiles, I->audio_data_offset, nch, (uint32_t)I->adpcm_bytes,
                               (uint32_t)I->interleave, (uint32_t)I->adpcm_bytes, d_adpcm, adpcm_pitch, (hipStream_t)stream);
}

int vga_genh_read(const uint8_t *file, size_t size, const vga_genh_info *I, uint8_t *const *adpcm_out)
{
    if (!file || !I) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    const int nch = I->channel_count;
    const int64_t bytes = I->audio_data_offset + (int64_t)nch * I->adpcm_bytes;
    if (nch < 1 || nch > 2 || I->audio_data_offset < 0 || bytes > (int64_t)size) { set_error("info does not describe this file"); return VGA_ERR_ARGUMENT; }
    if (int rc = check_out_rows(adpcm_out, nch)) return rc;
    if (I->adpcm_bytes == 0) return VGA_OK;
    HostStage h;
    return h.read_rows(file, (size_t)bytes, adpcm_out, nch, I->adpcm_bytes, 1, [&](const uint8_t *f, void *d, int64_t dp, hipStream_t s) {
        return vga_genh_read_device(I, f, bytes, 1, static_cast<uint8_t *>(d), dp, s);
    });
}

}  // extern "C"
