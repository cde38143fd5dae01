// nwwav.hip -- NintendoWare wave files (BRWAV, BCWAV, BFWAV) and prefetch files (BCSTP, BFSTP): the host parser
// (nwwav_parse.hpp) behind the C ABI, and the bank reader, which takes the channels of thousands of parsed files out
// of one device buffer into the packed layouts of the ragged GC-ADPCM decoder and of PCM16 / PCM8 rows in one launch.
// Everything on the device is byte movement: HBM-bound, every audio byte read once and written once.
#include "container_host.hpp"
#include "nwwav_parse.hpp"

#include <vector>

using namespace vga;

namespace vga {
namespace nwwav {

constexpr uint32_t kPieceBytes = 16384;                     // of destination: 1024 chunks of 16 bytes, 4 per lane
constexpr int kThreads = 256, kMaxGroupPieces = 64;
constexpr int64_t kGuardBytes = 256;                        // vga_gcadpcm_ragged_adpcm_bytes - the end of the last row
enum : uint32_t { kOutMask = 3, kSwap16 = 4, kPrefetch = 8 };   // Piece::flags; the output is the NwCodec

// `total` bytes (a multiple of 16) at `dst` of output flags & kOutMask: the first `copy` come from the bank's files,
// the rest are zeros.  Plain rows: byte k is d_files[src + k].  Prefetch rows: byte k is byte pos0 + k of channel `c`
// of the region at src, `in` bytes per channel in blocks of `il` (Interleave.cs:118-167).
struct Piece {
    int64_t src, dst;
    uint32_t copy, total, flags, il, in, pos0;
    uint32_t nch, c;
};

__device__ __forceinline__ uint32_t swap16(uint32_t v) { return ((v & 0x00ff00ffu) << 8) | ((v >> 8) & 0x00ff00ffu); }

// bytes m .. m + 15 of the 32 that lo and hi hold, m = 4 * Q + sh / 8
template <int Q>
__device__ __forceinline__ uint4 funnel(const uint32_t (&w)[8], uint32_t sh)
{
    return make_uint4(__funnelshift_r(w[Q], w[Q + 1], sh), __funnelshift_r(w[Q + 1], w[Q + 2], sh),
                      __funnelshift_r(w[Q + 2], w[Q + 3], sh), __funnelshift_r(w[Q + 3], w[Q + 4], sh));
}

// chunks first, first + step, ... of one piece
__device__ __forceinline__ void move_piece(const Piece &p, const uint8_t *__restrict__ files, uint8_t *__restrict__ out, uint32_t first,
                                           uint32_t step)
{
    const uint8_t *src = files + p.src;
    const uintptr_t lo = (uintptr_t)src, hi = lo + p.copy;   // what may be read
    const uint32_t m = (uint32_t)(lo & 15), sh = (m & 3) * 8;
    const bool swap = p.flags & kSwap16, prefetch = p.flags & kPrefetch;
    const uint32_t blocks = prefetch ? (p.in + p.il - 1) / p.il : 0, last = prefetch ? p.in - (blocks - 1) * p.il : 0;
    for (uint32_t k = first; k < p.total / 16; k += step) {
        const uint32_t at = k * 16;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (at < p.copy) {
            const uint8_t *s = src + at;
            uint32_t n = min(16u, p.copy - at);
            bool wide = false;
            if (prefetch) {                                 // where the chunk starts, and how much of it one block holds
                const uint32_t pos = p.pos0 + at, b = pos / p.il, cur = b == blocks - 1 ? last : p.il, within = pos - b * p.il;
                s = src + (uint64_t)b * p.il * p.nch + (uint64_t)p.c * cur + within;
                if (within + n > cur) {                     // the chunk crosses into the next block: byte by byte
                    uint32_t w[4] = {0, 0, 0, 0};
                    for (uint32_t j = 0; j < n; j++) {
                        const uint32_t q = pos + j, bj = q / p.il, cj = bj == blocks - 1 ? last : p.il;
                        w[j >> 2] |= (uint32_t)src[(uint64_t)bj * p.il * p.nch + (uint64_t)p.c * cj + (q - bj * p.il)] << ((j & 3) * 8);
                    }
                    v = make_uint4(w[0], w[1], w[2], w[3]);
                    n = 0;
                }
            } else {
                const uintptr_t a = (uintptr_t)s & ~(uintptr_t)15;
                wide = a >= lo && a + (m ? 32 : 16) <= hi;   // aligned loads that stay inside the row
                if (wide) {
                    const uint4 x = *reinterpret_cast<const uint4 *>(a);
                    if (m == 0) v = x;
                    else {
                        const uint4 y = *reinterpret_cast<const uint4 *>(a + 16);
                        const uint32_t w[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
                        switch (m >> 2) {                   // uniform over the piece
                        case 0: v = funnel<0>(w, sh); break;
                        case 1: v = funnel<1>(w, sh); break;
                        case 2: v = funnel<2>(w, sh); break;
                        default: v = funnel<3>(w, sh); break;
                        }
                    }
                    n = 0;
                }
            }
            if (n) {                                        // head and tail of a row, and prefetch blocks: byte loads
                uint32_t w[4] = {0, 0, 0, 0};
                for (uint32_t j = 0; j < n; j++) w[j >> 2] |= (uint32_t)s[j] << ((j & 3) * 8);
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            if (swap) v = make_uint4(swap16(v.x), swap16(v.y), swap16(v.z), swap16(v.w));
        }
        *reinterpret_cast<uint4 *>(out + p.dst + at) = v;
    }
}

// One workgroup per group of pieces: a long row's piece alone, all 256 threads on its chunks; up to 64 pieces of short
// rows together, one wave on each in turn.
__global__ __launch_bounds__(kThreads) void bank_read_kernel(const Piece *__restrict__ pieces, const uint32_t *__restrict__ group_first,
                                                              const uint8_t *__restrict__ files, uint8_t *__restrict__ adpcm,
                                                              uint8_t *__restrict__ pcm16, uint8_t *__restrict__ pcm8)
{
    const uint32_t first = group_first[blockIdx.x], end = group_first[blockIdx.x + 1];
    if (end - first == 1) {
        const Piece p = pieces[first];
        const uint32_t o = p.flags & kOutMask;
        move_piece(p, files, o == VGA_NW_CODEC_GCADPCM ? adpcm : o == VGA_NW_CODEC_PCM16 ? pcm16 : pcm8, threadIdx.x, kThreads);
        return;
    }
    for (uint32_t i = first + threadIdx.x / 64; i < end; i += kThreads / 64) {
        const Piece p = pieces[i];
        const uint32_t o = p.flags & kOutMask;
        move_piece(p, files, o == VGA_NW_CODEC_GCADPCM ? adpcm : o == VGA_NW_CODEC_PCM16 ? pcm16 : pcm8, threadIdx.x % 64, 64);
    }
}

}  // namespace nwwav
}  // namespace vga

// ---------------------------------------------------------------- host side
struct vga_nwwav_bank {
    struct Row { int file, channel, codec, samples; int64_t offset; };   // offset: bytes (GC, PCM8) or samples (PCM16)
    std::vector<Row> rows;
    std::vector<int16_t> coefs, hist1, hist2, gain;         // of the GC rows
    int count[3] = {0, 0, 0};
    int64_t out_bytes[3] = {0, 0, 0}, source_bytes = 0;
    void *d_tables = nullptr;
    const nwwav::Piece *d_pieces = nullptr;
    const uint32_t *d_groups = nullptr;
    int groups = 0, device = 0;
};

extern "C" {

int vga_nwwav_parse(const uint8_t *file, size_t size, vga_nwwav_info *out)
{
    if (!file || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    nwwav::Failure f;
    const int rc = nwwav::parse(file, size, out, &f);
    if (rc) set_error("%s", f.msg);
    return rc;
}

int vga_nwwav_read(const uint8_t *file, size_t size, const vga_nwwav_info *I, uint8_t *const *out)
{
    if (!file || !I || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (I->channel_count < 1 || I->channel_count > VGA_NW_MAX_CHANNELS || I->channel_bytes < 0) { set_error("info does not describe a file"); return VGA_ERR_ARGUMENT; }
    for (int c = 0; c < I->channel_count; c++) {
        if (!out[c]) { set_error("channel %d: null pointer", c); return VGA_ERR_ARGUMENT; }
        if (nwwav::read_channel(file, size, I, c, out[c])) { set_error("info does not describe this file"); return VGA_ERR_ARGUMENT; }
    }
    return VGA_OK;
}

int vga_nwwav_bank_create(const vga_nwwav_info *infos, const int64_t *file_offsets, int nfiles, vga_nwwav_bank **out)
{
    using nwwav::Piece;
    if (!out) { set_error("null output"); return VGA_ERR_ARGUMENT; }
    *out = nullptr;
    if (!infos || !file_offsets || nfiles < 1) { set_error("a bank takes at least one parsed file and its offset"); return VGA_ERR_ARGUMENT; }
    for (int f = 0; f < nfiles; f++) {
        const vga_nwwav_info &I = infos[f];
        const bool prefetch = I.kind == VGA_NWWAV_CSTP || I.kind == VGA_NWWAV_FSTP;
        bool ok = file_offsets[f] >= 0 && I.kind >= VGA_NWWAV_RWAV && I.kind <= VGA_NWWAV_FSTP && I.codec >= 0 && I.codec <= 2 &&
                  I.channel_count >= 1 && I.channel_count <= VGA_NW_MAX_CHANNELS && I.sample_count >= 0 &&
                  I.channel_bytes == nwwav::samples_to_bytes(I.sample_count, I.codec);
        if (ok && prefetch)
            ok = I.interleave_size > 0 && I.prefetch_size >= 0 && I.prefetch_audio_offset >= 0 &&
                 I.channel_bytes <= I.prefetch_size / I.channel_count;
        for (int c = 0; ok && !prefetch && c < I.channel_count; c++) ok = I.audio_offset[c] >= 0;
        if (!ok) { set_error("file %d: not an info of vga_nwwav_parse, or a negative offset", f); return VGA_ERR_ARGUMENT; }
    }
    if (int rc = require_device()) return rc;
    vga_nwwav_bank *b = new vga_nwwav_bank;
    std::vector<Piece> pieces;
    int64_t end[3] = {0, 0, 0};                             // bytes
    for (int f = 0; f < nfiles; f++) {
        const vga_nwwav_info &I = infos[f];
        const bool prefetch = I.kind >= VGA_NWWAV_CSTP;
        const int o = I.codec;
        for (int c = 0; c < I.channel_count; c++) {
            b->rows.push_back({f, c, o, I.sample_count, o == VGA_NW_CODEC_PCM16 ? end[o] / 2 : end[o]});
            b->count[o]++;
            if (o == VGA_NW_CODEC_GCADPCM) {
                b->coefs.insert(b->coefs.end(), I.coefs[c], I.coefs[c] + 16);
                b->hist1.push_back(I.start_context[c][1]);
                b->hist2.push_back(I.start_context[c][2]);
                b->gain.push_back(I.gain[c]);
            }
            const int64_t n = I.channel_bytes, padded = round_up(n, 16);
            const int64_t src = file_offsets[f] + (prefetch ? I.prefetch_audio_offset : I.audio_offset[c]);
            if (n > 0) b->source_bytes = std::max(b->source_bytes, prefetch ? src + I.prefetch_size : src + n);
            for (int64_t at = 0; at < padded; at += nwwav::kPieceBytes) {
                Piece p{};
                p.total = (uint32_t)std::min<int64_t>(nwwav::kPieceBytes, padded - at);
                p.copy = (uint32_t)std::min<int64_t>(p.total, n - at);
                p.dst = end[o] + at;
                p.flags = (uint32_t)o;
                // the swap of ToShortArray(structure.Endianness) (Common.cs:102): the host is little-endian
                if (o == VGA_NW_CODEC_PCM16 && I.endianness == VGA_NW_BIG_ENDIAN) p.flags |= nwwav::kSwap16;
                if (prefetch) {
                    p.flags |= nwwav::kPrefetch;
                    p.src = src;
                    p.il = (uint32_t)I.interleave_size;
                    p.in = (uint32_t)(I.prefetch_size / I.channel_count);
                    p.pos0 = (uint32_t)at;
                    p.nch = (uint32_t)I.channel_count;
                    p.c = (uint32_t)c;
                } else
                    p.src = src + at;
                pieces.push_back(p);
            }
            end[o] += padded;
        }
    }
    if (b->count[VGA_NW_CODEC_GCADPCM]) {                   // the ragged decoder's guard: one piece of zeros
        Piece p{};
        p.dst = end[VGA_NW_CODEC_GCADPCM];
        p.total = (uint32_t)nwwav::kGuardBytes;
        p.flags = VGA_NW_CODEC_GCADPCM;
        pieces.push_back(p);
        end[VGA_NW_CODEC_GCADPCM] += nwwav::kGuardBytes;
    }
    for (int o = 0; o < 3; o++) b->out_bytes[o] = end[o];
    // groups: a piece above a quarter of kPieceBytes alone (all four waves share it); smaller ones that follow each
    // other together, up to one piece's bytes and kMaxGroupPieces of them per workgroup (one wave each in turn)
    std::vector<uint32_t> groups{0};
    uint32_t held = 0, n_held = 0;
    for (size_t i = 0; i < pieces.size(); i++) {
        const bool alone = pieces[i].total > nwwav::kPieceBytes / 4 || (i > 0 && pieces[i - 1].total > nwwav::kPieceBytes / 4);
        if (n_held && (alone || held + pieces[i].total > nwwav::kPieceBytes || n_held == (uint32_t)nwwav::kMaxGroupPieces)) {
            groups.push_back((uint32_t)i);
            held = n_held = 0;
        }
        held += pieces[i].total;
        n_held++;
    }
    if (n_held) groups.push_back((uint32_t)pieces.size());
    b->groups = (int)groups.size() - 1;
    (void)hipGetDevice(&b->device);
    const size_t piece_bytes = pieces.size() * sizeof(Piece), bytes = piece_bytes + groups.size() * 4;
    hipError_t e = device_malloc(&b->d_tables, bytes);
    if (e == hipSuccess && piece_bytes) e = hipMemcpy(b->d_tables, pieces.data(), piece_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(static_cast<uint8_t *>(b->d_tables) + piece_bytes, groups.data(), groups.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (b->d_tables) (void)hipFree(b->d_tables);
        delete b;
        set_error("bank tables: %s", hipGetErrorString(e));
        return VGA_ERR_DEVICE;
    }
    b->d_pieces = static_cast<const Piece *>(b->d_tables);
    b->d_groups = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(b->d_tables) + piece_bytes);
    *out = b;
    return VGA_OK;
}

void vga_nwwav_bank_destroy(vga_nwwav_bank *b)
{
    if (!b) return;
    if (b->d_tables) (void)hipFree(b->d_tables);
    delete b;
}

int vga_nwwav_bank_channels(const vga_nwwav_bank *b) { return b ? (int)b->rows.size() : 0; }
int vga_nwwav_bank_codec_channels(const vga_nwwav_bank *b, int codec) { return b && codec >= 0 && codec <= 2 ? b->count[codec] : 0; }

int vga_nwwav_bank_rows(const vga_nwwav_bank *b, int *file_out, int *channel_out, int *codec_out, int *sample_counts_out, int64_t *offsets_out)
{
    if (!b) { set_error("null bank"); return VGA_ERR_ARGUMENT; }
    for (size_t i = 0; i < b->rows.size(); i++) {
        const vga_nwwav_bank::Row &r = b->rows[i];
        if (file_out) file_out[i] = r.file;
        if (channel_out) channel_out[i] = r.channel;
        if (codec_out) codec_out[i] = r.codec;
        if (sample_counts_out) sample_counts_out[i] = r.samples;
        if (offsets_out) offsets_out[i] = r.offset;
    }
    return VGA_OK;
}

int vga_nwwav_bank_gc_sample_counts(const vga_nwwav_bank *b, int *sample_counts_out)
{
    if (!b || !sample_counts_out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    for (const vga_nwwav_bank::Row &r : b->rows)
        if (r.codec == VGA_NW_CODEC_GCADPCM) *sample_counts_out++ = r.samples;
    return VGA_OK;
}

int vga_nwwav_bank_gc_tables(const vga_nwwav_bank *b, int16_t *coefs_out, int16_t *hist1_out, int16_t *hist2_out, int16_t *gain_out)
{
    if (!b) { set_error("null bank"); return VGA_ERR_ARGUMENT; }
    if (coefs_out) std::copy(b->coefs.begin(), b->coefs.end(), coefs_out);
    if (hist1_out) std::copy(b->hist1.begin(), b->hist1.end(), hist1_out);
    if (hist2_out) std::copy(b->hist2.begin(), b->hist2.end(), hist2_out);
    if (gain_out) std::copy(b->gain.begin(), b->gain.end(), gain_out);
    return VGA_OK;
}

int64_t vga_nwwav_bank_adpcm_bytes(const vga_nwwav_bank *b) { return b ? b->out_bytes[VGA_NW_CODEC_GCADPCM] : 0; }
int64_t vga_nwwav_bank_pcm16_samples(const vga_nwwav_bank *b) { return b ? b->out_bytes[VGA_NW_CODEC_PCM16] / 2 : 0; }
int64_t vga_nwwav_bank_pcm8_bytes(const vga_nwwav_bank *b) { return b ? b->out_bytes[VGA_NW_CODEC_PCM8] : 0; }
int64_t vga_nwwav_bank_source_bytes(const vga_nwwav_bank *b) { return b ? b->source_bytes : 0; }

int vga_nwwav_bank_read_device(const vga_nwwav_bank *b, const uint8_t *d_files, uint8_t *d_adpcm, int16_t *d_pcm16, uint8_t *d_pcm8,
                               void *stream)
{
    if (!b) { set_error("null bank"); return VGA_ERR_ARGUMENT; }
    const void *outs[3] = {d_pcm8, d_pcm16, d_adpcm};       // by NwCodec
    for (int o = 0; o < 3; o++) {
        if (b->out_bytes[o] > 0 && !outs[o]) { set_error("null device buffer for codec %d rows", o); return VGA_ERR_ARGUMENT; }
        if ((uintptr_t)outs[o] & 15) { set_error("device buffers must be 16-byte aligned"); return VGA_ERR_ARGUMENT; }
    }
    if (b->source_bytes > 0 && !d_files) { set_error("null file buffer"); return VGA_ERR_ARGUMENT; }
    int device = -1;
    (void)hipGetDevice(&device);
    if (device != b->device) { set_error("the bank was created on device %d, the current one is %d", b->device, device); return VGA_ERR_ARGUMENT; }
    if (b->groups == 0) return VGA_OK;
    hipLaunchKernelGGL(nwwav::bank_read_kernel, dim3(b->groups), dim3(nwwav::kThreads), 0, (hipStream_t)stream, b->d_pieces, b->d_groups,
                       d_files, d_adpcm, reinterpret_cast<uint8_t *>(d_pcm16), d_pcm8);
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

}  // extern "C"
