// wave_files_kernels.hip -- the kernels of include/vgaudio_hip_files/wave_files.h: the data chunks of a SET of WAVE files of
// different shapes taken apart into planar int16 rows and put together from them, every kernel one launch over tables the
// set's object holds (wave_files_host.hpp).
//
//   wave_files_header_kernel       one workgroup per file copies the header the host laid out at create
//   wave_files_read_tile_kernel, wave_files_write_tile_kernel
//                                  frames of at most 2048 bytes: (file, span of F frames) items through LDS.  The INTERLEAVED
//                                  side moves 16-byte vectors at aligned ADDRESSES (the span's first byte sits at LDS position
//                                  r = address mod 16; the bytes of a vector that is not wholly the span's go singly), the
//                                  PLANAR side 8 samples of one row per lane, as one 16-byte vector where the row's address
//                                  allows.  Both sides address the LDS through lds_at / Walk below.
//   wave_files_read_kernel, wave_files_write_kernel
//                                  every other file: one thread per granule of the OUTPUT (8 samples of a row; 16 bytes of the
//                                  data chunk), gathered sample by sample, (row or file, chunk of 2048 granules) items, no LDS
// 8-bit files go through Pcm8Codec.Decode / Encode on the planar side (Pcm8Codec.cs:5-28).  All of it is byte movement:
// HBM-bound, every byte read once and written once.  All addressing into d_images and d_pcm is in 64 bits.
//
// THE LDS LAYOUT of a span.  Position p (0 .. r + span bytes) lies at byte  lds_at(p) = p + kPad * (p / P),  P = 8 frames'
// bytes: kPad = 4 bytes of padding behind every 8 frames.  On the planar side the 32 lanes of a bank group hold 32
// consecutive groups of 8 frames of one channel and read, sample by sample, addresses P + 4 bytes apart: 4 * nch + 1 dwords
// for 16-bit files, 2 * nch + 1 for 8-bit files, an ODD number, so the 32 lanes fall on 32 different banks of the 32
// ((a / 4) mod 32 for the 1-, 2- and 4-byte LDS accesses) whatever the channel count is.  Without the padding the distance
// is 4 * nch dwords and 32 lanes share 32 / gcd(4 * nch, 32) banks: 4-way conflicts for 1 channel, 8-way for 2 and for 6,
// 32-way for 8.  (A half that straddles two channels of a span -- 6 channels: 170 groups a channel -- meets 2-way there.)
// The padding costs the interleaved side its 16-byte LDS accesses: a vector goes as four dwords, in step k dword
// (k + interleaved_rot) mod 4.  Lane l's vector starts 4 l dwords in plus one dword per pad in front of it.  With P <= 256
// every lane moves dword k: the pads between the 32 vectors of a half spread them, enumerated (tools/wave_files_lds_conflicts.py)
// none for 1 and 8 channels of 16 bits, 2-way for 2 and 6 (ds_write_b32 hides 2-way behind its register transfer; the
// ds_read_b32 of the write kernel does not).  With P > 256 few or no pads fall inside a half's 512 bytes and a fixed dword
// is 3- to 4-way, so lane l moves dword (k + l / 8) mod 4 -- lanes 8 apart, whose vectors are 32 banks apart, take different
// dwords: at most 2-way.  Rotating at P <= 256 too would be WORSE (2, 3, 3, 2-way for 1, 2, 6, 8 channels).  DESIGN.md 4.6i
// has the table.  None of it is measured with counters.
#include "common.hpp"
#include "wave_files_kernels.hpp"

namespace vga {
namespace wavf {

constexpr uint32_t kPad = 4;
// positions run to 15 + SPAN_BYTES; the shortest period is 8 bytes (8-bit mono): half as much again
constexpr int kLdsBytes = (SPAN_BYTES + 16) / 8 * 12 + 16;

constexpr int kRounds = SPAN_BYTES / 16 / 256;             // rounds of the 256 lanes over a span's vectors

__device__ __forceinline__ uint32_t lds_at(uint32_t p, uint32_t P) { return p + kPad * (p / P); }

// the LDS addresses of one lane's samples on the planar side: position p0 + j * frame for j = 0, 1, ... (p0 = r + byte of the
// channel inside its frame + group * P), without a division per sample
struct Walk {
    uint32_t addr, rem, frame, P;
    __device__ __forceinline__ Walk(uint32_t within, uint32_t group, uint32_t frame_, uint32_t P_) : frame(frame_), P(P_)
    {
        const uint32_t q = within / P;
        rem = within - q * P;
        addr = within + group * P + kPad * (q + group);       // = lds_at(within + group * P, P)
    }
    __device__ __forceinline__ uint32_t next_byte() const { return addr + 1 + (rem + 1 == P ? kPad : 0); }   // of position p + 1
    __device__ __forceinline__ void step()
    {
        addr += frame;
        rem += frame;
        if (rem >= P) { rem -= P; addr += kPad; }
    }
};

__device__ __forceinline__ int16_t pcm8_decode(uint8_t b) { return (int16_t)((int8_t)(b ^ 0x80) * 256); }
__device__ __forceinline__ uint8_t pcm8_encode(int16_t s) { return (uint8_t)((s >> 8) ^ 0x80); }

__device__ __forceinline__ uint32_t pick(const uint4 &x, uint32_t i) { return i == 0 ? x.x : i == 1 ? x.y : i == 2 ? x.z : x.w; }
__device__ __forceinline__ void place(uint4 &x, uint32_t i, uint32_t v)
{
    if (i == 0) x.x = v; else if (i == 1) x.y = v; else if (i == 2) x.z = v; else x.w = v;
}
// the LDS address of dword i (0..3) of the vector at position p = 16 * v: q = p / P, rem = p mod P
__device__ __forceinline__ uint32_t lds_dword(uint32_t p, uint32_t q, uint32_t rem, uint32_t i, uint32_t P)
{
    const uint32_t at = rem + 4 * i;                           // < 2 * P: P >= 8 is a multiple of 8, and rem = 0 when P <= 16
    return p + 4 * i + kPad * (q + (at >= P ? 1 : 0));
}
// what a lane adds to the step number to get the dword of its vector it moves in that step (one value per workgroup's P)
__device__ __forceinline__ uint32_t interleaved_rot(uint32_t P) { return P > 256 ? threadIdx.x >> 3 : 0; }

__global__ __launch_bounds__(256) void wave_files_header_kernel(const FileTab *__restrict__ tab, const uint8_t *__restrict__ headers,
                                                                uint8_t *__restrict__ images)
{
    const FileTab &t = tab[blockIdx.x];
    const uint8_t *h = headers + (int64_t)blockIdx.x * HEADER_PITCH;
    uint8_t *image = images + t.image_off;
    for (int i = threadIdx.x; i < t.header_size; i += 256) image[i] = h[i];
}

// ---------------------------------------------------------------- the tile form
__global__ __launch_bounds__(256) void wave_files_read_tile_kernel(const FileTab *__restrict__ tab, const int64_t *__restrict__ row_off,
                                                                   const Item *__restrict__ items, const uint8_t *__restrict__ images,
                                                                   int16_t *__restrict__ pcm)
{
    __shared__ __align__(16) uint8_t lds[kLdsBytes];
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[it.x];
    const int nch = t.nch, bps = t.bps, first = (int)it.y;
    const int count = min(t.span_frames, t.frames - first);
    const uint32_t frame = (uint32_t)(nch * bps), P = 8 * frame, len = (uint32_t)count * frame;
    const uint8_t *src = images + t.data_at + (int64_t)first * frame;
    const uint32_t r = (uint32_t)((uintptr_t)src & 15);
    const uint8_t *base = src - r;                             // aligned; nothing in front of src is read
    // interleaved side: aligned vectors that are wholly the span's, the bytes of the others singly.  The loads of kRounds rounds
    // of the 256 lanes are issued before the first of them is used; r pushes at most one vector behind them.
    const uint32_t rot = interleaved_rot(P);
    auto whole = [&](uint32_t p) { return p >= r && p + 16 <= r + len; };
    auto to_lds = [&](uint32_t p, const uint4 &x) {
        const uint32_t q = p / P, rem = p - q * P;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t i = (k + rot) & 3;
            *reinterpret_cast<uint32_t *>(lds + lds_dword(p, q, rem, i, P)) = pick(x, i);
        }
    };
    auto bytes_to_lds = [&](uint32_t p) {
        for (uint32_t b = max(p, r); b < min(p + 16, r + len); b++) lds[lds_at(b, P)] = base[b];
    };
    uint4 x[kRounds];
#pragma unroll
    for (int k = 0; k < kRounds; k++) {
        const uint32_t p = 16 * (threadIdx.x + 256 * k);
        if (whole(p)) x[k] = *reinterpret_cast<const uint4 *>(base + p);
    }
#pragma unroll
    for (int k = 0; k < kRounds; k++) {
        const uint32_t p = 16 * (threadIdx.x + 256 * k);
        if (whole(p)) to_lds(p, x[k]);
        else bytes_to_lds(p);
    }
    for (uint32_t p = 16 * (threadIdx.x + 256 * kRounds); p < r + len; p += 16 * 256) {
        if (whole(p)) to_lds(p, *reinterpret_cast<const uint4 *>(base + p));
        else bytes_to_lds(p);
    }
    __syncthreads();
    // planar side: lane = (channel, group of 8 frames), neighbouring lanes neighbouring groups of one row
    const int groups = (count + 7) / 8;
    const bool odd = (r & 1) != 0;
    for (int e = threadIdx.x; e < groups * nch; e += 256) {
        const int c = e / groups, g = e - c * groups;
        const int n = min(8, count - 8 * g);
        Walk w(r + (uint32_t)(c * bps), (uint32_t)g, frame, P);
        uint16_t s[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            s[j] = 0;
            if (j < n) {
                if (bps == 1) s[j] = (uint16_t)pcm8_decode(lds[w.addr]);
                else if (!odd) s[j] = *reinterpret_cast<const uint16_t *>(lds + w.addr);
                else s[j] = (uint16_t)(lds[w.addr] | (lds[w.next_byte()] << 8));
                w.step();
            }
        }
        int16_t *row = pcm + row_off[t.first_channel + c] + first + 8 * g;
        if (n == 8 && ((uintptr_t)row & 15) == 0) {
            *reinterpret_cast<uint4 *>(row) = make_uint4(s[0] | ((uint32_t)s[1] << 16), s[2] | ((uint32_t)s[3] << 16),
                                                         s[4] | ((uint32_t)s[5] << 16), s[6] | ((uint32_t)s[7] << 16));
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (j < n) row[j] = (int16_t)s[j];
        }
    }
}

__global__ __launch_bounds__(256) void wave_files_write_tile_kernel(const FileTab *__restrict__ tab, const int64_t *__restrict__ row_off,
                                                                    const Item *__restrict__ items, const int16_t *__restrict__ pcm,
                                                                    uint8_t *__restrict__ images)
{
    __shared__ __align__(16) uint8_t lds[kLdsBytes];
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[it.x];
    const int nch = t.nch, bps = t.bps, first = (int)it.y;
    const int count = min(t.span_frames, t.frames - first);
    const uint32_t frame = (uint32_t)(nch * bps), P = 8 * frame, len = (uint32_t)count * frame;
    uint8_t *dst = images + t.data_at + (int64_t)first * frame;
    const uint32_t r = (uint32_t)((uintptr_t)dst & 15);
    uint8_t *base = dst - r;                                   // aligned; nothing in front of dst is written
    // planar side: the row loads of kRounds rounds of the 256 lanes are issued before the first of them is used
    const int groups = (count + 7) / 8, lanes = groups * nch;
    const bool odd = (r & 1) != 0;
    for (int e0 = 0; e0 < lanes; e0 += 256 * kRounds) {
        uint4 x[kRounds];
        const int16_t *row[kRounds];
        int n[kRounds];
#pragma unroll
        for (int k = 0; k < kRounds; k++) {
            const int e = e0 + 256 * k + (int)threadIdx.x;
            n[k] = 0;
            if (e < lanes) {
                const int c = e / groups, g = e - c * groups;
                n[k] = min(8, count - 8 * g);
                row[k] = pcm + row_off[t.first_channel + c] + first + 8 * g;
                if (n[k] == 8 && ((uintptr_t)row[k] & 15) == 0) x[k] = *reinterpret_cast<const uint4 *>(row[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < kRounds; k++) {
            const int e = e0 + 256 * k + (int)threadIdx.x;
            if (n[k] == 0) continue;
            const int c = e / groups, g = e - c * groups;
            uint16_t s[8];
            if (n[k] == 8 && ((uintptr_t)row[k] & 15) == 0) {
                s[0] = (uint16_t)x[k].x; s[1] = (uint16_t)(x[k].x >> 16); s[2] = (uint16_t)x[k].y; s[3] = (uint16_t)(x[k].y >> 16);
                s[4] = (uint16_t)x[k].z; s[5] = (uint16_t)(x[k].z >> 16); s[6] = (uint16_t)x[k].w; s[7] = (uint16_t)(x[k].w >> 16);
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++) s[j] = j < n[k] ? (uint16_t)row[k][j] : 0;
            }
            Walk w(r + (uint32_t)(c * bps), (uint32_t)g, frame, P);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (j < n[k]) {
                    if (bps == 1) lds[w.addr] = pcm8_encode((int16_t)s[j]);
                    else if (!odd) *reinterpret_cast<uint16_t *>(lds + w.addr) = s[j];
                    else { lds[w.addr] = (uint8_t)s[j]; lds[w.next_byte()] = (uint8_t)(s[j] >> 8); }
                    w.step();
                }
            }
        }
    }
    __syncthreads();
    // interleaved side
    const uint32_t nvec = (r + len + 15) / 16, rot = interleaved_rot(P);
    for (uint32_t v = threadIdx.x; v < nvec; v += 256) {
        const uint32_t p = 16 * v;
        if (p >= r && p + 16 <= r + len) {
            const uint32_t q = p / P, rem = p - q * P;
            uint4 x;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t i = (k + rot) & 3;
                place(x, i, *reinterpret_cast<const uint32_t *>(lds + lds_dword(p, q, rem, i, P)));
            }
            *reinterpret_cast<uint4 *>(base + p) = x;
        } else {
            for (uint32_t b = max(p, r); b < min(p + 16, r + len); b++) base[b] = lds[lds_at(b, P)];
        }
    }
}

// ---------------------------------------------------------------- the general form
// InterleavedByteToShort (Interleave.cs:188-207) / DeInterleave(1, nch) + Pcm8Codec.Decode: sample i of channel c is at byte
// (i * nch + c) * bps of the data chunk
__global__ __launch_bounds__(256) void wave_files_read_kernel(const FileTab *__restrict__ tab, const int64_t *__restrict__ row_off,
                                                              const int *__restrict__ row_file, const Item *__restrict__ items,
                                                              const uint8_t *__restrict__ images, int16_t *__restrict__ pcm)
{
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[row_file[it.x]];
    const int c = it.x - t.first_channel, nch = t.nch, bps = t.bps;
    const uint8_t *in = images + t.data_at;
    int16_t *row = pcm + row_off[it.x];
#pragma unroll 1
    for (int k = 0; k < CHUNK_GRANULES / 256; k++) {
        const int64_t i0 = ((int64_t)it.y * CHUNK_GRANULES + k * 256 + threadIdx.x) * 8;
        if (i0 >= t.frames) return;
        const int n = (int)min((int64_t)8, t.frames - i0);
        uint16_t s[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            s[j] = 0;
            if (j < n) {
                const uint8_t *at = in + ((i0 + j) * nch + c) * bps;
                s[j] = bps == 1 ? (uint16_t)pcm8_decode(at[0]) : (uint16_t)(at[0] | (at[1] << 8));
            }
        }
        int16_t *out = row + i0;
        if (n == 8 && ((uintptr_t)out & 15) == 0) {
            *reinterpret_cast<uint4 *>(out) = make_uint4(s[0] | ((uint32_t)s[1] << 16), s[2] | ((uint32_t)s[3] << 16),
                                                         s[4] | ((uint32_t)s[5] << 16), s[6] | ((uint32_t)s[7] << 16));
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (j < n) out[j] = (int16_t)s[j];
        }
    }
}

// ShortToInterleavedByte (Interleave.cs:168-186) / Pcm8Codec.Encode + Interleave(stream, 1): 16 bytes of the data chunk per
// thread, counted from the chunk's start
__global__ __launch_bounds__(256) void wave_files_write_kernel(const FileTab *__restrict__ tab, const int64_t *__restrict__ row_off,
                                                               const Item *__restrict__ items, const int16_t *__restrict__ pcm,
                                                               uint8_t *__restrict__ images)
{
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[it.x];
    const int nch = t.nch, bps = t.bps, frame = nch * bps;
    const int64_t total = (int64_t)t.frames * frame;
    const int64_t *rows = row_off + t.first_channel;
    uint8_t *data = images + t.data_at;
#pragma unroll 1
    for (int q = 0; q < CHUNK_GRANULES / 256; q++) {
        const int64_t o = ((int64_t)it.y * CHUNK_GRANULES + q * 256 + threadIdx.x) * GRANULE_BYTES;
        if (o >= total) return;
        const int n = (int)min((int64_t)GRANULE_BYTES, total - o);
        int64_t fr = o / frame;
        const int within = (int)(o - fr * frame);
        int c = within / bps, k = within - c * bps;
        uint32_t x[4] = {0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < GRANULE_BYTES; b++) {
            if (b < n) {
                const int16_t s = pcm[rows[c] + fr];
                const uint32_t byte = bps == 1 ? pcm8_encode(s) : (uint32_t)((uint16_t)s >> (8 * k)) & 0xFF;
                x[b / 4] |= byte << (8 * (b % 4));
                if (++k == bps) {
                    k = 0;
                    if (++c == nch) { c = 0; fr++; }
                }
            }
        }
        uint8_t *out = data + o;
        if (n == GRANULE_BYTES && ((uintptr_t)out & 15) == 0) {
            *reinterpret_cast<uint4 *>(out) = make_uint4(x[0], x[1], x[2], x[3]);
        } else if (((uintptr_t)out & 3) == 0) {
#pragma unroll
            for (int d = 0; d < 4; d++) {
                if (4 * d + 4 <= n) *reinterpret_cast<uint32_t *>(out + 4 * d) = x[d];
                else
                    for (int b = 4 * d; b < min(n, 4 * d + 4); b++) out[b] = (uint8_t)(x[d] >> (8 * (b % 4)));
            }
        } else {
#pragma unroll
            for (int b = 0; b < GRANULE_BYTES; b++)
                if (b < n) out[b] = (uint8_t)(x[b / 4] >> (8 * (b % 4)));
        }
    }
}

// ---------------------------------------------------------------- launchers
int launch_write_images(const DeviceTables &t, bool general, const int16_t *d_pcm, uint8_t *d_images, hipStream_t stream)
{
    if (t.files <= 0) return VGA_OK;
    const int k = general ? 1 : 0, tile = general ? 0 : t.tile_items, rest = t.item_count[k] - tile;
    hipLaunchKernelGGL(wave_files_header_kernel, dim3(t.files), dim3(256), 0, stream, t.tab, t.headers, d_images);
    VGA_HIP_TRY(hipGetLastError());
    if (tile > 0) {
        hipLaunchKernelGGL(wave_files_write_tile_kernel, dim3(tile), dim3(256), 0, stream, t.tab, t.row_off, t.items[k], d_pcm, d_images);
        VGA_HIP_TRY(hipGetLastError());
    }
    if (rest > 0) {
        hipLaunchKernelGGL(wave_files_write_kernel, dim3(rest), dim3(256), 0, stream, t.tab, t.row_off, t.items[k] + tile, d_pcm, d_images);
        VGA_HIP_TRY(hipGetLastError());
    }
    return VGA_OK;
}

int launch_read_images(const DeviceTables &t, bool general, const uint8_t *d_images, int16_t *d_pcm, hipStream_t stream)
{
    if (t.channels <= 0) return VGA_OK;
    const int k = general ? 1 : 0, tile = general ? 0 : t.tile_items, rest = t.item_count[k] - tile;
    if (tile > 0) {
        hipLaunchKernelGGL(wave_files_read_tile_kernel, dim3(tile), dim3(256), 0, stream, t.tab, t.row_off, t.items[k], d_images, d_pcm);
        VGA_HIP_TRY(hipGetLastError());
    }
    if (rest > 0) {
        hipLaunchKernelGGL(wave_files_read_kernel, dim3(rest), dim3(256), 0, stream, t.tab, t.row_off, t.row_file, t.items[k] + tile,
                           d_images, d_pcm);
        VGA_HIP_TRY(hipGetLastError());
    }
    return VGA_OK;
}

}  // namespace wavf
}  // namespace vga
