// adx_span.hpp -- ADX audio of 18-byte frames between an image (one frame per channel in turn, AdxWriter.WriteData :119-131 /
// AdxReader.ReadData :116-124) and one row per channel, a SPAN of frames per workgroup through LDS.  18 and 16 share no
// divisor above 2 and the audio offset has any alignment, so a copy straight between image and rows moves 2-byte granules at
// best (the general paths).  Here the span is loaded with aligned 16-byte vectors (the ragged ends byte by byte), and every
// thread assembles 16-byte granules of the other side from LDS and stores them aligned.  A span holds a multiple of 8 frames
// per channel, so every span starts its rows on a 16-byte boundary (8 * 18 = 144 = 9 * 16).
// The figures are plain constants for host code (adx_files_host.hpp cuts work items by them); the bodies are device
// functions that the per-file reader (container_readers.hip) and the kernels of a set of files (adx_files_kernels.hip) call.
#pragma once
#include <cstdint>

namespace vga {
namespace adxspan {

constexpr int kFrame = 18;
constexpr int kSpanBytes = 16384;             // LDS per workgroup for the span (plus 32 bytes of alignment slack)
constexpr int kLdsBytes = kSpanBytes + 32;
constexpr int kMaxChannels = kSpanBytes / (kFrame * 8);   // 113: a span must hold 8 frames per channel
constexpr int kThreads = 256;

// frames per channel of one span of a file of nch channels (nch <= kMaxChannels)
constexpr int span_frames(int nch) { return kSpanBytes / (kFrame * nch) / 8 * 8; }

#ifdef __HIPCC__

// What a span body does to the frames it holds in LDS, between its load and its store phase.  NoCipher: nothing, and no
// code.  A cipher with active == true is called by every thread as cipher(nch, k0, nk, frame_at) -- frame_at(fr, c): the 18
// bytes of frame k0 + fr of channel c in LDS -- and a second barrier follows it (adx_keyed_files_kernels.hip).
struct NoCipher { static constexpr bool active = false; };

// image -> rows.  base: the image's audio (any alignment), frame_count frames per channel: nothing outside is read.
// Frames k0 .. k0 + span - 1 (or to the end) go to row_of(c) + k0 * 18; rows are 16-byte aligned.
template <class RowOf, class Cipher = NoCipher>
__device__ __forceinline__ void deinterleave_span(uint8_t *__restrict__ lds, const uint8_t *__restrict__ base, int nch, int frame_count,
                                                  int k0, int span, RowOf row_of, Cipher cipher = Cipher())
{
    const int64_t audio = (int64_t)frame_count * kFrame * nch;
    const int nk = min(span, frame_count - k0);
    const int64_t span0 = (int64_t)k0 * kFrame * nch, span1 = span0 + (int64_t)nk * kFrame * nch;
    const int mis = (int)((uintptr_t)(base + span0) & 15);            // LDS byte 0 is audio byte span0 - mis
    const int64_t x0 = span0 - mis;
    const int granules = (int)((span1 - x0 + 15) >> 4);
    for (int g = threadIdx.x; g < granules; g += kThreads) {
        const int64_t x = x0 + 16 * (int64_t)g;
        uint4 v;
        if (x >= 0 && x + 16 <= audio) {
            v = *reinterpret_cast<const uint4 *>(base + x);
        } else {
            uint8_t t[16];
#pragma unroll
            for (int k = 0; k < 16; k++) t[k] = x + k >= 0 && x + k < audio ? base[x + k] : 0;
            memcpy(&v, t, 16);
        }
        *reinterpret_cast<uint4 *>(lds + 16 * g) = v;
    }
    __syncthreads();
    if constexpr (Cipher::active) {
        cipher(nch, k0, nk, [&](int fr, int c) { return lds + mis + (fr * nch + c) * kFrame; });
        __syncthreads();
    }
    const int row_bytes = nk * kFrame;
    const int per_row = (row_bytes + 15) >> 4;
    for (int q = threadIdx.x; q < per_row * nch; q += kThreads) {
        const int c = q / per_row, j0 = (q - c * per_row) * 16;
        const int fr = j0 / kFrame, w = j0 - fr * kFrame;
        const int n1 = min(16, kFrame - w);                            // bytes from frame fr, the rest from frame fr + 1
        const int o1 = mis + (fr * nch + c) * kFrame + w, o2 = mis + ((fr + 1) * nch + c) * kFrame - n1;
        const int avail = min(16, row_bytes - j0);
        uint8_t t[16];
#pragma unroll
        for (int k = 0; k < 16; k++) t[k] = k < avail ? lds[k < n1 ? o1 + k : o2 + k] : 0;
        uint8_t *d = row_of(c) + (int64_t)k0 * kFrame + j0;
        if (avail == 16) {
            uint4 v;
            memcpy(&v, t, 16);
            *reinterpret_cast<uint4 *>(d) = v;
        } else {
            for (int k = 0; k < avail; k++) d[k] = t[k];
        }
    }
}

// rows -> image, the mirror image.  Frames k0 .. k0 + span - 1 (or to frame_count) of every row (row_of(c), 16-byte aligned;
// the vector that holds a row's last bytes may reach up to 15 bytes behind them: packed rows are rounded up to 16 and a guard
// follows the last) go to out + k0 * 18 * nch, `out` the image's audio at any alignment.  In LDS row c's part of the span
// lies at c * pitch.  The output's 16-byte granules are those of the image's own address grid: the bytes in front of the first
// whole one and behind the last go out singly; a granule takes its bytes from at most two (frame, channel) runs, since a
// run is 18 bytes.
template <class RowOf, class Cipher = NoCipher>
__device__ __forceinline__ void interleave_span(uint8_t *__restrict__ lds, RowOf row_of, int nch, int frame_count, int k0, int span,
                                                uint8_t *__restrict__ out, Cipher cipher = Cipher())
{
    const int nk = min(span, frame_count - k0);
    const int row_bytes = nk * kFrame;
    const int per_row = (row_bytes + 15) >> 4, pitch = per_row * 16;  // nch * pitch <= nch * span * 18 <= kSpanBytes
    for (int q = threadIdx.x; q < per_row * nch; q += kThreads) {
        const int c = q / per_row, g = q - c * per_row;
        *reinterpret_cast<uint4 *>(lds + c * pitch + 16 * g) = *reinterpret_cast<const uint4 *>(row_of(c) + (int64_t)k0 * kFrame + 16 * g);
    }
    __syncthreads();
    if constexpr (Cipher::active) {
        cipher(nch, k0, nk, [&](int fr, int c) { return lds + c * pitch + fr * kFrame; });
        __syncthreads();
    }
    const int group = kFrame * nch, total = nk * group;               // bytes of one frame of all channels; of the span
    uint8_t *d = out + (int64_t)k0 * group;
    const int lead = min((int)((16 - ((uintptr_t)d & 15)) & 15), total);
    const int granules = (total - lead) >> 4, tail0 = lead + 16 * granules;
    auto byte_at = [&](int o) {
        const int fr = o / group, r = o - fr * group, c = r / kFrame;
        return lds[c * pitch + fr * kFrame + (r - c * kFrame)];
    };
    for (int o = threadIdx.x; o < lead; o += kThreads) d[o] = byte_at(o);
    for (int o = tail0 + threadIdx.x; o < total; o += kThreads) d[o] = byte_at(o);
    for (int g = threadIdx.x; g < granules; g += kThreads) {
        const int o = lead + 16 * g;
        const int fr = o / group, r = o - fr * group, c = r / kFrame, w = r - c * kFrame;
        const int n1 = min(16, kFrame - w);                            // bytes from (fr, c), the rest from the run behind it
        const bool wrap = c + 1 == nch;
        const int o1 = c * pitch + fr * kFrame + w;
        const int o2 = (wrap ? 0 : c + 1) * pitch + (wrap ? fr + 1 : fr) * kFrame - n1;
        uint8_t t[16];
#pragma unroll
        for (int k = 0; k < 16; k++) t[k] = lds[k < n1 ? o1 + k : o2 + k];
        uint4 v;
        memcpy(&v, t, 16);
        *reinterpret_cast<uint4 *>(d + o) = v;
    }
}

#endif  // __HIPCC__

}  // namespace adxspan
}  // namespace vga
