// hca_keyed_walk.hpp -- CriHcaEncryption.TestKey's view of ONE frame under ONE candidate key, once for the kernels of
// hca_keyed_files_kernels.hip and for host code (tests/host/hca_keyed_files_host_driver.cpp): CriHcaPacking.UnpackFrame for
// validity only (CriHcaPacking.cs:10-15, :71-237 -- UnpackFrameHeader, ReadScaleFactors / DeltaDecode, the code LENGTHS of
// ReadSpectralCoefficients, UnpackingWasSuccessful).  Free of <hip/hip_runtime.h>; a HIP compiler sees __host__ __device__.
//
// The walk is a template over two policies:
//   Bytes  unsigned plain(int i): byte i of the DECRYPTED frame, 0 <= i < frame_size - 2 (the stored byte through the
//          candidate's substitution table: LDS, global memory or a host array)
//   Res    the resolutions of the frame, 0..15 each, eight to a 32-bit word: put(c, w, word) / word(c, w) for channel c, word
//          w = band / 8.  No array is indexed per lane in private memory: the kernels keep the words in LDS.
// THE CRC.  CryptFrame refreshes the last two bytes with the CRC-16 of the decrypted bytes in front, and the bit reader CAN
// reach them: a code is peeked at its longest length and advanced by its own, so a peek that starts 18 bits before the end
// reads two CRC bits and may still leave the 16 .. 128 remaining bits that pass.  The verdict can depend on them, so they
// are computed -- lazily, by the first read that touches byte frame_size - 2: most walks end far in front of it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VGA_HCAK_HD __host__ __device__ __forceinline__
#else
#define VGA_HCAK_HD inline
#endif

namespace vga {
namespace hcak {

constexpr int FRAMES_TO_TEST = 10;               // CriHcaEncryption.FramesToTest
enum { FRAME_FAILS = 0, FRAME_PASSES = 1, FRAME_BAD_SYNC = 2 };     // one frame; and one candidate over its frames

// the tables the walk reads (208 bytes): QuantizedSpectrumBits, QuantizedSpectrumMaxBits, ScaleToResolutionCurve
struct WalkTables {
    uint8_t dec_bits[8][16];
    uint8_t max_bits[16];
    uint8_t res_curve[64];
};

// what the search needs of one file: one per file of a set made from parsed headers, in the object's device tables
struct WalkFile {
    int64_t frames_off;                          // of frame 0, in bytes from d_images
    int frame_size, frame_count;
    int encryption_type;
    int usable;                                  // 0: hca::make_device_info refuses the header (the search refuses a type-56 file)
    int nch;
    uint8_t coded_count[8];                      // at most 128
    uint8_t skip_bits[8];                        // behind a channel's scale factors: 32 (stereo secondary), 6 per HFR group, or 0
    uint8_t ath_curve[128];
};

// CriHcaPacking.cs:60-69
VGA_HCAK_HD int walk_resolution(const WalkTables &T, int scale_factor, int noise_level)
{
    if (scale_factor == 0) return 0;
    int p = noise_level - 5 * scale_factor / 2 + 2;
    p = p < 0 ? 0 : (p > 58 ? 58 : p);
    return T.res_curve[p];
}

// BitReader.PeekInt / ReadInt (BitReader.cs:51-92) over the decrypted frame, for reads of at most 16 bits
template <class Bytes>
struct WalkReader {
    Bytes &src;
    int frame_size, frame_bits, pos, crc;        // crc < 0: not computed yet
    VGA_HCAK_HD unsigned byte_at(int i)
    {
        if (i >= frame_size) return 0;
        if (i < frame_size - 2) return src.plain(i);
        if (crc < 0) {                           // Crc16.Compute (polynomial 0x8005, MSB first, from 0) over the decrypted bytes
            unsigned c = 0;
            for (int k = 0; k < frame_size - 2; k++) {
                c ^= src.plain(k) << 8;
                for (int j = 0; j < 8; j++) c = ((c << 1) ^ ((c & 0x8000u) ? 0x8005u : 0u)) & 0xFFFFu;
            }
            crc = (int)c;
        }
        return i == frame_size - 2 ? ((unsigned)crc >> 8) & 0xFFu : (unsigned)crc & 0xFFu;
    }
    VGA_HCAK_HD int peek(int bits)
    {
        if (bits == 0) return 0;
        const int remaining = frame_bits - pos;
        if (remaining <= 0) return 0;
        const int first = pos >> 3;
        // Three bytes per read, fetched and substituted anew.  A window of eight decrypted bytes kept in registers between
        // reads was measured and is slower.
        unsigned w = byte_at(first) << 16;       // (pos & 7) + bits <= 23: three bytes hold every read
        w |= byte_at(first + 1) << 8;
        w |= byte_at(first + 2);
        int v = (int)((w >> (24 - (pos & 7) - bits)) & ((1u << bits) - 1u));
        if (bits > remaining) v = (v >> (bits - remaining)) << (bits - remaining);
        return v;
    }
    VGA_HCAK_HD int read(int bits)
    {
        const int v = peek(bits);
        pos += bits;
        return v;
    }
};

// FRAME_PASSES, FRAME_FAILS or FRAME_BAD_SYNC for one frame of w.frame_size bytes
template <class Bytes, class Res>
VGA_HCAK_HD int walk_frame(const WalkFile &w, const WalkTables &T, Bytes &src, Res &res)
{
    WalkReader<Bytes> r = {src, w.frame_size, w.frame_size * 8, 0, -1};
    if (r.read(16) != 0xffff) return FRAME_BAD_SYNC;            // UnpackFrameHeader (:71-87): InvalidDataException
    const int noise_level = r.read(9);
    const int eval_boundary = r.read(7);
    bool any_delta_bits = false;
    for (int c = 0; c < w.nch; c++) {
        const int count = w.coded_count[c];
        const int delta_bits = r.read(3);                       // ReadScaleFactors (:111-130)
        any_delta_bits |= delta_bits > 0;
        const int max_delta = delta_bits > 0 ? 1 << (delta_bits - 1) : 0;
        int prev = 0;
        uint32_t word = 0;
        for (int i = 0; i < count; i++) {
            int sf = 0;
            if (delta_bits != 0) {
                if (delta_bits >= 6 || i == 0) sf = r.read(6);
                else {                                          // DeltaDecode (:185-211)
                    const int delta = r.read(delta_bits) - (max_delta - 1);
                    if (delta < max_delta) {
                        sf = prev + delta;
                        if (sf < 0 || sf > 63) return FRAME_FAILS;
                    } else sf = r.read(6);
                }
                prev = sf;
            }
            const int rs = walk_resolution(T, sf, (int)w.ath_curve[i] + noise_level - (i < eval_boundary ? 1 : 0));
            word |= (uint32_t)rs << (4 * (i & 7));
            if ((i & 7) == 7 || i == count - 1) {
                res.put(c, i >> 3, word);
                word = 0;
            }
        }
        r.pos += w.skip_bits[c];
    }
    for (int sf = 0; sf < 8; sf++)                              // ReadSpectralCoefficients (:148-183): lengths only
        for (int c = 0; c < w.nch; c++) {
            const int count = w.coded_count[c];
            uint32_t word = 0;
            for (int s = 0; s < count; s++) {
                if ((s & 7) == 0) word = res.word(c, s >> 3);
                const int resolution = (int)((word >> (4 * (s & 7))) & 15u);
                int bits = T.max_bits[resolution];
                const int code = r.peek(bits);
                if (resolution < 8) bits = T.dec_bits[resolution][code];
                else if (code / 2 == 0) bits--;
                r.pos += bits;
            }
        }
    const int remaining = r.frame_bits - r.pos;                 // UnpackingWasSuccessful (:213-237)
    const bool empty = noise_level <= 0 && !any_delta_bits;
    return ((remaining >= 16 && remaining <= 128) || empty || (noise_level == 0 && remaining >= 16)) ? FRAME_PASSES : FRAME_FAILS;
}

// One candidate over its tested frames, given each frame's verdict in order (TestKey :48-63): rejected at its first failing
// frame whatever later frames hold; a wrong sync word in front of that is the reference's exception.
// first_fail / first_bad_sync: the lowest tested frame with that verdict, `none` when there is none.
VGA_HCAK_HD int candidate_outcome(int first_fail, int first_bad_sync, int none)
{
    return first_bad_sync < first_fail ? FRAME_BAD_SYNC : (first_fail < none ? FRAME_FAILS : FRAME_PASSES);
}

}  // namespace hcak
}  // namespace vga
