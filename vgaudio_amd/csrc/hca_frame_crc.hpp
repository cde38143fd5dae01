// hca_frame_crc.hpp -- the CRC-16 of one HCA frame computed by one wave (Utilities/Crc16.cs with polynomial 0x8005,
// MSB first, initial value 0; CriHcaEncryption.cs:10, HcaReader.cs:18).  Lane l takes the l-th contiguous chunk of the
// frame's first FrameSize - 2 bytes and CRCs it on its own; the chunk CRCs are moved to their place with x^(8k) mod P
// (crc_pow, the table vga::hca::crc_pow_table builds) and XOR-reduced across the wave.  Used by the decryption pass
// (crypt_kernels.hip) and the HCA file reader (container_readers.hip).
#pragma once
#include "common.hpp"

namespace vga {
namespace hca_crc {

// entries of the crc_pow table: wave_combine reads entry nbytes - end < frame size, and a frame size is at most 0xFFFF
// (the decoder's limit; a file's 16-bit field stays below 0x8000)
constexpr int kPowEntries = 65536;

// multiply in GF(2)[x] / (x^16 + x^15 + x^2 + 1)
__device__ __forceinline__ unsigned gf_mul16(unsigned a, unsigned b)
{
    unsigned r = 0;
#pragma unroll
    for (int i = 15; i >= 0; i--) {
        r = ((r << 1) ^ ((r & 0x8000u) ? 0x8005u : 0u)) & 0xFFFFu;
        if ((a >> i) & 1u) r ^= b;
    }
    return r;
}

// one byte into a running CRC
__device__ __forceinline__ unsigned step(unsigned crc, unsigned byte)
{
    crc ^= byte << 8;
#pragma unroll
    for (int j = 0; j < 8; j++) crc = ((crc << 1) ^ ((crc & 0x8000u) ? 0x8005u : 0u)) & 0xFFFFu;
    return crc;
}

// the bytes [begin, end) of an nbytes-long message lane `lane` of 64 covers
struct Chunk { int begin, end; };
__device__ __forceinline__ Chunk lane_chunk(int lane, int nbytes)
{
    const int chunk = (nbytes + 63) / 64;
    const int begin = min(lane * chunk, nbytes);
    return Chunk{begin, min(begin + chunk, nbytes)};
}

// the message's CRC in every lane, from each lane's CRC of its own chunk
__device__ __forceinline__ unsigned wave_combine(unsigned crc, Chunk c, int nbytes, const uint16_t *__restrict__ crc_pow)
{
    unsigned part = c.begin < c.end ? gf_mul16(crc, crc_pow[nbytes - c.end]) : 0u;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) part ^= (unsigned)__shfl_xor((int)part, o);
    return part;
}

}  // namespace hca_crc
}  // namespace vga
