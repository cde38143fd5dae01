// adx_lcg.hpp -- the 15-bit LCG of CRI ADX encryption (CriAdxEncryption.cs:16-41) as an affine map, for device and host code.
// The reference steps xor = (xor * mult + inc) & 0x7fff once per (frame, channel) slot, serially.  The k-th state is an affine
// map of the seed modulo 2^15, obtained here by square-and-multiply so every slot is independent; maps compose, so a thread
// jumps once to its first slot and then steps by a stride of its own.  No HIP header is needed: a host program includes this
// file as it is (tests/host/adx_keyed_files_host_driver.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VGA_ADX_LCG_FN __host__ __device__ __forceinline__
#else
#define VGA_ADX_LCG_FN inline
#endif

namespace vga {
namespace adxlcg {

constexpr unsigned kMask = 0x7fffu;

struct Affine { unsigned a, c; };      // x -> a * x + c  (mod 2^15)

VGA_ADX_LCG_FN unsigned apply(Affine p, unsigned x) { return (p.a * x + p.c) & kMask; }

// `first`, then `second`
VGA_ADX_LCG_FN Affine then(Affine first, Affine second)
{
    return Affine{(second.a * first.a) & kMask, (second.a * first.c + second.c) & kMask};
}

// k steps of x -> mult * x + inc
VGA_ADX_LCG_FN Affine lcg_power(unsigned mult, unsigned inc, uint64_t k)
{
    Affine r{1u, 0u};
    unsigned a = mult & kMask, c = inc & kMask;
    while (k) {
        if (k & 1) { r.a = (r.a * a) & kMask; r.c = (r.c * a + c) & kMask; }
        c = (c * (a + 1)) & kMask;
        a = (a * a) & kMask;
        k >>= 1;
    }
    return r;
}

}  // namespace adxlcg
}  // namespace vga
