// byte_reader.hpp -- endian-aware reads over a file in host memory.  Plain C++ with no HIP in it, so that the parsers
// built on it alone (nwwav_parse.hpp) also compile for the host sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

namespace vga {
namespace container {

// Big- or little-endian reads over a file in host memory (BinaryReader, BinaryReaderBE); a read past the end or at a
// negative position sets `eof` (EndOfStreamException) and returns 0.
struct ByteReader {
    const uint8_t *p;
    int64_t len, pos = 0;
    bool big = false, eof = false;
    bool has(int64_t n) { if (pos < 0 || pos + n > len) { eof = true; return false; } return true; }
    int u8() { if (!has(1)) return 0; return p[pos++]; }
    int u16() { if (!has(2)) return 0; const int v = big ? (p[pos] << 8 | p[pos + 1]) : (p[pos] | p[pos + 1] << 8); pos += 2; return v; }
    int i16() { return (int16_t)u16(); }
    int i32()
    {
        if (!has(4)) return 0;
        const uint32_t b0 = p[pos], b1 = p[pos + 1], b2 = p[pos + 2], b3 = p[pos + 3];
        pos += 4;
        return (int)(big ? (b0 << 24 | b1 << 16 | b2 << 8 | b3) : (b3 << 24 | b2 << 16 | b1 << 8 | b0));
    }
    // the next n bytes equal `t` (they are consumed either way)
    bool magic(const char *t, int n) { if (!has(n)) return false; const bool ok = std::memcmp(p + pos, t, n) == 0; pos += n; return ok; }
    bool bytes(void *out, int n) { if (!has(n)) return false; std::memcpy(out, p + pos, n); pos += n; return true; }
    void skip_to(int64_t target) { if (target > pos) pos = std::min(target, len); }   // ReadBytes(remaining) stops at the end
};

}  // namespace container
}  // namespace vga
