// files_table_pack.hpp -- the one image a set of files uploads at create: the tables of a set, each on a
// multiple of 16 bytes, zeros between and after them.  HIP-free, so tests/host/files_table_pack_driver.cpp runs it on its own.
#pragma once
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <vector>

namespace vga {
namespace fileset {

class TablePack {
public:
    template <class T> struct Part { size_t at; };              // where a table of T starts in the image

    // a table: room for its bytes rounded up to 16 (an empty one takes none), copied in by image().  The vector is read then,
    // not now: it stays as it is, and where it is, until image() has run.
    template <class T> Part<T> add(const std::vector<T> &v)
    {
        static_assert(std::is_trivially_copyable<T>::value, "a table is copied byte for byte");
        const size_t at = add_raw(v.size() * sizeof(T));
        if (!v.empty()) parts_.push_back({at, v.data(), v.size() * sizeof(T)});
        return {at};
    }
    // room the caller writes itself into image() (zeros until then); returns where it starts
    size_t add_raw(size_t bytes)
    {
        const size_t at = room_;
        room_ += (bytes + 15) / 16 * 16;
        return at;
    }
    size_t bytes() const { return room_ + 16; }                 // the tables and 16 bytes of slack
    std::vector<unsigned char> image() const
    {
        std::vector<unsigned char> host(bytes(), 0);
        for (const Source &p : parts_) memcpy(host.data() + p.at, p.data, p.bytes);
        return host;
    }
    // the table's address once the image lies at `base`
    template <class T> const T *at(Part<T> part, const void *base) const
    {
        return reinterpret_cast<const T *>(static_cast<const unsigned char *>(base) + part.at);
    }

private:
    struct Source { size_t at; const void *data; size_t bytes; };
    std::vector<Source> parts_;
    size_t room_ = 0;
};

}  // namespace fileset
}  // namespace vga
