// files_table_pack_driver.cpp -- vgaudio_amd/csrc/files_table_pack.hpp on its own (no HIP), for tests/test_files_table_pack_host.py,
// which builds it with -fsanitize=address,undefined and compares what it writes with a model of its own.
//
//   files_table_pack_driver <cases file> <results file>
//
// Cases file (little endian): int32 cases; per case int32 parts, then per part int32 raw (0: a table, 1: a raw region), int32
// element size, int32 element count (a raw region: size 1, count = its bytes).  Byte i of part p holds pattern(p, i); the raw
// regions are written into the image after image(), as capi_gc_aligned.hip writes its tail batch.
// Results file: per case int32 parts, int64 offset per part, int64 bytes(), int64 size of the image, the image.
#include "../../vgaudio_amd/csrc/files_table_pack.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <utility>

using vga::fileset::TablePack;

static unsigned char pattern(int part, size_t i) { return (unsigned char)(part * 37 + i * 11 + 1); }

template <size_t N> struct Elem { unsigned char b[N]; };

struct Held {                                    // a part's source vector, alive until the case's image is made
    virtual ~Held() {}
};
template <size_t N> struct HeldVector : Held { std::vector<Elem<N>> v; };

using AtCheck = std::function<bool(const TablePack &, const unsigned char *)>;   // at(handle, base) == base + the handle's offset

// adds a table of `count` elements of N bytes
template <size_t N> size_t add_table(TablePack &pack, std::vector<std::unique_ptr<Held>> &held, std::vector<AtCheck> &checks, int part, int count)
{
    auto *h = new HeldVector<N>;
    held.emplace_back(h);
    h->v.resize((size_t)count);
    unsigned char *bytes = reinterpret_cast<unsigned char *>(h->v.data());
    for (size_t i = 0; i < (size_t)count * N; i++) bytes[i] = pattern(part, i);
    const TablePack::Part<Elem<N>> p = pack.add(h->v);
    checks.push_back([p](const TablePack &k, const unsigned char *base) {
        const Elem<N> *at = k.at(p, base);
        return reinterpret_cast<const unsigned char *>(at) == base + p.at;
    });
    return p.at;
}

static bool read_i32(std::FILE *f, int32_t *v, int n) { return std::fread(v, sizeof(int32_t), (size_t)n, f) == (size_t)n; }

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s <cases> <results>\n", argv[0]); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t cases = 0;
    if (!read_i32(in, &cases, 1)) return 2;
    for (int c = 0; c < cases; c++) {
        int32_t parts = 0;
        if (!read_i32(in, &parts, 1)) return 2;
        TablePack pack;
        std::vector<std::unique_ptr<Held>> held;
        std::vector<AtCheck> checks;
        std::vector<int64_t> offsets;
        std::vector<std::pair<int, size_t>> raw;                  // (part, bytes) of the raw regions
        for (int p = 0; p < parts; p++) {
            int32_t d[3];
            if (!read_i32(in, d, 3)) return 2;
            size_t at = 0;
            if (d[0]) {
                at = pack.add_raw((size_t)d[2]);
                raw.push_back({p, (size_t)d[2]});
            } else {
                switch (d[1]) {
                case 1: at = add_table<1>(pack, held, checks, p, d[2]); break;
                case 2: at = add_table<2>(pack, held, checks, p, d[2]); break;
                case 4: at = add_table<4>(pack, held, checks, p, d[2]); break;
                case 8: at = add_table<8>(pack, held, checks, p, d[2]); break;
                case 12: at = add_table<12>(pack, held, checks, p, d[2]); break;
                case 32: at = add_table<32>(pack, held, checks, p, d[2]); break;
                default: std::fprintf(stderr, "case %d: no element of %d bytes\n", c, d[1]); return 2;
                }
            }
            offsets.push_back((int64_t)at);
        }
        std::vector<unsigned char> image = pack.image();
        for (const AtCheck &check : checks)
            if (!check(pack, image.data())) { std::fprintf(stderr, "case %d: at() is not base + offset\n", c); return 1; }
        for (const auto &r : raw)
            for (size_t i = 0; i < r.second; i++) image[(size_t)offsets[(size_t)r.first] + i] = pattern(r.first, i);
        const int64_t sizes[2] = {(int64_t)pack.bytes(), (int64_t)image.size()};
        std::fwrite(&parts, sizeof parts, 1, out);
        if (!offsets.empty()) std::fwrite(offsets.data(), sizeof(int64_t), offsets.size(), out);
        std::fwrite(sizes, sizeof(int64_t), 2, out);
        std::fwrite(image.data(), 1, image.size(), out);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::printf("%d ok\n", cases);
    return 0;
}
