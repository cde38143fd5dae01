// The wave / prefetch parser (vgaudio_amd/csrc/nwwav_parse.hpp) is plain C++.  tests/test_nwwav_host.py compiles this
// with -fsanitize=address and feeds it images: every image, then random truncations and random single-byte corruptions
// of it, is parsed from a heap block of exactly its size, so that a read outside [file, file + size) stops the run.  A
// parse returns VGA_OK or VGA_ERR_INVALID_DATA; after VGA_OK every channel is extracted as well.
// Input: a file of [uint32 size][bytes] records.  Output: "<parsed> <rejected> ok".
#include "../../vgaudio_amd/csrc/nwwav_parse.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); }

static long parsed = 0, rejected = 0;

static bool check(const std::vector<uint8_t> &image, size_t size)
{
    uint8_t *exact = static_cast<uint8_t *>(std::malloc(size ? size : 1));
    std::memcpy(exact, image.data(), size);
    static vga_nwwav_info info;
    vga::nwwav::Failure f;
    const int rc = vga::nwwav::parse(exact, size, &info, &f);
    bool ok = rc == VGA_OK || (rc == VGA_ERR_INVALID_DATA && f.msg[0]);
    if (rc == VGA_OK) {
        parsed++;
        for (int c = 0; ok && c < info.channel_count; c++) {
            uint8_t *row = static_cast<uint8_t *>(std::malloc(info.channel_bytes ? info.channel_bytes : 1));
            ok = vga::nwwav::read_channel(exact, size, &info, c, row) == VGA_OK;
            std::free(row);
        }
    } else
        rejected++;
    if (!ok) std::printf("rc %d (%s) for an image of %zu bytes\n", rc, f.msg, size);
    std::free(exact);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const int rounds = std::atoi(argv[2]);
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t size;
    while (std::fread(&size, 4, 1, in) == 1) {
        std::vector<uint8_t> image(size);
        if (size && std::fread(image.data(), 1, size, in) != size) return 2;
        if (!check(image, size)) return 1;
        for (int k = 0; k < rounds && size; k++) {
            if (!check(image, rnd() % size)) return 1;
            std::vector<uint8_t> bad = image;
            bad[rnd() % size] = (uint8_t)rnd();
            if (!check(bad, size)) return 1;
        }
    }
    std::fclose(in);
    std::printf("%ld %ld ok\n", parsed, rejected);
    return 0;
}
