// adx_files_host_driver.cpp -- vgaudio_amd/csrc/adx_files_host.hpp (and adx_file_host.hpp under it) on its own
// (tests/test_adx_files_host.py): the header with a set_error / last_error of this file's, no HIP and no product library,
// built with g++ -fsanitize=address,undefined and run as a child process.  `adx_files_host_driver cases.bin results.bin` runs
// every case of cases.bin and writes what the header answered:
//   cases.bin    int32 n; n x { int32 kind, nfiles, noffsets;
//                  kind 0 (vga_adx_files_layout_for's arguments): nfiles x int32[13] (channels, the fields of vga_adx_file_params);
//                  kind 1 (vga_adx_files_create_from_infos's): nfiles x int32[7] (channel_count, frame_size, frame_count,
//                         audio_bytes, audio_offset, version, is_null);
//                  int64 offsets[noffsets] (noffsets == 0: NULL) }
//   results.bin  per case: int32 rc, message length, message bytes; when rc == 0
//                  int32 nfiles, nrows, first_channel[nfiles]; int64 image_off[nfiles]; int32 image_size[nfiles];
//                  int64 row_off[nrows]; int32 row_bytes[nrows]; int64 audio_bytes, image_bytes;
//                  twice (every file in its own form; every file general): int32 count;
//                  count x { int32 form, file, x; uint32 y; int32 granule; int64 begin, end, keep_end }
// Every array handed to the header is a heap block of exactly its size.  Prints "<cases> ok".
#include "../../vgaudio_amd/csrc/adx_files_host.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {
char g_error[512];
}

void vga::set_error(const char *fmt, ...)
{
    char next[sizeof g_error];                             // the arguments may point into g_error
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(next, sizeof next, fmt, ap);
    va_end(ap);
    memcpy(g_error, next, sizeof g_error);
}
const char *vga::last_error() { return g_error; }

using namespace vga;

namespace {

template <class T> bool read_n(FILE *f, T *out, size_t count) { return count == 0 || fread(out, sizeof(T), count, f) == count; }
template <class T> void put(FILE *f, const T &v) { fwrite(&v, sizeof(T), 1, f); }

void write_layout(FILE *out, const adxf::FilesLayout &L)
{
    const int nfiles = L.totals.files, nrows = L.totals.channels;
    put(out, nfiles);
    put(out, nrows);
    for (int f = 0; f < nfiles; f++) put(out, L.first_channel[f]);
    for (int f = 0; f < nfiles; f++) put(out, L.image_off[f]);
    for (int f = 0; f < nfiles; f++) put(out, L.image_size[f]);
    for (int c = 0; c < nrows; c++) put(out, L.row_off[c]);
    for (int c = 0; c < nrows; c++) put(out, L.row_bytes[c]);
    put(out, L.totals.audio_bytes);
    put(out, L.totals.image_bytes);
    for (int general = 0; general < 2; general++) {
        std::vector<vga_adx_files_item> items;
        adxf::describe_items(L, general != 0, items);
        put(out, (int)items.size());
        for (const vga_adx_files_item &it : items) {
            put(out, it.form); put(out, it.file); put(out, it.x); put(out, it.y); put(out, it.granule);
            put(out, it.begin); put(out, it.end); put(out, it.keep_end);
        }
    }
}

}  // namespace

int main(int argc, char **argv)
{
    FILE *in = argc > 2 ? fopen(argv[1], "rb") : nullptr;
    FILE *out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { printf("usage: adx_files_host_driver cases.bin results.bin\n"); return 2; }
    int n = 0;
    if (!read_n(in, &n, 1)) return 2;
    for (int i = 0; i < n; i++) {
        int head[3];
        if (!read_n(in, head, 3)) return 2;
        const int kind = head[0], nfiles = head[1], noffsets = head[2];
        const size_t count = nfiles > 0 ? (size_t)nfiles : 0;
        g_error[0] = 0;
        int rc = 0;
        adxf::FilesLayout *L = new adxf::FilesLayout;
        vga_adx_file *files = nullptr;
        vga_adx_file_info **infos = nullptr;
        if (kind == 0) {
            files = static_cast<vga_adx_file *>(malloc(count * sizeof(vga_adx_file)));
            for (size_t f = 0; f < count; f++) {
                int v[13];
                if (!read_n(in, v, 13)) return 2;
                files[f] = {v[0], {v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12]}};
            }
        } else {
            infos = static_cast<vga_adx_file_info **>(malloc(count * sizeof(vga_adx_file_info *)));
            for (size_t f = 0; f < count; f++) {
                int v[7];
                if (!read_n(in, v, 7)) return 2;
                vga_adx_file_info *I = v[6] ? nullptr : static_cast<vga_adx_file_info *>(calloc(1, sizeof(vga_adx_file_info)));
                if (I) {
                    I->channel_count = v[0]; I->frame_size = v[1]; I->frame_count = v[2]; I->audio_bytes = v[3];
                    I->audio_offset = v[4]; I->version = v[5];
                }
                infos[f] = I;
            }
        }
        int64_t *offsets = noffsets > 0 ? static_cast<int64_t *>(malloc((size_t)noffsets * sizeof(int64_t))) : nullptr;
        if (noffsets > 0 && !read_n(in, offsets, (size_t)noffsets)) return 2;
        if (kind == 0) rc = adxf::make_layout(count ? files : nullptr, nfiles, offsets, *L);
        else rc = adxf::make_layout_from_infos(count ? infos : nullptr, nfiles, offsets, *L);
        free(offsets);
        free(files);
        for (size_t f = 0; infos && f < count; f++) free(infos[f]);
        free(infos);
        put(out, rc);
        const int len = (int)strlen(g_error);
        put(out, len);
        fwrite(g_error, 1, (size_t)len, out);
        if (rc == 0) write_layout(out, *L);
        delete L;
    }
    fclose(in);
    fclose(out);
    printf("%d ok\n", n);
    return 0;
}
