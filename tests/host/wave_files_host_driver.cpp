// wave_files_host_driver.cpp -- vgaudio_amd/csrc/wave_files_host.hpp (and wave_file_host.hpp under it) on its own
// (tests/test_wave_files_host.py): the header with a set_error / last_error of this file's, no HIP and no product library,
// built with g++ -fsanitize=address,undefined and run as a child process.  `wave_files_host_driver cases.bin results.bin` runs
// every case of cases.bin and writes what the header answered:
//   cases.bin    int32 n; n x { int32 kind, nfiles, npcm, nimage;
//                  kind 0 (vga_wave_files_layout_for's arguments): nfiles x int32[7] (channels, bits, the fields of vga_wave_params);
//                  kind 1 (vga_wave_files_create_from_infos's): nfiles x int64[6] (channel_count, bits_per_sample, sample_count,
//                         data_size, data_offset, is_null);
//                  int64 pcm_offsets[npcm] (npcm == 0: NULL); int64 image_offsets[nimage] (nimage == 0: NULL) }
//   results.bin  per case: int32 rc, message length, message bytes; when rc == 0
//                  int32 nfiles, nrows, first_channel[nfiles]; int64 image_off[nfiles]; int32 image_size[nfiles];
//                  int64 row_off[nrows]; int32 row_samples[nrows]; int64 pcm_samples, image_bytes;
//                  (kind 0) nfiles x { int32 header size; the header's bytes };
//                  twice (every file in its own form; every file general): int32 count;
//                  count x { int32 form, file, x; uint32 y; int32 span; int64 begin, end }
// Every array handed to the header is a heap block of exactly its size.  Prints "<cases> ok".
#include "../../vgaudio_amd/csrc/wave_files_host.hpp"

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

void write_layout(FILE *out, const wavf::FilesLayout &L)
{
    const int nfiles = L.totals.files, nrows = L.totals.channels;
    put(out, nfiles);
    put(out, nrows);
    for (int f = 0; f < nfiles; f++) put(out, L.first_channel[f]);
    for (int f = 0; f < nfiles; f++) put(out, L.image_off[f]);
    for (int f = 0; f < nfiles; f++) put(out, L.image_size[f]);
    for (int c = 0; c < nrows; c++) put(out, L.row_off[c]);
    for (int c = 0; c < nrows; c++) put(out, L.row_samples[c]);
    put(out, L.totals.pcm_samples);
    put(out, L.totals.image_bytes);
    if (!L.from_infos)
        for (int f = 0; f < nfiles; f++) {
            put(out, L.tab[f].header_size);
            fwrite(L.headers.data() + (size_t)f * wavf::HEADER_PITCH, 1, (size_t)L.tab[f].header_size, out);
        }
    for (int general = 0; general < 2; general++) {
        std::vector<vga_wave_files_item> items;
        wavf::describe_items(L, general != 0, items);
        put(out, (int)items.size());
        for (const vga_wave_files_item &it : items) {
            put(out, it.form); put(out, it.file); put(out, it.x); put(out, it.y); put(out, it.span);
            put(out, it.begin); put(out, it.end);
        }
    }
}

int64_t *read_offsets(FILE *in, int count, bool *ok)
{
    if (count <= 0) return nullptr;
    int64_t *v = static_cast<int64_t *>(malloc((size_t)count * sizeof(int64_t)));
    *ok = *ok && read_n(in, v, (size_t)count);
    return v;
}

}  // namespace

int main(int argc, char **argv)
{
    FILE *in = argc > 2 ? fopen(argv[1], "rb") : nullptr;
    FILE *out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { printf("usage: wave_files_host_driver cases.bin results.bin\n"); return 2; }
    int n = 0;
    if (!read_n(in, &n, 1)) return 2;
    for (int i = 0; i < n; i++) {
        int head[4];
        if (!read_n(in, head, 4)) return 2;
        const int kind = head[0], nfiles = head[1];
        const size_t count = nfiles > 0 ? (size_t)nfiles : 0;
        g_error[0] = 0;
        int rc = 0;
        wavf::FilesLayout *L = new wavf::FilesLayout;
        vga_wave_file *files = nullptr;
        vga_wave_info **infos = nullptr;
        if (kind == 0) {
            files = static_cast<vga_wave_file *>(malloc(count * sizeof(vga_wave_file)));
            for (size_t f = 0; f < count; f++) {
                int v[7];
                if (!read_n(in, v, 7)) return 2;
                files[f] = {v[0], v[1], {v[2], v[3], v[4], v[5], v[6]}};
            }
        } else {
            infos = static_cast<vga_wave_info **>(malloc(count * sizeof(vga_wave_info *)));
            for (size_t f = 0; f < count; f++) {
                int64_t v[6];
                if (!read_n(in, v, 6)) return 2;
                vga_wave_info *I = v[5] ? nullptr : static_cast<vga_wave_info *>(calloc(1, sizeof(vga_wave_info)));
                if (I) {
                    I->channel_count = (int)v[0]; I->bits_per_sample = (int)v[1]; I->sample_count = (int)v[2];
                    I->data_size = (int)v[3]; I->data_offset = v[4];
                }
                infos[f] = I;
            }
        }
        bool ok = true;
        int64_t *pcm_offsets = read_offsets(in, head[2], &ok), *image_offsets = read_offsets(in, head[3], &ok);
        if (!ok) return 2;
        if (kind == 0) rc = wavf::make_layout(count ? files : nullptr, nfiles, pcm_offsets, image_offsets, *L);
        else rc = wavf::make_layout_from_infos(count ? infos : nullptr, nfiles, pcm_offsets, image_offsets, *L);
        free(pcm_offsets);
        free(image_offsets);
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
