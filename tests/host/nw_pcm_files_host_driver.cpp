// nw_pcm_files_host_driver.cpp -- vgaudio_amd/csrc/nw_pcm_files_host.hpp (and nw_host.hpp, wave_files_host.hpp under it) on its
// own (tests/test_nw_pcm_files_host.py): the header with a set_error / last_error of this file's, no HIP and no product
// library, built with g++ -fsanitize=address,undefined and run as a child process.  `nw_pcm_files_host_driver cases.bin
// results.bin` runs every case of cases.bin and writes what the header answered:
//   cases.bin    int32 n; n x { int32 kind, nfiles, npcm, nimage, codec, has_config;
//                  kind 0 (vga_nw_pcm_files_layout_for's arguments): int32[8] the fields of vga_nw_file_config, then
//                         nfiles x int32[6] the fields of vga_nw_file;
//                  kind 1 (vga_nw_pcm_files_create_from_infos's): nfiles x int32[11] (target, endianness, codec, channel_count,
//                         sample_count, interleave_size, audio_data_offset, audio_data_length, adpcm_bytes, looping, is_null);
//                  kind 2 (nw::pcm_read_info_check alone): one info as in kind 1, then int32 sample_kind, moves;
//                  int64 pcm_offsets[npcm] (npcm == 0: NULL); int64 image_offsets[nimage] (nimage == 0: NULL) }
//   results.bin  per case: int32 rc, message length, message bytes; when rc == 0 and kind < 2
//                  int32 nfiles, nrows, first_channel[nfiles]; int64 image_off[nfiles]; int32 image_size[nfiles];
//                  int64 row_off[nrows]; int32 row_samples[nrows]; int64 pcm_samples, image_bytes;
//                  nfiles x { int32 conv, vector; uint32 input_size, interleave, output_size; int64 audio_at };
//                  int32 vector_files, general_files, moving_files;
//                  twice (every file in its own form; every file general): int32 count;
//                  count x { int32 form, file, x; uint32 y; int32 conv; int64 begin, end }
// Every array handed to the header is a heap block of exactly its size.  Prints "<cases> ok".
#include "../../vgaudio_amd/csrc/nw_pcm_files_host.hpp"

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

void write_layout(FILE *out, const nwpf::FilesLayout &L)
{
    const int nfiles = L.P.totals.files, nrows = L.P.totals.channels;
    put(out, nfiles);
    put(out, nrows);
    for (int f = 0; f < nfiles; f++) put(out, L.P.first_channel[f]);
    for (int f = 0; f < nfiles; f++) put(out, L.P.image_off[f]);
    for (int f = 0; f < nfiles; f++) put(out, L.P.image_size[f]);
    for (int c = 0; c < nrows; c++) put(out, L.P.row_off[c]);
    for (int c = 0; c < nrows; c++) put(out, L.P.row_samples[c]);
    put(out, L.P.totals.pcm_samples);
    put(out, L.P.totals.image_bytes);
    for (int f = 0; f < nfiles; f++) {
        const nwpf::FileTab &t = L.tab[f];
        put(out, t.conv); put(out, t.vector); put(out, t.input_size); put(out, t.interleave); put(out, t.output_size); put(out, t.audio_at);
    }
    put(out, L.vector_files); put(out, L.general_files); put(out, L.moving_files);
    for (int general = 0; general < 2; general++) {
        std::vector<vga_nw_pcm_files_item> items;
        nwpf::describe_items(L, general != 0, items);
        put(out, (int)items.size());
        for (const vga_nw_pcm_files_item &it : items) {
            put(out, it.form); put(out, it.file); put(out, it.x); put(out, it.y); put(out, it.conv);
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

vga_nwstm_info *read_info(FILE *in, bool *ok)
{
    int v[11];
    *ok = *ok && read_n(in, v, 11);
    if (!*ok || v[10]) return nullptr;
    vga_nwstm_info *I = static_cast<vga_nwstm_info *>(calloc(1, sizeof(vga_nwstm_info)));
    I->target = v[0]; I->endianness = v[1]; I->codec = v[2]; I->channel_count = v[3]; I->sample_count = v[4];
    I->interleave_size = v[5]; I->audio_data_offset = v[6]; I->audio_data_length = v[7]; I->adpcm_bytes = v[8]; I->looping = v[9];
    return I;
}

}  // namespace

int main(int argc, char **argv)
{
    FILE *in = argc > 2 ? fopen(argv[1], "rb") : nullptr;
    FILE *out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { printf("usage: nw_pcm_files_host_driver cases.bin results.bin\n"); return 2; }
    int n = 0;
    if (!read_n(in, &n, 1)) return 2;
    for (int i = 0; i < n; i++) {
        int head[6];
        if (!read_n(in, head, 6)) return 2;
        const int kind = head[0], nfiles = head[1], codec = head[4];
        const size_t count = nfiles > 0 ? (size_t)nfiles : 0;
        g_error[0] = 0;
        int rc = 0;
        bool ok = true;
        nwpf::FilesLayout *L = new nwpf::FilesLayout;
        vga_nw_file *files = nullptr;
        vga_nw_file_config *config = nullptr;
        vga_nwstm_info **infos = nullptr;
        int check[2] = {0, 0};
        if (kind == 0) {
            int c[8];
            if (!read_n(in, c, 8)) return 2;
            if (head[5]) {
                config = static_cast<vga_nw_file_config *>(malloc(sizeof(vga_nw_file_config)));
                *config = {c[0], c[1], c[2], c[3], c[4], c[5], (uint32_t)c[6], c[7]};
            }
            files = static_cast<vga_nw_file *>(malloc(count * sizeof(vga_nw_file)));
            for (size_t f = 0; f < count; f++) {
                int v[6];
                if (!read_n(in, v, 6)) return 2;
                files[f] = {v[0], v[1], v[2], v[3], v[4], v[5]};
            }
        } else {
            infos = static_cast<vga_nwstm_info **>(malloc(count * sizeof(vga_nwstm_info *)));
            for (size_t f = 0; f < count; f++) infos[f] = read_info(in, &ok);
            if (kind == 2 && !read_n(in, check, 2)) return 2;
        }
        int64_t *pcm_offsets = read_offsets(in, head[2], &ok), *image_offsets = read_offsets(in, head[3], &ok);
        if (!ok) return 2;
        if (kind == 0) rc = nwpf::make_layout(count ? files : nullptr, nfiles, config, codec, pcm_offsets, image_offsets, *L);
        else if (kind == 1) rc = nwpf::make_layout_from_infos(count ? infos : nullptr, nfiles, pcm_offsets, image_offsets, *L);
        else rc = nw::pcm_read_info_check(infos[0], check[0], check[1] != 0);
        free(pcm_offsets);
        free(image_offsets);
        free(files);
        free(config);
        for (size_t f = 0; infos && f < count; f++) free(infos[f]);
        free(infos);
        put(out, rc);
        const int len = (int)strlen(g_error);
        put(out, len);
        fwrite(g_error, 1, (size_t)len, out);
        if (rc == 0 && kind < 2) write_layout(out, *L);
        delete L;
    }
    fclose(in);
    fclose(out);
    printf("%d ok\n", n);
    return 0;
}
