// hca_files_host_driver.cpp -- vgaudio_amd/csrc/hca_files_host.hpp on its own (tests/test_hca_files_host.py): the header
// with a set_error / last_error of this file's, no HIP and no product library, built with g++ -fsanitize=address,undefined and
// run as a child process.  The two per-file functions the header calls are stand-ins here: vga_hca_file_size with the
// library's formula and words, vga_hca_file_header with the library's range check and a header of zeros behind "HCA" (the
// chunks are the library's business; the test compares only the refusals both know).
// `hca_files_host_driver cases.bin results.bin` runs every case of cases.bin and writes what the header answered:
//   cases.bin    int32 n; n x { int32 kind, nfiles, nframe_offsets, nimage_offsets, with_keys, ntables, tables_null;
//                  kind 0 (vga_hca_files_create's arguments): nfiles x int32[4] (frame_size, frame_count, header_size, key);
//                  kind 1 (vga_hca_files_create_from_infos's): nfiles x int32[5] (frame_size, frame_count, frames_offset, key, is_null);
//                  int64 frame_offsets[nframe_offsets]; int64 image_offsets[nimage_offsets] (0 entries: NULL) }
//   results.bin  per case: int32 rc, message length, message bytes; when rc == 0
//                  int32 nfiles; int64 frame_off[nfiles], image_off[nfiles]; int32 image_size[nfiles];
//                  int64 total_frames, frame_bytes, image_bytes; int32 span_files, general_files, moving_files;
//                  twice (every file in its own form; every file general): int32 count;
//                  count x { int32 form, file, first_frame, frames; int64 begin, end }
// Every array handed to the header is a heap block of exactly its size.  Prints "<cases> ok".
#include "../../vgaudio_amd/csrc/hca_files_host.hpp"

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

extern "C" int vga_hca_file_size(const vga_hca_info *h)
{
    if (!h) { vga::set_error("null HcaInfo"); return VGA_ERR_ARGUMENT; }
    const int64_t n = (int64_t)h->header_size + (int64_t)h->frame_size * h->frame_count;
    if (h->header_size < 0 || h->frame_size < 0 || h->frame_count < 0 || n > 0x7FFFFFFF) {
        vga::set_error("HCA file size out of range");
        return VGA_ERR_OUT_OF_RANGE;
    }
    return (int)n;
}

extern "C" int vga_hca_file_header(const vga_hca_info *h, const char *, float, int, int, uint8_t *header_out)
{
    if (!h || !header_out) { vga::set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (h->header_size < 8 || h->header_size > 0x7FFF) { vga::set_error("HCA header size %d out of range", h->header_size); return VGA_ERR_OUT_OF_RANGE; }
    memset(header_out, 0, (size_t)h->header_size);
    memcpy(header_out, "HCA", 3);
    return VGA_OK;
}

using namespace vga;

namespace {

template <class T> bool read_n(FILE *f, T *out, size_t count) { return count == 0 || fread(out, sizeof(T), count, f) == count; }
template <class T> void put(FILE *f, const T &v) { fwrite(&v, sizeof(T), 1, f); }

void write_layout(FILE *out, const hcaf::FilesLayout &L)
{
    const int nfiles = L.totals.files;
    put(out, nfiles);
    for (int f = 0; f < nfiles; f++) put(out, L.frame_off[f]);
    for (int f = 0; f < nfiles; f++) put(out, L.image_off[f]);
    for (int f = 0; f < nfiles; f++) put(out, L.image_size[f]);
    put(out, L.totals.total_frames);
    put(out, L.totals.frame_bytes);
    put(out, L.totals.image_bytes);
    put(out, L.span_files);
    put(out, L.general_files);
    put(out, L.moving_files);
    for (int general = 0; general < 2; general++) {
        std::vector<vga_hca_files_item> items;
        hcaf::describe_items(L, general != 0, items);
        put(out, (int)items.size());
        for (const vga_hca_files_item &it : items) {
            put(out, it.form); put(out, it.file); put(out, it.first_frame); put(out, it.frames);
            put(out, it.begin); put(out, it.end);
        }
    }
}

}  // namespace

int main(int argc, char **argv)
{
    FILE *in = argc > 2 ? fopen(argv[1], "rb") : nullptr;
    FILE *out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { printf("usage: hca_files_host_driver cases.bin results.bin\n"); return 2; }
    int n = 0;
    if (!read_n(in, &n, 1)) return 2;
    for (int i = 0; i < n; i++) {
        int head[7];
        if (!read_n(in, head, 7)) return 2;
        const int kind = head[0], nfiles = head[1], nfo = head[2], nio = head[3], with_keys = head[4], ntables = head[5], tables_null = head[6];
        const size_t count = nfiles > 0 ? (size_t)nfiles : 0;
        g_error[0] = 0;
        int rc = 0;
        hcaf::FilesLayout *L = new hcaf::FilesLayout;
        vga_hca_file *files = nullptr;
        vga_hca_file_info **infos = nullptr;
        int *keys = nullptr;
        if (kind == 0) {
            files = static_cast<vga_hca_file *>(calloc(count ? count : 1, sizeof(vga_hca_file)));
            for (size_t f = 0; f < count; f++) {
                int v[4];
                if (!read_n(in, v, 4)) return 2;
                files[f].hca.frame_size = v[0]; files[f].hca.frame_count = v[1]; files[f].hca.header_size = v[2];
                files[f].volume = 1.0f; files[f].key = v[3];
            }
        } else {
            infos = static_cast<vga_hca_file_info **>(malloc((count ? count : 1) * sizeof(vga_hca_file_info *)));
            keys = static_cast<int *>(malloc((count ? count : 1) * sizeof(int)));
            for (size_t f = 0; f < count; f++) {
                int v[5];
                if (!read_n(in, v, 5)) return 2;
                vga_hca_file_info *I = v[4] ? nullptr : static_cast<vga_hca_file_info *>(calloc(1, sizeof(vga_hca_file_info)));
                if (I) { I->hca.frame_size = v[0]; I->hca.frame_count = v[1]; I->frames_offset = v[2]; I->hca.header_size = v[2]; }
                infos[f] = I;
                keys[f] = v[3];
            }
        }
        int64_t *fo = nfo > 0 ? static_cast<int64_t *>(malloc((size_t)nfo * sizeof(int64_t))) : nullptr;
        if (nfo > 0 && !read_n(in, fo, (size_t)nfo)) return 2;
        int64_t *io = nio > 0 ? static_cast<int64_t *>(malloc((size_t)nio * sizeof(int64_t))) : nullptr;
        if (nio > 0 && !read_n(in, io, (size_t)nio)) return 2;
        uint8_t *tables = ntables > 0 && !tables_null ? static_cast<uint8_t *>(malloc((size_t)ntables * 256)) : nullptr;
        for (int k = 0; tables && k < ntables * 256; k++) tables[k] = (uint8_t)(k * 7);
        if (kind == 0) rc = hcaf::make_layout(count ? files : nullptr, nfiles, fo, tables, ntables, with_keys != 0, *L);
        else rc = hcaf::make_layout_from_infos(count ? infos : nullptr, nfiles, io, keys, tables, ntables, with_keys != 0, fo, *L);
        free(tables);
        free(fo);
        free(io);
        free(files);
        free(keys);
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
