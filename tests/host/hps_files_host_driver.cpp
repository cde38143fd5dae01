// hps_files_host_driver.cpp -- vgaudio_amd/csrc/hps_files_host.hpp (and gc_stream_host.hpp under it) on its own
// (tests/test_hps_files_host.py): the headers with a set_error / last_error of this file's, no HIP and no product library,
// built with g++ -fsanitize=address,undefined and run as a child process.  `hps_files_host_driver cases.bin results.bin` runs
// every case of cases.bin and writes what the headers answered:
//   cases.bin    int32 n; n x { int32 kind, nfiles;
//                  kind 0 (vga_hps_files_layout_for's arguments): nfiles x int32[6] the fields of vga_hps_file
//                  kind 1 (vga_hps_files_create_from_infos's): int32 has_offsets; nfiles x { int32 channel_count, sample_count,
//                         adpcm_bytes, sample_rate, block_count; block_count x the bytes of a vga_hps_block_info };
//                         int64 offsets[nfiles] when has_offsets
//                  kind 3 (vga_hps_layout_for's and vga_hps_block_map's; nfiles is the channel count): the bytes of a
//                         vga_hps_params }
//   results.bin  per case: int32 rc, message length, message bytes; when rc == 0
//                  kind 3: the bytes of the vga_hps_layout, then block_count x the bytes of a vga_hps_block
//                  kinds 0, 1: int32 nfiles, nch, blocks; int32 first_channel[nfiles]; int64 image_off[nfiles], first_block[nfiles];
//                  int32 image_size[nfiles], counts[nch]; int64 adpcm_off[nch], pcm_off[nch]; int64 pcm_samples, adpcm_bytes,
//                  image_bytes, blocks; blocks x the 32 bytes of a block table entry;
//                  int32 regions; regions x { int32 kernel, index, granule; int64 begin, end }
// Every array handed to the headers is a heap block of exactly its size.  Prints "<cases> ok".
#include "../../vgaudio_amd/csrc/hps_files_host.hpp"

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

void put_status(FILE *out, int rc)
{
    put(out, rc);
    const int len = (int)strlen(g_error);
    put(out, len);
    fwrite(g_error, 1, (size_t)len, out);
}

void write_layout(FILE *out, const hpf::FilesLayout &L)
{
    const int nfiles = L.totals.files, nch = L.totals.channels;
    put(out, nfiles);
    put(out, nch);
    put(out, (int)L.blocks.size());
    for (int f = 0; f < nfiles; f++) put(out, L.first_channel[f]);
    for (int f = 0; f < nfiles; f++) put(out, L.image_off[f]);
    for (int f = 0; f < nfiles; f++) put(out, L.first_block[f]);
    for (int f = 0; f < nfiles; f++) put(out, L.image_size[f]);
    for (int c = 0; c < nch; c++) put(out, L.counts[c]);
    for (int c = 0; c < nch; c++) put(out, L.channel[c].adpcm_off);
    for (int c = 0; c < nch; c++) put(out, L.channel[c].pcm_off);
    const int64_t totals[4] = {L.totals.pcm_samples, L.totals.adpcm_bytes, L.totals.image_bytes, L.totals.blocks};
    fwrite(totals, sizeof totals, 1, out);
    if (!L.blocks.empty()) fwrite(L.blocks.data(), sizeof(hpf::Block), L.blocks.size(), out);
    std::vector<vga_hps_files_region> r;
    hpf::regions_of(L, r);
    put(out, (int)r.size());
    for (const vga_hps_files_region &x : r) { put(out, x.kernel); put(out, x.index); put(out, x.granule); put(out, x.begin); put(out, x.end); }
}

}  // namespace

int main(int argc, char **argv)
{
    FILE *in = argc > 2 ? fopen(argv[1], "rb") : nullptr;
    FILE *out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { printf("usage: hps_files_host_driver cases.bin results.bin\n"); return 2; }
    int n = 0;
    if (!read_n(in, &n, 1)) return 2;
    for (int i = 0; i < n; i++) {
        int kind = 0, nfiles = 0;
        if (!read_n(in, &kind, 1) || !read_n(in, &nfiles, 1)) return 2;
        g_error[0] = 0;
        int rc = 0;
        if (kind == 3) {                                   // nfiles holds the channel count
            vga_hps_params *p = static_cast<vga_hps_params *>(malloc(sizeof *p));
            vga_hps_layout *N = static_cast<vga_hps_layout *>(malloc(sizeof *N));
            if (!read_n(in, p, 1)) return 2;
            std::vector<vga_hps_block> map;
            rc = gcs::hps_layout(p, nfiles, N, &map);
            put_status(out, rc);
            if (rc == 0) {
                fwrite(N, sizeof *N, 1, out);
                fwrite(map.data(), sizeof(vga_hps_block), map.size(), out);
            }
            free(N);
            free(p);
            continue;
        }
        const size_t count = nfiles > 0 ? (size_t)nfiles : 0;
        hpf::FilesLayout *L = new hpf::FilesLayout;
        if (kind == 0) {
            vga_hps_file *files = static_cast<vga_hps_file *>(malloc(count * sizeof(vga_hps_file)));
            for (size_t f = 0; f < count; f++) {
                int v[6];
                if (!read_n(in, v, 6)) return 2;
                files[f] = {v[0], v[1], v[2], v[3], v[4], v[5]};
            }
            rc = hpf::make_layout(count ? files : nullptr, nfiles, *L);
            free(files);
        } else {
            int has_offsets = 0;
            if (!read_n(in, &has_offsets, 1)) return 2;
            vga_hps_info **infos = static_cast<vga_hps_info **>(malloc(count * sizeof(vga_hps_info *)));
            vga_hps_block_info **tables = static_cast<vga_hps_block_info **>(malloc(count * sizeof(vga_hps_block_info *)));
            for (size_t f = 0; f < count; f++) {
                int v[5];
                if (!read_n(in, v, 5)) return 2;
                vga_hps_info *I = static_cast<vga_hps_info *>(calloc(1, sizeof(vga_hps_info)));
                I->channel_count = v[0]; I->sample_count = v[1]; I->adpcm_bytes = v[2]; I->sample_rate = v[3]; I->block_count = v[4];
                infos[f] = I;
                const size_t nb = v[4] > 0 ? (size_t)v[4] : 0;
                tables[f] = static_cast<vga_hps_block_info *>(malloc((nb ? nb : 1) * sizeof(vga_hps_block_info)));
                if (!read_n(in, tables[f], nb)) return 2;
            }
            int64_t *offsets = has_offsets ? static_cast<int64_t *>(malloc(count * sizeof(int64_t))) : nullptr;
            if (has_offsets && !read_n(in, offsets, count)) return 2;
            rc = hpf::make_layout_from_infos(count ? infos : nullptr, count ? tables : nullptr, nfiles, offsets, *L);
            free(offsets);
            for (size_t f = 0; f < count; f++) { free(infos[f]); free(tables[f]); }
            free(infos);
            free(tables);
        }
        put_status(out, rc);
        if (rc == 0) write_layout(out, *L);
        delete L;
    }
    fclose(in);
    fclose(out);
    printf("%d ok\n", n);
    return 0;
}
