// gc_files_host_driver.cpp -- vgaudio_amd/csrc/gc_files_host.hpp on its own (tests/test_gc_files_host.py): the header with a
// set_error of this file's, no HIP and no product library, built with g++ -fsanitize=address,undefined and run as a child
// process.  `gc_files_host_driver cases.bin results.bin` runs every case of cases.bin and writes what the header answered:
//   cases.bin    int32 n; n x { int32 kind;
//                  kind 0 (vga_gc_files_layout_for's arguments): int32 nfiles, has_dsp, samples_per_interleave, loop_point_alignment,
//                         trim_file; nfiles x int32[8] (channels, sample_rate, the six fields of vga_gcadpcm_channel_params)
//                  kind 1 (vga_gc_files_create_from_dsp's): int32 nfiles, has_offsets; nfiles x int32[10] (channel_count, sample_count,
//                         nibble_count, frames_per_interleave, audio_offset, adpcm_bytes, interleave_size, data_length, looping,
//                         sample_rate); int64 offsets[nfiles] when has_offsets }
//   results.bin  per case: int32 rc, message length, message bytes; when rc == 0:
//                  int32 nfiles, nch, first_channel[nfiles]; int64 image_off[nfiles]; int32 counts[nch];
//                  int64 pcm_off[nch], adpcm_off[nch], seek_off[nch]; int32 entries[nch], loop_start[nch], spacing[nch], file[nch];
//                  int64 pcm_samples, adpcm_bytes, seek_shorts, image_bytes, build_workspace_bytes;
//                  int32 ngeom; ngeom x uint32[4] (input_size, interleave, output_size, granule16);
//                  int32 audio items; items x { int32 x; uint32 y }; int32 meta items; items x int32[2]
// Every array handed to the header is a heap block of exactly its size.  Prints "<cases> ok".
#include "../../vgaudio_amd/csrc/gc_files_host.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {
char g_error[512];
}

void vga::set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

using namespace vga;

namespace {

template <class T> bool read_n(FILE *f, T *out, size_t count) { return count == 0 || fread(out, sizeof(T), count, f) == count; }
template <class T> void put(FILE *f, const T &v) { fwrite(&v, sizeof(T), 1, f); }

void write_layout(FILE *out, const gcf::FilesLayout &L)
{
    const int nfiles = L.totals.files, nch = L.totals.channels;
    put(out, nfiles);
    put(out, nch);
    for (int f = 0; f < nfiles; f++) put(out, L.first_channel[f]);
    for (int f = 0; f < nfiles; f++) put(out, L.image_off[f]);
    for (int c = 0; c < nch; c++) put(out, L.counts[c]);
    for (int c = 0; c < nch; c++) put(out, L.channel[c].pcm_off);
    for (int c = 0; c < nch; c++) put(out, L.channel[c].adpcm_off);
    for (int c = 0; c < nch; c++) put(out, L.channel[c].seek_off);
    for (int c = 0; c < nch; c++) put(out, L.channel[c].entries);
    for (int c = 0; c < nch; c++) put(out, L.channel[c].loop_start);
    for (int c = 0; c < nch; c++) put(out, L.channel[c].spacing);
    for (int c = 0; c < nch; c++) put(out, L.channel[c].file);
    const int64_t totals[5] = {L.totals.pcm_samples, L.totals.adpcm_bytes, L.totals.seek_shorts, L.totals.image_bytes,
                               (int64_t)L.totals.build_workspace_bytes};
    fwrite(totals, sizeof totals, 1, out);
    put(out, (int)L.geom.size());
    for (const gcf::FileGeom &g : L.geom) {
        const uint32_t v[4] = {g.input_size, g.interleave, g.output_size, g.granule16};
        fwrite(v, sizeof v, 1, out);
    }
    put(out, (int)L.audio_items.size());
    for (const gcf::Item &it : L.audio_items) { put(out, it.x); put(out, it.y); }
    put(out, (int)L.meta_items.size());
    for (const gcf::MetaItem &it : L.meta_items) { put(out, it.x); put(out, it.y); }
}

}  // namespace

int main(int argc, char **argv)
{
    FILE *in = argc > 2 ? fopen(argv[1], "rb") : nullptr;
    FILE *out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { printf("usage: gc_files_host_driver cases.bin results.bin\n"); return 2; }
    int n = 0;
    if (!read_n(in, &n, 1)) return 2;
    for (int i = 0; i < n; i++) {
        int kind = 0, nfiles = 0;
        if (!read_n(in, &kind, 1) || !read_n(in, &nfiles, 1)) return 2;
        const size_t count = nfiles > 0 ? (size_t)nfiles : 0;
        gcf::FilesLayout *L = new gcf::FilesLayout;
        g_error[0] = 0;
        int rc = 0;
        if (kind == 0) {
            int cfg[4];
            if (!read_n(in, cfg, 4)) return 2;
            vga_gc_file *files = static_cast<vga_gc_file *>(malloc(count * sizeof(vga_gc_file)));
            for (size_t f = 0; f < count; f++) {
                int v[8];
                if (!read_n(in, v, 8)) return 2;
                files[f].channels = v[0];
                files[f].sample_rate = v[1];
                files[f].channel = {v[2], v[3], v[4], v[5], v[6], v[7]};
            }
            vga_dsp_file_config *dsp = nullptr;
            if (cfg[0]) {
                dsp = static_cast<vga_dsp_file_config *>(malloc(sizeof *dsp));
                *dsp = {cfg[1], cfg[2], cfg[3]};
            }
            rc = gcf::make_layout(count ? files : nullptr, nfiles, dsp, *L);
            free(dsp);
            free(files);
        } else {
            int has_offsets = 0;
            if (!read_n(in, &has_offsets, 1)) return 2;
            vga_dsp_info **infos = static_cast<vga_dsp_info **>(malloc(count * sizeof(vga_dsp_info *)));
            for (size_t f = 0; f < count; f++) {
                int v[10];
                if (!read_n(in, v, 10)) return 2;
                vga_dsp_info *I = static_cast<vga_dsp_info *>(calloc(1, sizeof(vga_dsp_info)));
                I->channel_count = v[0]; I->sample_count = v[1]; I->nibble_count = v[2]; I->frames_per_interleave = v[3];
                I->audio_offset = v[4]; I->adpcm_bytes = v[5]; I->interleave_size = v[6]; I->data_length = v[7];
                I->looping = v[8]; I->sample_rate = v[9];
                infos[f] = I;
            }
            int64_t *offsets = has_offsets ? static_cast<int64_t *>(malloc(count * sizeof(int64_t))) : nullptr;
            if (has_offsets && !read_n(in, offsets, count)) return 2;
            rc = gcf::make_layout_from_dsp(count ? infos : nullptr, nfiles, offsets, *L);
            free(offsets);
            for (size_t f = 0; f < count; f++) free(infos[f]);
            free(infos);
        }
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
