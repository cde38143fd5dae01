// gc_aligned_host_driver.cpp -- vgaudio_amd/csrc/gc_aligned_host.hpp on its own (tests/test_gc_aligned_host.py): the header
// with a set_error of this file's, no HIP and no product library, built with g++ -fsanitize=address,undefined and run as a
// child process.  `gc_aligned_host_driver cases.bin results.bin` runs every case of cases.bin and writes what the header
// answered:
//   cases.bin    int32 n; n x { int32 nfiles; nfiles x int32[8] (channels, sample_rate, the six fields of
//                vga_gcadpcm_channel_params) }
//   results.bin  per case: int32 rc, message length, message bytes; when rc == 0:
//                  int32 nfiles, nch, aligned channels, first_channel[nfiles], counts[nch], out_counts[nch], tail_counts[aligned];
//                  nch x { int64[7] (in pcm, in adpcm, out pcm, out adpcm, tail pcm, tail adpcm, seek offsets); int32[15] (file,
//                  tail_row, bytes_to_keep, samples_to_keep, samples_to_encode, head, loop_start, loop_length, loop_start_aligned,
//                  out_samples, out_bytes, spacing, entries, 0, 0) };
//                  int64[6] totals (pcm_samples, adpcm_bytes, out_pcm_samples, out_adpcm_bytes, seek_shorts, workspace_bytes);
//                  int64[8] workspace cut (in_pcm, tail_pcm, tail_adpcm, tail_coefs, hist1, hist2, scratch, scratch bytes);
//                  int32[4] any_aligned, any_seek, any_loop_start, ctx_past_file;
//                  three times (gather, adpcm, pcm): int32 items; items x { int32 x; uint32 y }; int32 meta items; items x int32[2]
// The encoder's scratch is handed in as 0 bytes (gc::encode_scratch_bytes lives in a kernel file): workspace_bytes ends where
// the scratch would begin.  Every array handed to the header is a heap block of exactly its size.  Prints "<cases> ok".
#include "../../vgaudio_amd/csrc/gc_aligned_host.hpp"

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

size_t no_scratch(int) { return 0; }

void put_items(FILE *out, const std::vector<gca::Item> &items)
{
    put(out, (int)items.size());
    for (const gca::Item &it : items) { put(out, it.x); put(out, it.y); }
}

void write_layout(FILE *out, const gca::AlignedLayout &L)
{
    const int nfiles = L.totals.files, nch = L.totals.channels, nal = L.totals.aligned_channels;
    put(out, nfiles);
    put(out, nch);
    put(out, nal);
    for (int f = 0; f < nfiles; f++) put(out, L.in.first_channel[f]);
    for (int c = 0; c < nch; c++) put(out, L.in.counts[c]);
    for (int c = 0; c < nch; c++) put(out, L.out_counts[c]);
    for (int c = 0; c < nal; c++) put(out, L.tail_counts[c]);
    for (int c = 0; c < nch; c++) {
        const gca::AlignRow &r = L.channel[c];
        const int64_t off[7] = {r.in_pcm_off, r.in_adpcm_off, r.out_pcm_off, r.out_adpcm_off, r.tail_pcm_off, r.tail_adpcm_off, r.seek_off};
        const int v[15] = {r.file, r.tail_row, r.bytes_to_keep, r.samples_to_keep, r.samples_to_encode, r.head, r.loop_start, r.loop_length,
                           r.loop_start_aligned, r.out_samples, r.out_bytes, r.spacing, r.entries, 0, 0};
        fwrite(off, sizeof off, 1, out);
        fwrite(v, sizeof v, 1, out);
    }
    const int64_t totals[6] = {L.totals.pcm_samples, L.totals.adpcm_bytes, L.totals.out_pcm_samples, L.totals.out_adpcm_bytes,
                               L.totals.seek_shorts, (int64_t)L.totals.workspace_bytes};
    fwrite(totals, sizeof totals, 1, out);
    const int64_t cut[8] = {(int64_t)L.ws.in_pcm_at, (int64_t)L.ws.tail_pcm_at, (int64_t)L.ws.tail_adpcm_at, (int64_t)L.ws.tail_coefs_at,
                            (int64_t)L.ws.hist1_at, (int64_t)L.ws.hist2_at, (int64_t)L.ws.scratch_at, (int64_t)L.ws.scratch_bytes};
    fwrite(cut, sizeof cut, 1, out);
    const int flags[4] = {L.any_aligned, L.any_seek, L.any_loop_start, L.ctx_past_file};
    fwrite(flags, sizeof flags, 1, out);
    put_items(out, L.gather_items);
    put_items(out, L.adpcm_items);
    put_items(out, L.pcm_items);
    put(out, (int)L.meta_items.size());
    for (const gca::MetaItem &it : L.meta_items) { put(out, it.x); put(out, it.y); }
}

}  // namespace

int main(int argc, char **argv)
{
    FILE *in = argc > 2 ? fopen(argv[1], "rb") : nullptr;
    FILE *out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { printf("usage: gc_aligned_host_driver cases.bin results.bin\n"); return 2; }
    int n = 0;
    if (!read_n(in, &n, 1)) return 2;
    for (int i = 0; i < n; i++) {
        int nfiles = 0;
        if (!read_n(in, &nfiles, 1)) return 2;
        const size_t count = nfiles > 0 ? (size_t)nfiles : 0;
        gca::AlignedLayout *L = new gca::AlignedLayout;
        g_error[0] = 0;
        vga_gc_file *files = static_cast<vga_gc_file *>(malloc(count * sizeof(vga_gc_file)));
        for (size_t f = 0; f < count; f++) {
            int v[8];
            if (!read_n(in, v, 8)) return 2;
            files[f].channels = v[0];
            files[f].sample_rate = v[1];
            files[f].channel = {v[2], v[3], v[4], v[5], v[6], v[7]};
        }
        const int rc = gca::make_layout(count ? files : nullptr, nfiles, no_scratch, *L);
        // the argument checks on pointers that are never followed
        if (rc == 0 && nfiles > 0) {
            char *base = reinterpret_cast<char *>((uintptr_t)0x10000);
            const size_t need = gca::workspace_needed(*L, false, true, true);
            if (gca::check_align(*L, base, base, base, nullptr, base, nullptr, base, need) != VGA_OK) return 3;
            if (gca::check_align(*L, base + 8, base, base, nullptr, base, nullptr, base, need) != VGA_ERR_ARGUMENT) return 3;
            if (need > 0 && gca::check_align(*L, base, base, base, nullptr, base, nullptr, base, need - 1) != VGA_ERR_ARGUMENT) return 3;
            if (gca::check_align(*L, base, base, base, nullptr, base, base, base, need) != (L->ctx_past_file >= 0 ? VGA_ERR_OUT_OF_RANGE : VGA_OK)) return 3;
            g_error[0] = 0;
        }
        free(files);
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
