// files_layout_driver.cpp -- vgaudio_amd/csrc/files_layout.hpp and gc_files_layout.hpp on their own (no HIP, no product library),
// for tests/test_files_layout_host.py, which builds it with -fsanitize=address,undefined and compares what it writes with a
// model of its own.
//
//   files_layout_driver <cases file> <results file>
//
// Cases file (little endian): int32 cases; per case int32 kind, then
//   0 IMAGES   int32 n, has_offsets; int64 size[n]; int64 offset[n] when has_offsets
//              -> n x { int64 at; int32 verdict }; int64 at, end, total()
//   1 COUNTER  int64 count so far; int32 n, rows (0: "channels", 1: "rows")      -> int32 rc; int64 count; message
//   2 GC ROWS  int32 nch; int32 samples[nch]; int32 seek entries[nch]
//              -> nch x { int64 pcm_off, adpcm_off, seek_off }; int32 channels; int64 pcm_samples, adpcm_bytes, seek shorts
//   3 OVERLAP  int32 n; int64 off[n]; int32 len[n]                                -> int32 found, a, b (-1, -1 when none)
//   4 META     int16 coefs[2][16], gain[2], start[2][3], loop[2][3]; int32 channel -> int16 v[23]
//   5 ROWS     int32 n, has_offsets; int64 limit; int64 length[n], room[n]; int64 offset[n] when has_offsets
//              -> n x { int64 at; int32 verdict }; int64 at, end
//   6 ITEMS    int32 fast, first, count; int64 per, unit; int32 fast items ({100 + i, i})
//              -> twice { int32 items; items x { int32 x; uint32 y } }; int32 what put_in_front returned
//   7 OPENING  int32 nfiles, have_array   -> check_files(.., "infos"): int32 rc; message;  name_file(3, -2) over "inner 5": rc; message
//   8 REGIONS  int32 n; int64 capacity; int32 has_out, has_count -> int32 rc; message; int64 count; int32 copied; copied x int64
// A message is int32 length and the bytes.  Every array handed to the headers is a heap block of exactly its size.
#include "../../vgaudio_amd/csrc/gc_files_layout.hpp"

#include <cstdarg>
#include <cstdio>

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

FILE *in, *out;

template <class T> T get()
{
    T v;
    if (fread(&v, sizeof(T), 1, in) != 1) { fprintf(stderr, "short cases file\n"); exit(2); }
    return v;
}
template <class T> std::vector<T> get_n(int n)
{
    std::vector<T> v((size_t)n);
    for (T &x : v) x = get<T>();
    return v;
}
template <class T> void put(const T &v) { fwrite(&v, sizeof(T), 1, out); }
void put_message()
{
    const int len = (int)strlen(g_error);
    put(len);
    fwrite(g_error, 1, (size_t)len, out);
}

struct Row { int64_t pcm_off, adpcm_off, seek_off; int entries; };
struct Totals { int channels; int64_t pcm_samples, adpcm_bytes; };
struct Info { int16_t coefs[2][16], gain[2], start_context[2][3], loop_context[2][3]; };
struct Meta { int16_t v[23]; };
struct Item { int x; uint32_t y; };

void images()
{
    const int n = get<int>(), has_offsets = get<int>();
    const std::vector<int64_t> size = get_n<int64_t>(n), offset = get_n<int64_t>(has_offsets ? n : 0);
    fileset::Images im;
    for (int i = 0; i < n; i++) {
        const fileset::Placed p = im.place(size[i], has_offsets ? &offset[i] : nullptr);
        put(p.at);
        put((int)p.verdict);
    }
    put(im.at);
    put(im.end);
    put(im.total());
}

void counter()
{
    int64_t count = get<int64_t>();
    const int n = get<int>(), rows = get<int>();
    put(fileset::count_rows(7, n, count, rows ? "rows" : "channels"));
    put(count);
    put_message();
}

void gc_rows()
{
    const int nch = get<int>();
    const std::vector<int> samples = get_n<int>(nch), entries = get_n<int>(nch);
    std::vector<Row> channel;
    Totals totals = {};
    gc::RaggedLayout rows;
    fileset::lay_out_rows(rows, samples, channel, totals);
    for (int c = 0; c < nch; c++) channel[c].entries = entries[c];
    const int64_t seek_shorts = fileset::lay_out_seek(channel);
    for (const Row &r : channel) { put(r.pcm_off); put(r.adpcm_off); put(r.seek_off); }
    put(totals.channels);
    put(totals.pcm_samples);
    put(totals.adpcm_bytes);
    put(seek_shorts);
}

void overlap()
{
    const int n = get<int>();
    const std::vector<int64_t> off = get_n<int64_t>(n);
    const std::vector<int> len = get_n<int>(n);
    int a = -1, b = -1;
    const bool found = fileset::find_overlap(n, [&](int i) { return off[i]; }, [&](int i) { return len[i]; }, a, b);
    put((int)found);
    put(found ? a : -1);
    put(found ? b : -1);
}

void meta()
{
    Info *I = new Info(get<Info>());
    const Meta m = fileset::fill_meta<Meta>(*I, get<int>());
    delete I;
    put(m);
}

void rows()
{
    const int n = get<int>(), has_offsets = get<int>();
    const int64_t limit = get<int64_t>();
    const std::vector<int64_t> length = get_n<int64_t>(n), room = get_n<int64_t>(n), offset = get_n<int64_t>(has_offsets ? n : 0);
    fileset::Rows r;
    for (int i = 0; i < n; i++) {
        const fileset::Placed p = r.place(length[i], room[i], limit, has_offsets ? &offset[i] : nullptr);
        put(p.at);
        put((int)p.verdict);
    }
    put(r.at);
    put(r.end);
}

void items()
{
    const int fast = get<int>(), first = get<int>(), count = get<int>();
    const int64_t per = get<int64_t>(), unit = get<int64_t>();
    const int nfast = get<int>();
    std::vector<Item> tables[2], front;
    fileset::cut_general_items(tables, fast != 0, first, count, per, unit);
    for (int i = 0; i < nfast; i++) front.push_back({100 + i, (uint32_t)i});
    const int put_front = fileset::put_in_front(tables[0], front);
    for (const std::vector<Item> &t : tables) {
        put((int)t.size());
        for (const Item &it : t) { put(it.x); put(it.y); }
    }
    put(put_front);
}

void opening()
{
    const int nfiles = get<int>(), have_array = get<int>();
    put(fileset::check_files(nfiles, have_array != 0, "infos"));
    put_message();
    set_error("inner %d", 5);
    put(fileset::name_file(3, -2));
    put_message();
}

void regions()
{
    const int n = get<int>();
    const int64_t capacity = get<int64_t>();
    const int has_out = get<int>(), has_count = get<int>();
    std::vector<int64_t> r, copied((size_t)(capacity > 0 ? capacity : 1), -1);     // (never a null data())
    for (int i = 0; i < n; i++) r.push_back(1000 + i);
    int64_t count = -1;
    const int rc = fileset::copy_regions(r, has_out ? copied.data() : nullptr, capacity, has_count ? &count : nullptr);
    put(rc);
    put_message();
    put(count);
    const int ncopied = rc == 0 && has_out ? n : 0;
    put(ncopied);
    for (int i = 0; i < ncopied; i++) put(copied[(size_t)i]);
}

}  // namespace

int main(int argc, char **argv)
{
    in = argc > 2 ? fopen(argv[1], "rb") : nullptr;
    out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { fprintf(stderr, "usage: files_layout_driver <cases> <results>\n"); return 2; }
    void (*const kinds[])() = {images, counter, gc_rows, overlap, meta, rows, items, opening, regions};
    const int cases = get<int>();
    for (int c = 0; c < cases; c++) {
        const int kind = get<int>();
        if (kind < 0 || kind >= (int)(sizeof kinds / sizeof kinds[0])) { fprintf(stderr, "case %d: no kind %d\n", c, kind); return 2; }
        g_error[0] = 0;
        kinds[kind]();
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("%d ok\n", cases);
    return 0;
}
