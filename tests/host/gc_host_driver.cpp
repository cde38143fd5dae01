// gc_host_driver.cpp -- vgaudio_amd/csrc/gc_host.hpp on its own (tests/test_gc_host_layer.py): the header with a
// set_error of this file's, no HIP and no product library.  Built twice with g++:
//   * a shared library whose extern "C" wrappers the Python test compares with the product library's entry points and
//     with a model of its own;
//   * with -DGC_HOST_MAIN, AddressSanitizer and UBSan, a program that runs a file of cases the test wrote (int32 unless
//     said otherwise; `null`: 1 = no parameters, 2 = no output; a message is int32 length + bytes):
//       n; n x { p[6]; nch; null; rc; message; layout[4]; int64 workspace bytes }       channel_layout_for
//       n; n x { p[8]; nch; null; rc; message; layout[10] }                             dsp_layout_for
//       n; n x { count; lengths[count]; int64 pcm_base, adpcm_base, pcm_end, adpcm_end; order[count];
//                int64 pcm_off[count], adpcm_off[count] }                               RaggedLayout
//       n; n x { count; lengths[count]; chunk_units; m; chunk_begin[m] }                cut_chunks
//     Prints "<channel layouts> <dsp layouts> <ragged layouts> <chunk cuts> ok" and exits 0, or says what differs and exits 1.
#include "../../vgaudio_amd/csrc/gc_host.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

namespace {
thread_local char g_error[512];
}

void vga::set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

using namespace vga;

extern "C" {

const char *gh_last_error() { return g_error; }
long long gh_guard_bytes() { return gc::GUARD_BYTES; }
long long gh_chunk_samples() { return gc::CHUNK_SAMPLES; }

// the six conversions, in the order of the vga_gcadpcm_* exports
int gh_convert(int which, int v)
{
    switch (which) {
    case 0: return gc::nibble_count_to_sample_count(v);
    case 1: return gc::sample_count_to_nibble_count(v);
    case 2: return gc::nibble_to_sample(v);
    case 3: return gc::sample_to_nibble(v);
    case 4: return gc::sample_count_to_byte_count(v);
    default: return gc::byte_count_to_sample_count(v);
    }
}

int gh_channel_layout_for(const vga_gcadpcm_channel_params *p, vga_gcadpcm_channel_layout *out) { return gc::channel_layout_for(p, out); }
size_t gh_build_channels_workspace_bytes(int nch, const vga_gcadpcm_channel_params *p) { return gc::build_channels_workspace_bytes(nch, p); }
int gh_dsp_layout_for(const vga_dsp_params *p, int nch, vga_dsp_layout *out) { return gc::dsp_layout_for(p, nch, out); }

// plan_channels after channel_layout_for; out9: the plan's nine numbers
int gh_plan_channels(const vga_gcadpcm_channel_params *p, int nch, int want_ctx, long long *out9)
{
    vga_gcadpcm_channel_layout L;
    if (int rc = gc::channel_layout_for(p, &L)) return rc;
    gc::ChannelsPlan plan;
    if (int rc = gc::plan_channels(p, L, nch, want_ctx != 0, plan)) return rc;
    const long long v[9] = {plan.ws_pcm_pitch, plan.frames_to_keep, plan.bytes_to_keep, plan.samples_to_keep, plan.samples_to_encode,
                            plan.new_pitch, (long long)plan.new_pcm_at, (long long)plan.hist1_at, (long long)plan.hist2_at};
    memcpy(out9, v, sizeof v);
    return VGA_OK;
}

// totals8: pcm_end, adpcm_end, max_length, total_frames, uniform, pcm_pitch, adpcm_pitch, groups
void gh_ragged_layout(const int *lengths, int n, long long pcm_base, long long adpcm_base, int *order, long long *pcm_off,
                      long long *adpcm_off, int *group_frames, long long *totals8)
{
    gc::RaggedLayout L;
    L.lay_out(lengths, n, pcm_base, adpcm_base);
    for (int c = 0; c < n; c++) {
        order[c] = L.order[c];
        pcm_off[c] = L.pcm_off[c];
        adpcm_off[c] = L.adpcm_off[c];
    }
    for (size_t g = 0; g < L.group_frames.size(); g++) group_frames[g] = L.group_frames[g];
    const long long t[8] = {L.pcm_end, L.adpcm_end, L.max_length, L.total_frames, L.uniform ? 1 : 0, L.uniform ? L.pcm_pitch : 0,
                            L.uniform ? L.adpcm_pitch : 0, (long long)L.group_frames.size()};
    memcpy(totals8, t, sizeof t);
}

// returns the number of entries of chunk_begin (the last is n); at most `room` are written
int gh_cut_chunks(const int *counts, int n, int chunk_units, int *out, int room)
{
    const std::vector<int> b = gc::cut_chunks(counts, n, chunk_units);
    for (size_t i = 0; i < b.size() && (int)i < room; i++) out[i] = b[i];
    return (int)b.size();
}

int gh_longest_first(const int *counts, int n, int *order)
{
    const gc::LongestFirst lf(counts, n);
    for (size_t i = 0; i < lf.order.size(); i++) order[i] = lf.order[i];
    return lf.identity ? 1 : 0;
}

// rows of 16 (coefficients): gathered into the sorted order, then scattered back to the caller's
void gh_gather_scatter(const int *counts, int n, const int16_t *rows, int16_t *gathered, int16_t *back)
{
    const gc::LongestFirst lf(counts, n);
    const std::vector<int16_t> g = lf.gather_rows(rows, 16);
    std::copy(g.begin(), g.end(), gathered);
    lf.scatter_rows(g, 16, back);
}

// the check lists of the ragged host calls, on arrays the test built
int gh_check_encode_v(const int16_t *const *pcm, const int *counts, int nch, const int16_t *coefs_out, uint8_t *const *adpcm_out,
                      int with_coefs, const int16_t *coefs_in)
{
    return gc::check_encode_v(pcm, counts, nch, coefs_out, adpcm_out, with_coefs != 0, coefs_in);
}
int gh_check_decode_v(const uint8_t *const *adpcm, const int16_t *coefs, const int *counts, int nch, int16_t *const *pcm_out)
{
    return gc::check_decode_v(adpcm, coefs, counts, nch, pcm_out);
}

}  // extern "C"

#ifdef GC_HOST_MAIN
namespace {

FILE *g_file;

template <class T> std::vector<T> take(size_t count)
{
    std::vector<T> v(count);                                   // a heap block of exactly its size
    if (count && fread(v.data(), sizeof(T), count, g_file) != count) { printf("short cases file\n"); exit(2); }
    return v;
}
int take_int() { return take<int>(1)[0]; }
std::string take_message()
{
    const std::vector<char> m = take<char>((size_t)take_int());
    return std::string(m.begin(), m.end());
}

int fail(const char *what, int index, long long got, long long want)
{
    printf("%s %d: got %lld, want %lld (%s)\n", what, index, got, want, g_error);
    return 1;
}

// one refusing-or-not layout call against what the test recorded: its code, its message, the output's bytes
template <class Params, class Layout, class Call>
int run_layout_case(const char *what, int index, size_t param_ints, Call call)
{
    const std::vector<int> p = take<int>(param_ints);
    const int nch = take_int(), null = take_int(), want_rc = take_int();
    const std::string want_message = take_message();
    const std::vector<int> want = take<int>(sizeof(Layout) / sizeof(int));
    Params params;
    memcpy(&params, p.data(), sizeof params);
    Layout *out = new Layout;                                   // a heap block of exactly its size
    memset(out, 0x5A, sizeof *out);
    const int rc = call(null == 1 ? nullptr : &params, nch, null == 2 ? nullptr : out);
    const bool same = memcmp(out, want.data(), sizeof *out) == 0;
    delete out;
    if (rc != want_rc) return fail(what, index, rc, want_rc);
    if (rc && want_message != g_error) return fail("message", index, 0, 0);
    if (!same) return fail("layout bytes", index, 0, 0);
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    g_file = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!g_file) { printf("usage: gc_host_driver cases.bin\n"); return 2; }
    const int channels = take_int();
    for (int i = 0; i < channels; i++) {
        int nch_seen = 0;
        const vga_gcadpcm_channel_params *p_seen = nullptr;
        vga_gcadpcm_channel_params copy;
        if (run_layout_case<vga_gcadpcm_channel_params, vga_gcadpcm_channel_layout>(
                "channel_layout_for", i, 6, [&](const vga_gcadpcm_channel_params *p, int nch, vga_gcadpcm_channel_layout *out) {
                    nch_seen = nch;
                    if (p) { copy = *p; p_seen = &copy; }
                    return gc::channel_layout_for(p, out);
                }))
            return 1;
        const long long want_ws = take<long long>(1)[0];
        const long long ws = (long long)gc::build_channels_workspace_bytes(nch_seen, p_seen);
        if (ws != want_ws) return fail("workspace bytes", i, ws, want_ws);
        long long plan[9];
        if (p_seen) (void)gh_plan_channels(p_seen, nch_seen, 1, plan);
    }
    const int dsps = take_int();
    for (int i = 0; i < dsps; i++)
        if (run_layout_case<vga_dsp_params, vga_dsp_layout>("dsp_layout_for", i, 8, [](const vga_dsp_params *p, int nch, vga_dsp_layout *out) {
                return gc::dsp_layout_for(p, nch, out);
            }))
            return 1;
    const int raggeds = take_int();
    for (int i = 0; i < raggeds; i++) {
        const int n = take_int();
        const std::vector<int> lengths = take<int>(n);
        const std::vector<long long> ends = take<long long>(4);
        const std::vector<int> order = take<int>(n);
        const std::vector<long long> pcm_off = take<long long>(n), adpcm_off = take<long long>(n);
        gc::RaggedLayout L;
        L.lay_out(lengths.data(), n, ends[0], ends[1]);
        if (L.pcm_end != ends[2] || L.adpcm_end != ends[3]) return fail("ragged ends", i, L.pcm_end, ends[2]);
        for (int c = 0; c < n; c++)
            if (L.order[c] != order[c] || L.pcm_off[c] != pcm_off[c] || L.adpcm_off[c] != adpcm_off[c]) return fail("ragged row", i, c, c);
        const gc::LongestFirst lf(lengths.data(), n);
        for (int c = 0; c < n; c++)
            if (lf.order[c] != order[c]) return fail("longest first", i, lf.order[c], order[c]);
        std::vector<int16_t> rows((size_t)n * 16), back((size_t)n * 16);
        for (size_t k = 0; k < rows.size(); k++) rows[k] = (int16_t)(k * 7);
        lf.scatter_rows(lf.gather_rows(rows.data(), 16), 16, back.data());
        if (rows != back) return fail("gather / scatter", i, 0, 0);
    }
    const int cuts = take_int();
    for (int i = 0; i < cuts; i++) {
        const int n = take_int();
        const std::vector<int> counts = take<int>(n);
        const int chunk_units = take_int(), m = take_int();
        const std::vector<int> want = take<int>(m);
        const std::vector<int> got = gc::cut_chunks(counts.data(), n, chunk_units);
        if (got != want) return fail("cut_chunks", i, (long long)got.size(), m);
    }
    fclose(g_file);
    printf("%d %d %d %d ok\n", channels, dsps, raggeds, cuts);
    return 0;
}
#endif
