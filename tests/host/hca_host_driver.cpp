// hca_host_driver.cpp -- vgaudio_amd/csrc/hca_host.hpp on its own (tests/test_hca_host_layer.py): the header with a
// set_error of this file's, no HIP and no product library.  Built twice with g++:
//   * a shared library whose extern "C" wrappers the Python test compares with the product library's entry points;
//   * with -DHCA_HOST_MAIN, AddressSanitizer and UBSan, a program that runs a file of cases the test wrote:
//       int32 n; n x { int32 params[9]; int32 rc; vga_hca_info info }      CriHcaEncoder.Initialize, what the product gave
//       int32 m; m x { vga_hca_info info; int32 rc }                       headers for make_device_info and its code
//     Prints "<initialized> <refused> <device infos> ok" and exits 0, or says what differs and exits 1.
#include "../../vgaudio_amd/csrc/hca_host.hpp"

#include <cstdarg>
#include <cstdio>

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

namespace {

// every Encode() call of the streaming shell until its guard refuses (CriHcaEncoder.cs:128-131): counts[i] = frames of call
// i, -1 for a call the guard refuses.  Returns the number of calls walked.
int walk_stream(const vga_hca_info &h, int *counts, int calls)
{
    hca::StreamCounters c = hca::stream_counters_for(h);
    for (int i = 0; i < calls; i++) counts[i] = hca::stream_finished(c, h) ? -1 : c.advance_one_block(h);
    return calls;
}

}  // namespace

extern "C" {

const char *hh_last_error() { return g_error; }
int hh_encoder_initialize(const vga_hca_params *p, vga_hca_info *h) { return hca::encoder_initialize(p, h); }

int hh_make_device_info(const vga_hca_info *h, void *out, int out_bytes)
{
    if (out_bytes < (int)sizeof(hca::DeviceInfo)) return VGA_ERR_ARGUMENT;
    hca::DeviceInfo d;
    if (int rc = hca::make_device_info(*h, d)) return rc;
    memcpy(out, &d, sizeof d);
    return VGA_OK;
}

// as vga_testing_hca_decode_classes: the number of classes, or the code of the first header make_device_info refuses
int hh_decode_classes(const vga_hca_info *h, int n, int *class_out)
{
    std::vector<hca::DeviceInfo> dev(n);
    for (int s = 0; s < n; s++)
        if (int rc = hca::make_device_info(h[s], dev[s])) return rc;
    std::vector<int> cls;
    const int classes = hca::decode_classes(dev.data(), n, cls);
    for (int s = 0; s < n; s++) class_out[s] = cls[s];
    return classes;
}

int hh_status_to_error(int status) { return hca::status_to_error(status); }
int hh_stream_counts(const vga_hca_info *h, int *counts, int calls) { return walk_stream(*h, counts, calls); }
int hh_bitrate_too_low(const vga_hca_info *h) { return hca::bitrate_too_low(*h) ? 1 : 0; }
long long hh_frames_pitch(const vga_hca_info *h) { return hca::frames_pitch_for(*h); }

}  // extern "C"

#ifdef HCA_HOST_MAIN
namespace {

bool read_ints(FILE *f, void *out, size_t count) { return fread(out, sizeof(int), count, f) == count; }

int fail(const char *what, int index, int got, int want)
{
    printf("%s %d: got %d, want %d (%s)\n", what, index, got, want, g_error);
    return 1;
}

}  // namespace

int main(int argc, char **argv)
{
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) { printf("usage: hca_host_driver cases.bin\n"); return 2; }
    int n = 0, initialized = 0, refused = 0, device_infos = 0;
    if (!read_ints(f, &n, 1)) return 2;
    std::vector<vga_hca_info> good;
    for (int i = 0; i < n; i++) {
        vga_hca_params p;
        vga_hca_info want, got;
        int want_rc = 0;
        if (!read_ints(f, &p, 9) || !read_ints(f, &want_rc, 1) || !read_ints(f, &want, sizeof want / sizeof(int))) return 2;
        const int rc = hca::encoder_initialize(&p, &got);
        if (rc != want_rc) return fail("Initialize", i, rc, want_rc);
        if (rc) { refused++; continue; }
        if (memcmp(&got, &want, sizeof got) != 0) return fail("Initialize fields", i, 0, 0);
        initialized++;
        // the walk of the whole stream on heap blocks of exactly its calls: every frame comes out, then the guard refuses
        const int calls = std::max(1, hca::divide_by_round_up(got.sample_count, hca::SPF)) + 1;
        std::vector<int> counts(calls);
        walk_stream(got, counts.data(), calls);
        int sum = 0;
        for (int k = 0; k + 1 < calls; k++) {
            if (counts[k] < 0) return fail("stream walk ends early", i, k, calls - 1);
            sum += counts[k];
        }
        if (sum != got.frame_count || counts[calls - 1] != -1) return fail("stream walk", i, sum, got.frame_count);
        hca::DeviceInfo d;
        if (hca::make_device_info(got, d) == VGA_OK) {
            good.push_back(got);
            device_infos++;
        }
        (void)hca::bitrate_too_low(got);
        (void)hca::frames_pitch_for(got);
    }
    std::vector<int> cls(good.size());
    if (hh_decode_classes(good.data(), (int)good.size(), cls.data()) < 1) return fail("classes", 0, 0, 1);
    int m = 0;
    if (!read_ints(f, &m, 1)) return 2;
    for (int i = 0; i < m; i++) {
        vga_hca_info h;
        int want_rc = 0;
        if (!read_ints(f, &h, sizeof h / sizeof(int)) || !read_ints(f, &want_rc, 1)) return 2;
        hca::DeviceInfo *d = new hca::DeviceInfo;               // a heap block of exactly its size
        const int rc = hca::make_device_info(h, *d);
        delete d;
        if (rc != want_rc) return fail("make_device_info", i, rc, want_rc);
        device_infos++;
    }
    for (int bits = 0; bits < 64; bits++) (void)hca::status_to_error(bits);
    fclose(f);
    printf("%d %d %d ok\n", initialized, refused, device_infos);
    return 0;
}
#endif
