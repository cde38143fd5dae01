// hca_keyed_files_host_driver.cpp -- the HIP-free host layer of include/vgaudio_hip_files/hca_keyed_files.h
// (vgaudio_amd/csrc/hca_keyed_files_host.hpp) and the shared frame walk (hca_keyed_walk.hpp) as a stand-alone program with a
// set_error / last_error of this file's, no HIP and no product library, built with g++ -fsanitize=address,undefined and run
// as a child process (tests/test_hca_keyed_files_host.py).  It reads the case table's files, frames and tables and the calls
// to check from argv[1] and writes to argv[2]:
//   per file: first tested frame, tested frames; per candidate of the "singles" the search's answer over that one candidate
//   (index, status); per candidate list the file's (index, status)
//   per set and call: the code, the message, and the workspace size or the work items where the call has them
// The two per-file functions hca_files_host.hpp calls are stand-ins, as in hca_files_host_driver.cpp.
#include "../../vgaudio_amd/csrc/hca_keyed_files_host.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace tables {
#define HCA_TABLE_QUAL static const
#include "../../vgaudio_amd/csrc/hca_tables_data.h"
}

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
    return h ? h->header_size + h->frame_size * h->frame_count : VGA_ERR_ARGUMENT;
}
extern "C" int vga_hca_file_header(const vga_hca_info *h, const char *, float, int, int, uint8_t *header_out)
{
    memset(header_out, 0, (size_t)h->header_size);
    return VGA_OK;
}

using namespace vga;

namespace {

struct In {
    std::vector<uint8_t> d;
    size_t at = 0;
    template <class T> T take()
    {
        T v;
        if (at + sizeof v > d.size()) { fprintf(stderr, "cases file too short\n"); exit(2); }
        memcpy(&v, d.data() + at, sizeof v);
        at += sizeof v;
        return v;
    }
    const uint8_t *bytes(size_t n)
    {
        if (at + n > d.size()) { fprintf(stderr, "cases file too short\n"); exit(2); }
        const uint8_t *p = d.data() + at;
        at += n;
        return p;
    }
};
struct Out {
    FILE *f;
    template <class T> void put(T v) { fwrite(&v, sizeof v, 1, f); }
    void answer(int rc)
    {
        const char *msg = rc ? last_error() : "";
        put<int>(rc);
        put<int>((int)strlen(msg));
        fwrite(msg, 1, strlen(msg), f);
    }
};

enum { FIND = 0, READ = 1, WORKSPACE = 2, ITEMS = 3 };

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    In in;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END);
        in.d.resize((size_t)ftell(f));
        fseek(f, 0, SEEK_SET);
        if (fread(in.d.data(), 1, in.d.size(), f) != in.d.size()) return 2;
        fclose(f);
    }
    Out out = {fopen(argv[2], "wb")};
    if (!out.f) return 2;

    hcak::WalkTables T;
    memset(&T, 0, sizeof T);
    memcpy(T.dec_bits, tables::HCA_QuantizedSpectrumBits, sizeof T.dec_bits);
    memcpy(T.max_bits, tables::HCA_QuantizedSpectrumMaxBits, sizeof T.max_bits);
    memcpy(T.res_curve, tables::HCA_ScaleToResolutionCurve, 59);

    if (in.take<int>() != (int)sizeof(vga_hca_file_info)) { fprintf(stderr, "vga_hca_file_info differs\n"); return 2; }
    const int ncodes = in.take<int>();
    const uint8_t *dec_at = in.bytes((size_t)ncodes * 256);
    std::vector<uint8_t> dec(dec_at, dec_at + (size_t)ncodes * 256);
    const int nfiles = in.take<int>();
    std::vector<vga_hca_file_info> infos((size_t)nfiles);
    std::vector<std::vector<uint8_t>> frames((size_t)nfiles);
    std::vector<int> singles((size_t)nfiles);
    for (int f = 0; f < nfiles; f++) {
        infos[f] = in.take<vga_hca_file_info>();
        singles[f] = in.take<int>();
        const int64_t n = in.take<int64_t>();
        const uint8_t *p = in.bytes((size_t)n);
        frames[f].assign(p, p + n);                        // a buffer of exactly the stream's size: ASan sees a byte too far
    }
    const int nlists = in.take<int>();
    std::vector<std::vector<int>> lists((size_t)nlists);
    std::vector<int> type1((size_t)nlists);
    for (int l = 0; l < nlists; l++) {
        const int n = in.take<int>();
        type1[l] = in.take<int>();
        for (int k = 0; k < n; k++) lists[l].push_back(in.take<int>());
    }

    // ---- the search over the shared walk
    for (int f = 0; f < nfiles; f++) {
        hcak::WalkFile w;
        hcak::make_walk_file(infos[f].hca, infos[f].encryption_type, 0, w);
        if (!w.usable) { fprintf(stderr, "file %d: %s\n", f, last_error()); return 2; }
        int first = 0, ntest = 0;
        hcak::first_tested_frame(frames[f].data(), w.frame_count, w.frame_size, first, ntest);
        out.put<int>(first);
        out.put<int>(ntest);
        for (int k = 0; k < singles[f]; k++) {
            int index, status;
            hcak::host_find_key(w, T, frames[f].data(), dec.data() + (size_t)k * 256, 1, -1, index, status);
            out.put<int>(index);
            out.put<int>(status);
        }
        for (int l = 0; l < nlists; l++) {
            std::vector<uint8_t> tab;
            for (int k : lists[l]) tab.insert(tab.end(), dec.begin() + (size_t)k * 256, dec.begin() + (size_t)(k + 1) * 256);
            int index, status;
            hcak::host_find_key(w, T, frames[f].data(), tab.data(), (int)lists[l].size(), type1[l], index, status);
            out.put<int>(index);
            out.put<int>(status);
        }
    }

    // ---- the checks: sets of the first `count` files, made for reading without keys (0), with keys of their own (1), for
    // writing (2), for reading with a type-56 file whose header the walk cannot use (3)
    const int nsets = in.take<int>();
    for (int s = 0; s < nsets; s++) {
        const int kind = in.take<int>(), count = in.take<int>();
        std::vector<vga_hca_file_info> mine(infos.begin(), infos.begin() + count);
        if (kind == 3)                                     // nine channels: no frame of the first type-56 file can be unpacked
            for (vga_hca_file_info &i : mine)
                if (i.encryption_type == 56) { i.hca.channel_count = 9; break; }
        std::vector<const vga_hca_file_info *> ptrs;
        for (int f = 0; f < count; f++) ptrs.push_back(&mine[f]);
        hcaf::FilesLayout L;
        int rc = VGA_OK;
        if (kind == 2) {
            std::vector<vga_hca_file> files((size_t)count);
            for (int f = 0; f < count; f++) files[f] = {infos[f].hca, nullptr, 1.0f, 0, 0, -1};
            rc = hcaf::make_layout(files.data(), count, nullptr, nullptr, 0, true, L);
        } else {
            std::vector<int> keys((size_t)count, 0);
            rc = hcaf::make_layout_from_infos(ptrs.data(), count, nullptr, kind == 1 ? keys.data() : nullptr, kind == 1 ? dec.data() : nullptr,
                                              kind == 1 ? 1 : 0, true, nullptr, L);
        }
        out.answer(rc);
        if (rc) return 3;
        hcak::FindTables F;
        hcak::make_find_tables(L, F);
        const int ncalls = in.take<int>();
        for (int c = 0; c < ncalls; c++) {
            const int what = in.take<int>();
            int64_t a[4];
            for (int64_t &x : a) x = in.take<int64_t>();
            const int n0 = in.take<int>(), n1 = in.take<int>();
            const int64_t bytes = in.take<int64_t>();
            auto p = [&](int i) { return reinterpret_cast<const void *>((uintptr_t)a[i]); };   // never dereferenced
            if (what == FIND) out.answer(hcak::check_find(L, F, p(0), p(1), n0, n1, p(2), p(3), (uint64_t)bytes));
            else if (what == READ) out.answer(hcak::check_keyed_read(L, p(0), p(1), n0, p(2)));
            else if (what == WORKSPACE) {
                out.answer(VGA_OK);
                out.put<int64_t>(hcak::find_workspace_bytes(L, n0));
            } else {
                std::vector<vga_hca_find_keys_item> v;
                hcak::describe_find_items(L.encryption_type, n0, v);
                out.answer(VGA_OK);
                out.put<int>((int)v.size());
                for (const vga_hca_find_keys_item &i : v) { out.put<int>(i.file); out.put<int>(i.first_key); out.put<int>(i.key_count); }
            }
        }
    }
    if (in.at != in.d.size()) { fprintf(stderr, "cases file has %zu bytes left\n", in.d.size() - in.at); return 2; }
    fclose(out.f);
    printf("%d ok\n", nsets);
    return 0;
}
