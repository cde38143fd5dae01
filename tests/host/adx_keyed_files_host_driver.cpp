// adx_keyed_files_host_driver.cpp -- vgaudio_amd/csrc/adx_lcg.hpp and adx_keyed_files_host.hpp on their own
// (tests/test_adx_keyed_files_host.py): the headers with a set_error / last_error of this file's, no HIP and no product
// library, built with g++ -fsanitize=address,undefined and run as a child process.
// `adx_keyed_files_host_driver cases.bin results.bin`:
//   cases.bin    int32 nkeys; nkeys x int32[3] (seed, mult, inc); int32 ncheck; ncheck x int64 k (ascending);
//                int32 npairs; npairs x int64[2] (a, b);
//                int32 nsets; nsets x { int32 kind, nfiles, noffsets;
//                  kind 0 (a set for writing): nfiles x int32[13] (channels, the fields of vga_adx_file_params);
//                  kind 1 (for reading): nfiles x int32[7] (channel_count, frame_size, frame_count, audio_bytes, audio_offset,
//                         version, revision);
//                  int64 offsets[noffsets]; int32 ncalls; ncalls x { int32 what; int64 a[6]; int32 n[2]; int64 bytes } }
//                  what 0 write (a: audio, history, keys, images; n[0]: nkeys), 1 read (a: images, keys, audio; n[0]),
//                  2 find (a: images, keys, index_out, workspace; n: nkeys8, nkeys9; bytes), 3 workspace size (n), 4 find items
//   results.bin  int64 jump_mismatches (the jump against serial stepping, every key, every k up to 70 000 and every k of
//                the list), int64 compose_mismatches (power(a + b) against power(a) then power(b));
//                per set: int32 rc of the layout; per call: int32 rc, message length, message bytes;
//                what 3: int64 bytes; what 4: int32 count, count x int32[3]
// Pointers are numbers: the checks look at null and alignment only.  Prints "<sets> ok".
#include "../../vgaudio_amd/csrc/adx_keyed_files_host.hpp"
#include "../../vgaudio_amd/csrc/adx_lcg.hpp"

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

constexpr int64_t kDense = 70000;

// The state after k serial steps of every key against the jump, for k = 0 .. kDense and every k of `checks`.  Up to kDense
// the steps are taken one by one.  A state of 15 bits repeats within 2^15 steps, so the walk also notes when it first saw
// every state: from the first repeat on, step k is the step at the same place of the cycle -- still nothing but stepping.
int64_t jump_mismatches(const std::vector<vga_adx_key> &keys, const std::vector<int64_t> &checks)
{
    int64_t bad = 0;
    for (const vga_adx_key &key : keys) {
        const unsigned seed = (unsigned)key.seed & 0x7fffu, m = (unsigned)key.mult, c = (unsigned)key.inc;
        std::vector<unsigned> walk;                            // walk[k]: the state after k steps
        std::vector<int64_t> seen(0x8000, -1);
        int64_t cycle_start = -1, period = 0;
        unsigned x = seed;
        for (int64_t k = 0; k <= kDense; k++) {
            walk.push_back(x);
            if (cycle_start < 0 && seen[x] >= 0) { cycle_start = seen[x]; period = k - seen[x]; }
            if (seen[x] < 0) seen[x] = k;
            bad += adxlcg::apply(adxlcg::lcg_power(m, c, (uint64_t)k), seed) != x;
            x = (x * m + c) & 0x7fffu;
        }
        if (cycle_start < 0) return -1;                        // (cannot be: kDense > 2^15)
        for (int64_t k : checks) {
            const unsigned want = k <= kDense ? walk[(size_t)k] : walk[(size_t)(cycle_start + (k - cycle_start) % period)];
            bad += adxlcg::apply(adxlcg::lcg_power(m, c, (uint64_t)k), seed) != want;
        }
    }
    return bad;
}

int64_t compose_mismatches(const std::vector<vga_adx_key> &keys, const std::vector<int64_t> &pairs)
{
    int64_t bad = 0;
    for (const vga_adx_key &k : keys)
        for (size_t i = 0; i + 1 < pairs.size(); i += 2) {
            const unsigned m = (unsigned)k.mult, c = (unsigned)k.inc;
            const adxlcg::Affine both = adxlcg::lcg_power(m, c, (uint64_t)(pairs[i] + pairs[i + 1]));
            const adxlcg::Affine chain = adxlcg::then(adxlcg::lcg_power(m, c, (uint64_t)pairs[i]), adxlcg::lcg_power(m, c, (uint64_t)pairs[i + 1]));
            bad += both.a != chain.a || both.c != chain.c;
        }
    return bad;
}

void put_message(FILE *out, int rc)
{
    put(out, rc);
    const int len = rc ? (int)strlen(g_error) : 0;
    put(out, len);
    fwrite(g_error, 1, (size_t)len, out);
}

}  // namespace

int main(int argc, char **argv)
{
    FILE *in = argc > 2 ? fopen(argv[1], "rb") : nullptr;
    FILE *out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { printf("usage: adx_keyed_files_host_driver cases.bin results.bin\n"); return 2; }
    int nkeys = 0, ncheck = 0, npairs = 0, nsets = 0;
    if (!read_n(in, &nkeys, 1)) return 2;
    std::vector<vga_adx_key> keys((size_t)nkeys);
    if (!read_n(in, keys.data(), keys.size()) || !read_n(in, &ncheck, 1)) return 2;
    std::vector<int64_t> checks((size_t)ncheck);
    if (!read_n(in, checks.data(), checks.size()) || !read_n(in, &npairs, 1)) return 2;
    std::vector<int64_t> pairs((size_t)npairs * 2);
    if (!read_n(in, pairs.data(), pairs.size())) return 2;
    put(out, jump_mismatches(keys, checks));
    put(out, compose_mismatches(keys, pairs));
    if (!read_n(in, &nsets, 1)) return 2;
    for (int i = 0; i < nsets; i++) {
        int head[3];
        if (!read_n(in, head, 3)) return 2;
        const int kind = head[0], nfiles = head[1], noffsets = head[2];
        const size_t count = nfiles > 0 ? (size_t)nfiles : 0;
        g_error[0] = 0;
        adxf::FilesLayout *L = new adxf::FilesLayout;
        vga_adx_file *files = nullptr;
        vga_adx_file_info **infos = nullptr;
        if (kind == 0) {
            files = static_cast<vga_adx_file *>(malloc(count * sizeof(vga_adx_file)));
            for (size_t f = 0; f < count; f++) {
                int v[13];
                if (!read_n(in, v, 13)) return 2;
                files[f] = {v[0], {v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12]}};
            }
        } else {
            infos = static_cast<vga_adx_file_info **>(malloc(count * sizeof(vga_adx_file_info *)));
            for (size_t f = 0; f < count; f++) {
                int v[7];
                if (!read_n(in, v, 7)) return 2;
                vga_adx_file_info *I = static_cast<vga_adx_file_info *>(calloc(1, sizeof(vga_adx_file_info)));
                I->channel_count = v[0]; I->frame_size = v[1]; I->frame_count = v[2]; I->audio_bytes = v[3];
                I->audio_offset = v[4]; I->version = v[5]; I->revision = v[6];
                infos[f] = I;
            }
        }
        int64_t *offsets = noffsets > 0 ? static_cast<int64_t *>(malloc((size_t)noffsets * sizeof(int64_t))) : nullptr;
        if (noffsets > 0 && !read_n(in, offsets, (size_t)noffsets)) return 2;
        int rc = kind == 0 ? adxf::make_layout(count ? files : nullptr, nfiles, offsets, *L)
                           : adxf::make_layout_from_infos(count ? infos : nullptr, nfiles, offsets, *L);
        free(offsets);
        free(files);
        for (size_t f = 0; infos && f < count; f++) free(infos[f]);
        free(infos);
        put(out, rc);
        int ncalls = 0;
        if (!read_n(in, &ncalls, 1)) return 2;
        for (int c = 0; c < ncalls; c++) {
            int what = 0, n[2];
            int64_t a[6], bytes = 0;
            if (!read_n(in, &what, 1) || !read_n(in, a, 6) || !read_n(in, n, 2) || !read_n(in, &bytes, 1)) return 2;
            auto p = [&](int k) { return reinterpret_cast<const void *>((uintptr_t)a[k]); };
            g_error[0] = 0;
            if (what == 0) put_message(out, adxk::check_keyed_write(*L, p(0), p(1), p(2), n[0], p(3)));
            else if (what == 1) put_message(out, adxk::check_keyed_read(*L, p(0), p(1), n[0], p(2)));
            else if (what == 2) put_message(out, adxk::check_find(*L, p(0), p(1), n[0], n[1], p(2), p(3), (uint64_t)bytes));
            else if (what == 3) {
                put_message(out, 0);
                put(out, adxk::find_workspace_bytes(*L, n[0], n[1]));
            } else {
                std::vector<vga_adx_find_keys_item> items;
                adxk::describe_find_items(*L, items);
                put_message(out, 0);
                put(out, (int)items.size());
                for (const vga_adx_find_keys_item &it : items) { put(out, it.file); put(out, it.first_slot); put(out, it.slot_count); }
            }
        }
        delete L;
    }
    fclose(in);
    fclose(out);
    printf("%d ok\n", nsets);
    return 0;
}
