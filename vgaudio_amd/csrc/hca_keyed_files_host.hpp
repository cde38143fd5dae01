// hca_keyed_files_host.hpp -- the host side of include/vgaudio_hip_files/hca_keyed_files.h without HIP: the argument checks of
// the keyed calls, what the search needs of every file (hcak::WalkFile, built at create from the parsed headers the set keeps),
// the size and shape of the search's workspace, the search's work items, and the search itself on host memory over the same
// walk the kernels run (hca_keyed_walk.hpp) -- the model the CPU tests hold against the oracle.  Header-only and free of
// <hip/hip_runtime.h> (tests/host/hca_keyed_files_host_driver.cpp includes it as capi_hca_keyed_files.hip does).
#pragma once
#include "hca_files_host.hpp"
#include "hca_host.hpp"
#include "hca_keyed_walk.hpp"
#include "../../include/vgaudio_hip_files/hca_keyed_files.h"

namespace vga {
namespace hcak {

constexpr int KEY_BLOCK = 64;                    // candidates per work item: one lane each
constexpr int STAGE_MAX_FRAME = 2048;            // a first tested frame of up to this many bytes is staged in LDS
constexpr int STAGE_REST_BYTES = 9216;           // the later tested frames are staged when together they are no longer
constexpr int TABLE_STRIDE = 260;                // of a candidate's table in LDS: 65 dwords, so lanes on one byte value hit 64 banks

// ---- what the search needs of the set's files
struct FindTables {
    std::vector<WalkFile> walk;                  // per file
    std::vector<int> find_files;                 // the type-56 files, ascending
    int max_channels = 1;                        // of the usable type-56 files
};

inline void make_walk_file(const vga_hca_info &h, int encryption_type, int64_t frames_off, WalkFile &w)
{
    std::memset(&w, 0, sizeof w);
    w.frames_off = frames_off;
    w.frame_size = h.frame_size;
    w.frame_count = h.frame_count;
    w.encryption_type = encryption_type;
    hca::DeviceInfo d;
    if (hca::make_device_info(h, d) != VGA_OK) return;        // (usable stays 0)
    w.usable = 1;
    w.nch = d.nch;
    for (int c = 0; c < 8; c++) {
        w.coded_count[c] = (uint8_t)d.coded_count[c];
        w.skip_bits[c] = (uint8_t)(d.channel_type[c] == hca::CH_STEREO_SECONDARY ? 32 : (d.hfr_group_count > 0 ? 6 * d.hfr_group_count : 0));
    }
    std::memcpy(w.ath_curve, d.ath_curve, 128);
}

inline void make_find_tables(const hcaf::FilesLayout &L, FindTables &F)
{
    F = FindTables();
    if (!L.from_infos) return;
    F.walk.resize(L.hca.size());
    for (size_t f = 0; f < L.hca.size(); f++) {
        make_walk_file(L.hca[f], L.encryption_type[f], L.tab[f].src_off, F.walk[f]);
        if (L.encryption_type[f] != 56) continue;
        F.find_files.push_back((int)f);
        if (F.walk[f].usable) F.max_channels = std::max(F.max_channels, F.walk[f].nch);
    }
}

// ---- the workspace: first tested frame and number of tested frames per file (two ints each), then one outcome byte per
// (file, candidate), file after file
inline int64_t find_workspace_bytes(const hcaf::FilesLayout &L, int nkeys)
{
    if (!L.from_infos || nkeys < 0) return 0;
    const int64_t n = L.totals.files;
    return 8 * n + hcaf::pad_to(n * nkeys, 4);
}

// ---- the work items of the two test launches: every (type-56 file, candidate) lies in exactly one
inline void describe_find_items(const std::vector<int> &encryption_type, int nkeys, std::vector<vga_hca_find_keys_item> &out)
{
    for (size_t f = 0; f < encryption_type.size(); f++)
        if (encryption_type[f] == 56)
            for (int k = 0; k < nkeys; k += KEY_BLOCK) out.push_back({(int)f, k, std::min(KEY_BLOCK, nkeys - k)});
}
inline int64_t find_item_count(int64_t find_files, int nkeys) { return find_files * (((int64_t)nkeys + KEY_BLOCK - 1) / KEY_BLOCK); }

// ---- the calls' argument checks
inline int check_keyed_set(const hcaf::FilesLayout &L, const char *what)
{
    if (!L.from_infos) { set_error("%s: the set was not made from parsed headers (vga_hca_files_create_from_infos)", what); return VGA_ERR_INVALID_OP; }
    if (!L.tables.empty()) { set_error("%s: the set was created with keys of its own: two sources of keys in one call", what); return VGA_ERR_INVALID_OP; }
    return VGA_OK;
}

inline int check_keyed_read(const hcaf::FilesLayout &L, const void *d_images, const void *d_tables, int ntables, const void *d_frames)
{
    const char *what = "vga_hca_read_keyed_device_v";
    if (int rc = check_keyed_set(L, what)) return rc;
    if (ntables <= 0) { set_error("%s: %d tables: a keyed call needs at least one", what, ntables); return VGA_ERR_ARGUMENT; }
    if (!d_tables) { set_error("%s: null d_tables", what); return VGA_ERR_ARGUMENT; }
    return hcaf::check_read(L, d_images, d_frames, what);
}

inline int check_find(const hcaf::FilesLayout &L, const FindTables &F, const void *d_images, const void *d_tables, int nkeys, int type1_index,
                      const void *d_key_index_out, const void *d_workspace, uint64_t workspace_bytes)
{
    const char *what = "vga_hca_find_keys_device_v";
    if (int rc = check_keyed_set(L, what)) return rc;
    if (nkeys < 0) { set_error("%s: negative candidate count %d", what, nkeys); return VGA_ERR_ARGUMENT; }
    if (type1_index < -1) { set_error("%s: type1_index %d below -1", what, type1_index); return VGA_ERR_ARGUMENT; }
    if (nkeys > 0 && !d_tables) { set_error("%s: null d_tables", what); return VGA_ERR_ARGUMENT; }
    if (!d_key_index_out) { set_error("%s: null d_key_index_out", what); return VGA_ERR_ARGUMENT; }
    if (!d_images && L.moving_files > 0) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (!hcaf::aligned_to(d_images, 16)) { set_error("%s: d_images needs 16-byte alignment", what); return VGA_ERR_ARGUMENT; }
    for (int f : F.find_files)
        if (!F.walk[f].usable) { set_error("%s: file %d: HcaInfo is inconsistent: no frame of it can be unpacked", what, f); return VGA_ERR_ARGUMENT; }
    if (find_item_count((int64_t)F.find_files.size(), nkeys) > 0x7FFFFFFF) { set_error("%s: more than 2^31 work items", what); return VGA_ERR_ARGUMENT; }
    const int64_t need = find_workspace_bytes(L, nkeys);
    if (need > 0 && (!d_workspace || workspace_bytes < (uint64_t)need || ((uintptr_t)d_workspace & 3))) {
        set_error("%s: the workspace needs %lld bytes at an int boundary (vga_hca_find_keys_workspace_bytes), %llu given", what, (long long)need,
                  d_workspace ? (unsigned long long)workspace_bytes : 0ull);
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}

// ---- the search on host memory, over the same walk: what the kernels must give
struct HostBytes {
    const uint8_t *frame, *sub;
    unsigned plain(int i) const { return sub[frame[i]]; }
};
struct HostRes {
    uint32_t words[8][16];
    void put(int c, int w, uint32_t v) { words[c][w] = v; }
    uint32_t word(int c, int w) const { return words[c][w]; }
};

// FindFirstNonEmptyFrame (CriHcaEncryption.cs:65-88) and the number of frames TestKey reads
inline void first_tested_frame(const uint8_t *frames, int frame_count, int frame_size, int &first, int &ntest)
{
    first = 0;
    for (int j = 0; j < frame_count; j++) {
        bool any = false;
        for (int i = 2; i < frame_size - 2 && !any; i++) any = frames[(size_t)j * frame_size + i] != 0;
        if (any) { first = j; break; }
    }
    ntest = std::min(FRAMES_TO_TEST, frame_count - first);
}

// one candidate over the tested frames: FRAME_PASSES / FRAME_FAILS / FRAME_BAD_SYNC
inline int host_test_key(const WalkFile &w, const WalkTables &T, const uint8_t *frames, int first, int ntest, const uint8_t *table)
{
    int first_fail = ntest, first_bad = ntest;
    for (int j = 0; j < ntest; j++) {
        HostBytes b = {frames + (size_t)(first + j) * w.frame_size, table};
        HostRes res;
        const int r = walk_frame(w, T, b, res);
        if (r == FRAME_FAILS) first_fail = std::min(first_fail, j);
        if (r == FRAME_BAD_SYNC) first_bad = std::min(first_bad, j);
    }
    return candidate_outcome(first_fail, first_bad, ntest);
}

// index and status of one file, the FIND rules of the header; `frames` = the file's frames as they lie in the image
inline void host_find_key(const WalkFile &w, const WalkTables &T, const uint8_t *frames, const uint8_t *tables, int nkeys, int type1_index,
                          int &index, int &status)
{
    index = -1;
    status = 0;
    if (w.encryption_type == 1) index = type1_index;
    if (w.encryption_type != 56) return;
    status = 1;
    if (nkeys == 0) return;
    int first, ntest;
    first_tested_frame(frames, w.frame_count, w.frame_size, first, ntest);
    if (w.frame_count == 0) { index = 0; status = 0; return; }
    for (int k = 0; k < nkeys; k++) {
        const int o = host_test_key(w, T, frames, first, ntest, tables + (size_t)k * 256);
        if (o == FRAME_BAD_SYNC) { status = 2; return; }
        if (o == FRAME_PASSES) { index = k; status = 0; return; }
    }
}

}  // namespace hcak
}  // namespace vga
