// hca_keyed_files_kernels.hip -- the key search of include/vgaudio_hip_files/hca_keyed_files.h: CriHcaEncryption.FindKey
// (CriHcaEncryption.cs:34-88) for every type-56 file of a set, four launches whatever the numbers of files and candidates.
//
//   hcak_first_frame_kernel  a wave per file walks the file's frames in order and stops at the first that holds a non-zero
//                            byte in [2, frame_size - 2) (FindFirstNonEmptyFrame): first tested frame and number of tested
//                            frames into the workspace.  Only the frames in front of it are read.
//   hcak_test_kernel<true>   a wave per (file, 64 candidates): the file's first tested frame and the 64 tables are staged in
//                            LDS once, lane = candidate walks the frame (hca_keyed_walk.hpp), one outcome byte per
//                            (file, candidate) into the workspace.  Wrong keys mostly end here.
//   hcak_test_kernel<false>  the same items; an item without a candidate that passed the first frame returns at once.
//                            Otherwise lane = (surviving candidate, later frame) pair, dense over the pairs; per candidate the
//                            lowest failing frame and the lowest frame with a wrong sync word are taken with LDS atomicMin
//                            (order-free) and the candidate's outcome byte is rewritten by its own lane.
//   hcak_resolve_kernel      a wave per file puts the outcomes back in candidate order: the lowest candidate that is not
//                            "fails" decides -- passes: its index; wrong sync word: -1, status 2; none: -1, status 1.
// Every (file, candidate) outcome has its own byte and every byte is written before it is read by a later launch: the result
// does not depend on scheduling, nor on what the workspace held.
//
// LDS of a test workgroup (dynamic): 64 tables at a stride of 260 bytes (16 640; 65 dwords, so lanes that look up the same
// byte value hit 64 different banks), the staged frame bytes, and the resolutions of the frame a lane walks, 4 bits each, 64
// bytes per channel and lane, lane-interleaved by dword (the band index is uniform over the wave: no conflict).
#include "common.hpp"
#include "hca_device.hpp"
#include "hca_keyed_files_kernels.hpp"

namespace vga {
namespace hcak {

namespace {

constexpr int kTablesBytes = KEY_BLOCK * TABLE_STRIDE;

// a frame's decrypted bytes: the stored byte out of LDS or global memory, through the lane's table in LDS
struct DeviceBytes {
    const uint8_t *frame;                        // LDS or global
    const uint8_t *sub;                          // LDS
    __device__ __forceinline__ unsigned plain(int i) const { return sub[frame[i]]; }
};
// the lane's resolutions: word (c, w) at dword (c * 16 + w) * 64 + lane
struct DeviceRes {
    uint32_t *base;                              // LDS, + lane
    __device__ __forceinline__ void put(int c, int w, uint32_t v) { base[(c * 16 + w) * 64] = v; }
    __device__ __forceinline__ uint32_t word(int c, int w) const { return base[(c * 16 + w) * 64]; }
};

__device__ __forceinline__ void load_walk_tables(WalkTables &T, int lane)
{
    for (int i = lane; i < 128; i += 64) (&T.dec_bits[0][0])[i] = (&HCA_QuantizedSpectrumBits[0][0])[i];
    if (lane < 16) T.max_bits[lane] = HCA_QuantizedSpectrumMaxBits[lane];
    T.res_curve[lane] = lane < 59 ? HCA_ScaleToResolutionCurve[lane] : 0;
}

// `rows` tables of 256 bytes from global memory (any byte) to LDS at TABLE_STRIDE
__device__ __forceinline__ void stage_tables(uint8_t *lds, const uint8_t *tables, int rows, int lane)
{
    if (((uintptr_t)tables & 3) == 0) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(tables);
        uint32_t *dst = reinterpret_cast<uint32_t *>(lds);
        for (int i = lane; i < rows * 64; i += 64) dst[(i >> 6) * (TABLE_STRIDE / 4) + (i & 63)] = src[i];
    } else {
        for (int i = lane; i < rows * 256; i += 64) lds[(i >> 8) * TABLE_STRIDE + (i & 255)] = tables[i];
    }
}

// `bytes` bytes at `src` (any byte) into LDS with aligned dword loads: byte i lands at lds[lead + i], the returned lead is
// 0..3.  The first and the last dword may hold up to three bytes outside the range; an aligned dword that holds one byte of
// the image lies in the image's page.
__device__ __forceinline__ int stage_bytes(uint8_t *lds, const uint8_t *src, int bytes, int lane)
{
    const int lead = (int)((uintptr_t)src & 3);
    const uint32_t *s4 = reinterpret_cast<const uint32_t *>(src - lead);
    uint32_t *d4 = reinterpret_cast<uint32_t *>(lds);
    const int words = (lead + bytes + 3) >> 2;
    for (int i = lane; i < words; i += 64) d4[i] = s4[i];
    return lead;
}

}  // namespace

__global__ __launch_bounds__(64) void hcak_first_frame_kernel(const WalkFile *__restrict__ walk, const uint8_t *__restrict__ images,
                                                              int *__restrict__ first_out, int *__restrict__ ntest_out)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const WalkFile &w = walk[f];
    int first = 0, ntest = 0;
    if (w.encryption_type == 56 && w.usable) {
        const int fs = w.frame_size, fc = w.frame_count;
        const uint8_t *frames = images + w.frames_off;
        for (int j = 0; j < fc; j++) {
            bool any = false;
            const uint8_t *a = frames + (int64_t)j * fs;
            for (int i = 2 + lane; i < fs - 2; i += 64) any |= a[i] != 0;
            if (__any(any)) {
                first = j;
                break;
            }
        }
        ntest = min(FRAMES_TO_TEST, fc - first);
    }
    if (lane == 0) {
        first_out[f] = first;
        ntest_out[f] = ntest;
    }
}

template <bool FIRST>
__global__ __launch_bounds__(64) void hcak_test_kernel(const WalkFile *__restrict__ walk, const int *__restrict__ find_files, int key_blocks,
                                                       const uint8_t *__restrict__ images, const uint8_t *__restrict__ tables, int nkeys,
                                                       const int *__restrict__ first_in, const int *__restrict__ ntest_in,
                                                       uint8_t *__restrict__ outcome, int stage_room)
{
    extern __shared__ __align__(16) uint8_t lds[];
    __shared__ WalkTables T;
    __shared__ WalkFile w;
    __shared__ int s_fail[KEY_BLOCK], s_bad[KEY_BLOCK];
    const int lane = threadIdx.x;
    const int f = find_files[blockIdx.x / key_blocks], k0 = (int)(blockIdx.x % key_blocks) * KEY_BLOCK;
    const int rows = min(KEY_BLOCK, nkeys - k0);
    const int ntest = ntest_in[f];
    if (ntest <= (FIRST ? 0 : 1)) return;                              // no frame (left) to test: uniform
    uint8_t *mine = outcome + (int64_t)f * nkeys + k0 + lane;
    uint64_t survivors = 0;
    if (!FIRST) {
        survivors = __ballot(lane < rows && *mine == FRAME_PASSES);
        if (survivors == 0) return;                                    // uniform: one wave
    }
    for (int i = lane; i < (int)(sizeof(WalkFile) / 4); i += 64) reinterpret_cast<uint32_t *>(&w)[i] = reinterpret_cast<const uint32_t *>(walk + f)[i];
    load_walk_tables(T, lane);
    s_fail[lane] = FRAMES_TO_TEST;
    s_bad[lane] = FRAMES_TO_TEST;
    __syncthreads();

    uint8_t *lds_tables = lds, *lds_frames = lds + kTablesBytes;
    const int fs = w.frame_size;
    const int first = first_in[f] + (FIRST ? 0 : 1), nframes = FIRST ? 1 : ntest - 1;
    const uint8_t *frames = images + w.frames_off + (int64_t)first * fs;
    const bool staged = FIRST ? fs <= STAGE_MAX_FRAME : nframes * fs <= STAGE_REST_BYTES;
    const int room = staged ? ((nframes * fs + 7) & ~3) : 0;            // lead and overhang included
    uint32_t *res = reinterpret_cast<uint32_t *>(lds_frames + stage_room) + lane;
    stage_tables(lds_tables, tables + (size_t)k0 * 256, rows, lane);
    int lead = 0;
    if (staged && room <= stage_room) lead = stage_bytes(lds_frames, frames, nframes * fs, lane);
    const bool in_lds = staged && room <= stage_room;
    __syncthreads();
    const uint8_t *base = in_lds ? lds_frames + lead : frames;

    if (FIRST) {
        if (lane < rows) {
            DeviceBytes b = {base, lds_tables + lane * TABLE_STRIDE};
            DeviceRes r = {res};
            *mine = (uint8_t)walk_frame(w, T, b, r);
        }
    } else {
        const int nsurv = __popcll(survivors), pairs = nsurv * nframes;
        for (int p = lane; p < pairs; p += 64) {
            int s = p / nframes, cand = 0;
            const int j = p % nframes;
            for (; cand < 64; cand++)                                   // the s-th surviving candidate of the item
                if ((survivors >> cand) & 1) {
                    if (s == 0) break;
                    s--;
                }
            DeviceBytes b = {base + (int64_t)j * fs, lds_tables + cand * TABLE_STRIDE};
            DeviceRes r = {res};
            const int v = walk_frame(w, T, b, r);
            if (v == FRAME_FAILS) atomicMin(&s_fail[cand], j);
            if (v == FRAME_BAD_SYNC) atomicMin(&s_bad[cand], j);
        }
        __syncthreads();
        if ((survivors >> lane) & 1) *mine = (uint8_t)candidate_outcome(s_fail[lane], s_bad[lane], FRAMES_TO_TEST);
    }
}

__global__ __launch_bounds__(64) void hcak_resolve_kernel(const WalkFile *__restrict__ walk, int nkeys, int type1_index,
                                                          const int *__restrict__ ntest_in, const uint8_t *__restrict__ outcome,
                                                          int *__restrict__ index_out, int *__restrict__ status_out)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const WalkFile &w = walk[f];
    int index = -1, status = 0;
    if (w.encryption_type == 1) index = type1_index;
    if (w.encryption_type == 56) {
        status = 1;
        if (nkeys > 0 && w.frame_count == 0) {                         // no frame to refute the first key
            index = 0;
            status = 0;
        } else if (nkeys > 0 && ntest_in[f] > 0) {
            const uint8_t *o = outcome + (int64_t)f * nkeys;
            for (int k0 = 0; k0 < nkeys; k0 += 64) {
                const int mine = k0 + lane < nkeys ? o[k0 + lane] : FRAME_FAILS;
                const uint64_t decided = __ballot(mine != FRAME_FAILS);
                if (decided) {
                    const int l = __ffsll((unsigned long long)decided) - 1;
                    if (__shfl(mine, l) == FRAME_PASSES) {
                        index = k0 + l;
                        status = 0;
                    } else status = 2;
                    break;
                }
            }
        }
    }
    if (lane == 0) {
        index_out[f] = index;
        if (status_out) status_out[f] = status;
    }
}

__global__ __launch_bounds__(256) void hcak_read_status_kernel(const int *__restrict__ index, int ntables, int nfiles, int *__restrict__ status)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < nfiles) status[f] = index && index[f] >= ntables ? 1 : 0;
}

// ---------------------------------------------------------------- launchers
int launch_find_keys(const hcaf::DeviceTables &t, const uint8_t *d_images, const uint8_t *d_tables, int nkeys, int type1_index,
                     int *d_key_index_out, int *d_status, void *d_workspace, hipStream_t stream)
{
    if (t.files <= 0) return VGA_OK;
    int *first = static_cast<int *>(d_workspace), *ntest = first + t.files;
    uint8_t *outcome = reinterpret_cast<uint8_t *>(ntest + t.files);
    hipLaunchKernelGGL(hcak_first_frame_kernel, dim3(t.files), dim3(64), 0, stream, t.walk, d_images, first, ntest);
    VGA_HIP_TRY(hipGetLastError());
    const int key_blocks = (nkeys + KEY_BLOCK - 1) / KEY_BLOCK;
    const int64_t items = (int64_t)t.find_file_count * key_blocks;
    if (items > 0) {
        const size_t res_bytes = (size_t)t.find_max_channels * 64 * 64;
        const size_t lds_first = kTablesBytes + (STAGE_MAX_FRAME + 8) + res_bytes, lds_rest = kTablesBytes + (STAGE_REST_BYTES + 8) + res_bytes;
        hipLaunchKernelGGL(hcak_test_kernel<true>, dim3((unsigned)items), dim3(64), lds_first, stream, t.walk, t.find_files, key_blocks, d_images,
                           d_tables, nkeys, first, ntest, outcome, STAGE_MAX_FRAME + 8);
        VGA_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(hcak_test_kernel<false>, dim3((unsigned)items), dim3(64), lds_rest, stream, t.walk, t.find_files, key_blocks, d_images,
                           d_tables, nkeys, first, ntest, outcome, STAGE_REST_BYTES + 8);
        VGA_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(hcak_resolve_kernel, dim3(t.files), dim3(64), 0, stream, t.walk, nkeys, type1_index, ntest, outcome, d_key_index_out, d_status);
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

int launch_read_keyed(const hcaf::DeviceTables &t, bool general, const uint8_t *d_images, const uint8_t *d_tables, int ntables,
                      const int *d_key_index, uint8_t *d_frames, int *d_bad_crc, int *d_status, hipStream_t stream)
{
    if (t.files <= 0) return VGA_OK;
    hcaf::KeySource keys;
    keys.tables = d_tables;
    keys.index = d_key_index;
    keys.ntables = ntables;
    keys.external = 1;
    if (int rc = hcaf::launch_read_images(t, general, d_images, d_frames, d_bad_crc, stream, keys)) return rc;
    if (d_status) {
        hipLaunchKernelGGL(hcak_read_status_kernel, dim3((t.files + 255) / 256), dim3(256), 0, stream, d_key_index, ntables, t.files, d_status);
        VGA_HIP_TRY(hipGetLastError());
    }
    return VGA_OK;
}

}  // namespace hcak
}  // namespace vga
