// adx_keyed_files_kernels.hip -- the kernels of include/vgaudio_hip_files/adx_keyed_files.h: CRI ADX encryption
// (CriAdxEncryption.cs:16-94) for a SET of files, every kernel one launch over the tables the set's object holds.
//
//   adx_keyed_interleave_span_kernel, adx_keyed_deinterleave_span_kernel
//                                  adx_span.hpp's bodies with a cipher between their load and store phase: one thread per
//                                  frame held in LDS tests emptiness there and XORs the two scale bytes.  Every byte crosses
//                                  HBM once each way, as in the unkeyed kernels
//   adx_keyed_cipher_kernel        files in the general form: a pass over the call's output (image frames / rows), (file,
//                                  chunk of 2048 slots) items, one thread per slot
//   adx_keyed_status_kernel        d_status, one thread per file
//   adx_find_init_kernel, adx_find_scan_kernel, adx_find_resolve_kernel
//                                  the key search: a "still possible" bit per (file, candidate); (file, span of 1024 slots)
//                                  workgroups read the span's scales into LDS once and walk the LCG of every candidate still
//                                  possible along them, 64 candidates x 4 quarters of the span per pass; lowest surviving bit
// A thread jumps the LCG once to its first slot (adx_lcg.hpp) and then steps: by 256 slots in the cipher kernels, by one in
// the scan.  Everything else of a keyed call is adx_files_kernels.hip's (headers, general copy, footers, histories).
#include "common.hpp"
#include "adx_keyed_files_kernels.hpp"
#include "adx_lcg.hpp"

namespace vga {
namespace adxk {

using adxf::FileTab;
using adxf::Item;
using adxlcg::Affine;
using adxlcg::apply;
using adxlcg::lcg_power;

// the key of one file: on == false -> the file is moved unkeyed
struct FileKey { unsigned seed, mult, inc; int type; bool on; };

__device__ __forceinline__ FileKey key_of(const Keys &k, int file, int type)
{
    const int i = k.index ? k.index[file] : 0;
    FileKey r{0u, 0u, 0u, type, i >= 0 && i < k.nkeys};
    if (r.on) { r.seed = (unsigned)k.keys[i].seed; r.mult = (unsigned)k.keys[i].mult; r.inc = (unsigned)k.keys[i].inc; }
    return r;
}

// EncryptDecryptChannel's two bytes of a non-empty frame (:28-35).  x: the state at this slot from the masked seed; slot 0
// uses the caller's seed bits as they are (the reference's int before its first step)
__device__ __forceinline__ void cipher_frame(const FileKey &k, int64_t slot, unsigned x, uint8_t *f)
{
    const unsigned xr = slot == 0 ? k.seed : x;
    uint8_t b0 = (uint8_t)(f[0] ^ ((xr >> 8) & 0xffu));
    if (k.type == 9) b0 &= 0x1f;
    f[0] = b0;
    f[1] = (uint8_t)(f[1] ^ (xr & 0xffu));
}

// FrameNotEmpty (:96-107) of an 18-byte frame in LDS at any byte: the aligned words that cover it, the edges masked off
// (at most three bytes behind the frame are read: inside the span's LDS array, which ends in 32 bytes of slack)
__device__ __forceinline__ bool frame_not_empty(const uint8_t *f)
{
    const unsigned a = (unsigned)((uintptr_t)f & 3u);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(f - a);
    const unsigned e = a + adxspan::kFrame;                            // the frame is bytes [a, e) of the words, e = 18 .. 21
    uint32_t any = (w[0] >> (8 * a)) | w[1] | w[2] | w[3];
    any |= e >= 20 ? w[4] : w[4] & ((1u << (8 * (e - 16))) - 1u);
    if (e > 20) any |= w[5] & 0xffu;
    return any != 0;
}

// between the phases of a span body: the frames lie in LDS, slot k0 * nch + j is local frame j in image order
struct SpanCipher {
    static constexpr bool active = true;
    FileKey k;
    template <class FrameAt> __device__ __forceinline__ void operator()(int nch, int k0, int nk, FrameAt frame_at) const
    {
        const int n = nk * nch, t = (int)threadIdx.x;
        if (!k.on || t >= n) return;
        // The jump to the span's first slot and the stride are the same for the whole workgroup (scalar work); a thread
        // adds its own at most 255 steps: eight rounds of square-and-multiply instead of thirty.
        const int64_t s0 = (int64_t)k0 * nch;
        const Affine base = lcg_power(k.mult, k.inc, (uint64_t)s0), stride = lcg_power(k.mult, k.inc, adxspan::kThreads);
        unsigned x = apply(adxlcg::then(base, lcg_power(k.mult, k.inc, (uint64_t)t)), k.seed & adxlcg::kMask);
        for (int j = t; j < n; j += adxspan::kThreads) {
            const int fr = j / nch, c = j - fr * nch;
            uint8_t *f = frame_at(fr, c);
            if (frame_not_empty(f)) cipher_frame(k, s0 + j, x, f);
            x = apply(stride, x);
        }
    }
};

__global__ __launch_bounds__(256) void adx_keyed_interleave_span_kernel(const FileTab *__restrict__ tab, const int64_t *__restrict__ row_off,
                                                                        const Item *__restrict__ items, const uint8_t *__restrict__ audio,
                                                                        uint8_t *__restrict__ images, Keys keys)
{
    __shared__ __align__(16) uint8_t lds[adxspan::kLdsBytes];
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[it.x];
    const int64_t *rows = row_off + t.first_channel;
    adxspan::interleave_span(lds, [&](int c) { return audio + rows[c]; }, t.h.nch, t.copy_frames, (int)it.y, t.span_frames,
                             images + t.image_off + t.audio_offset, SpanCipher{key_of(keys, it.x, t.h.encryption_type)});
}

__global__ __launch_bounds__(256) void adx_keyed_deinterleave_span_kernel(const FileTab *__restrict__ tab, const int64_t *__restrict__ row_off,
                                                                          const Item *__restrict__ items, const uint8_t *__restrict__ images,
                                                                          uint8_t *__restrict__ audio, Keys keys)
{
    __shared__ __align__(16) uint8_t lds[adxspan::kLdsBytes];
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[it.x];
    const int64_t *rows = row_off + t.first_channel;
    adxspan::deinterleave_span(lds, images + t.image_off + t.audio_offset, t.h.nch, t.copy_frames, (int)it.y, t.span_frames,
                               [&](int c) { return audio + rows[c]; }, SpanCipher{key_of(keys, it.x, t.h.encryption_type)});
}

// The general form's cipher pass, in place over what the copy kernels left.  Read == false: the frames of the image, where
// slot order is image order; Read == true: the rows.
template <bool Read>
__global__ __launch_bounds__(256) void adx_keyed_cipher_kernel(const FileTab *__restrict__ tab, const int64_t *__restrict__ row_off,
                                                               const Item *__restrict__ items, uint8_t *__restrict__ data, Keys keys)
{
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[it.x];
    const FileKey k = key_of(keys, it.x, t.h.encryption_type);
    if (!k.on) return;
    const int nch = t.h.nch, fs = t.h.frame_size;
    const int64_t slots = (int64_t)t.copy_frames * nch;
    int64_t s = (int64_t)it.y * adxf::CIPHER_CHUNK_SLOTS + threadIdx.x;
    if (s >= slots) return;
    unsigned x = apply(lcg_power(k.mult, k.inc, (uint64_t)s), k.seed & adxlcg::kMask);
    const Affine stride = lcg_power(k.mult, k.inc, 256);
    for (int q = 0; q < adxf::CIPHER_CHUNK_SLOTS / 256 && s < slots; q++, s += 256) {
        uint8_t *f;
        if (Read) {
            const int64_t fr = s / nch;
            const int c = (int)(s - fr * nch);
            f = data + row_off[t.first_channel + c] + fr * fs;
        } else {
            f = data + t.image_off + t.audio_offset + s * fs;
        }
        unsigned any = 0;
        for (int b = 0; b < fs; b++) any |= f[b];
        if (any) cipher_frame(k, s, x, f);
        x = apply(stride, x);
    }
}

__global__ __launch_bounds__(256) void adx_keyed_status_kernel(int files, Keys keys, int *__restrict__ status)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < files) status[f] = (keys.index ? keys.index[f] : 0) >= keys.nkeys ? 1 : 0;
}

// ---------------------------------------------------------------- the key search
// candidates of a file: [lo, hi) of d_keys by its revision (CriAdxEncryption.cs:46; revision 0: none, AdxReader.cs:128)
struct Sublist { int lo, hi; };
__device__ __forceinline__ Sublist sublist_of(int revision, int nkeys8, int nkeys9)
{
    if (revision == 0) return {0, 0};
    return revision == 8 ? Sublist{0, nkeys8} : Sublist{nkeys8, nkeys8 + nkeys9};
}
// the bits of [lo, hi) that lie in word w
__device__ __forceinline__ uint32_t word_mask(int w, int lo, int hi)
{
    const int a = max(lo - 32 * w, 0), b = min(hi - 32 * w, 32);
    if (a >= b) return 0u;
    const uint32_t upto_b = b == 32 ? 0xFFFFFFFFu : (1u << b) - 1u;
    return upto_b & ~((1u << a) - 1u);
}

__global__ __launch_bounds__(256) void adx_find_init_kernel(const FileTab *__restrict__ tab, int files, int words, int nkeys8, int nkeys9,
                                                            uint32_t *__restrict__ bits)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)files * words) return;
    const int f = (int)(i / words), w = (int)(i - (int64_t)f * words);
    const Sublist s = sublist_of(tab[f].h.encryption_type, nkeys8, nkeys9);
    bits[i] = word_mask(w, s.lo, s.hi);
}

constexpr int kFindQuarter = adxf::FIND_SPAN_SLOTS / 4;
// scale j of the span in LDS: each quarter starts one bank further, so the four quarters of a pass read four banks
__device__ __forceinline__ int scale_at(int j) { return j + 2 * (j / kFindQuarter); }

// GetScales + TestKey (:59-94) over one span of one file
__global__ __launch_bounds__(256) void adx_find_scan_kernel(const FileTab *__restrict__ tab, const Item *__restrict__ items,
                                                            const uint8_t *__restrict__ images, const vga_adx_key *__restrict__ keys,
                                                            int words, int nkeys8, int nkeys9, uint32_t *bits)
{
    __shared__ uint16_t scales[adxf::FIND_SPAN_SLOTS + 8];
    __shared__ uint32_t dead[2];
    const Item it = items[blockIdx.x];
    const FileTab &t = tab[it.x];
    const int revision = t.h.encryption_type;
    const Sublist sub = sublist_of(revision, nkeys8, nkeys9);
    if (sub.lo >= sub.hi) return;
    const int fs = t.h.frame_size;
    const int64_t slots = (int64_t)t.copy_frames * t.h.nch, first = (int64_t)it.y * adxf::FIND_SPAN_SLOTS;
    const int count = (int)min((int64_t)adxf::FIND_SPAN_SLOTS, slots - first);
    const uint8_t *base = images + t.image_off + t.audio_offset + first * fs;
    for (int j = threadIdx.x; j < count; j += 256) {
        const uint8_t *f = base + (int64_t)j * fs;
        scales[scale_at(j)] = (uint16_t)(((unsigned)f[0] << 8) | f[1]);
    }
    __syncthreads();
    const unsigned mask = revision == 8 ? 0xE000u : 0x1000u;
    const int q0 = (int)(threadIdx.x & 3) * kFindQuarter, q1 = min(q0 + kFindQuarter, count);
    uint32_t *mine = bits + (int64_t)it.x * words;
    // 64 candidates a pass, the passes on multiples of 64 so that a pass is two whole words of the file's bits.  What a pass
    // finds out is gathered in LDS and leaves the workgroup as at most two atomics: every workgroup of a file meets the same
    // wrong candidates, and one atomic per lane would queue them all on the same few words.
    for (int cb = sub.lo & ~63; cb < sub.hi; cb += 64) {
        if (threadIdx.x < 2) dead[threadIdx.x] = 0u;
        __syncthreads();
        const int cand = cb + (int)(threadIdx.x >> 2);
        if (cand >= sub.lo && cand < sub.hi && q0 < count) {
            // a stale word only costs work: bits are only ever cleared, and the answer is read in the next launch
            const uint32_t word = __hip_atomic_load(&mine[cand >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((word >> (cand & 31)) & 1u) {
                const unsigned seed = (unsigned)keys[cand].seed, mult = (unsigned)keys[cand].mult & adxlcg::kMask, inc = (unsigned)keys[cand].inc & adxlcg::kMask;
                unsigned x = apply(lcg_power(mult, inc, (uint64_t)(first + q0)), seed & adxlcg::kMask);
                bool bad = false;
                for (int j = q0; j < q1; j++) {
                    const unsigned scale = scales[scale_at(j)];
                    const unsigned xr = first + j == 0 ? seed : x;     // the first comparison uses the raw seed
                    if (((scale ^ xr) & mask) != 0 && scale != 0) { bad = true; break; }
                    x = (x * mult + inc) & adxlcg::kMask;
                }
                if (bad) atomicOr(&dead[(cand - cb) >> 5], 1u << (cand & 31));
            }
        }
        __syncthreads();
        if (threadIdx.x < 2 && dead[threadIdx.x]) {
            uint32_t *word = &mine[(cb >> 5) + (int)threadIdx.x];
            if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & dead[threadIdx.x]) atomicAnd(word, ~dead[threadIdx.x]);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void adx_find_resolve_kernel(const FileTab *__restrict__ tab, int files, int words, int nkeys8, int nkeys9,
                                                               const uint32_t *__restrict__ bits, int *__restrict__ index_out)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= files) return;
    const Sublist s = sublist_of(tab[f].h.encryption_type, nkeys8, nkeys9);
    int found = -1;
    for (int w = s.lo >> 5; found < 0 && s.lo < s.hi && w <= (s.hi - 1) >> 5; w++) {
        const uint32_t live = bits[(int64_t)f * words + w] & word_mask(w, s.lo, s.hi);
        if (live) found = 32 * w + __ffs((int)live) - 1;
    }
    index_out[f] = found;
}

// ---------------------------------------------------------------- launchers
namespace {

int launch_status(const adxf::DeviceTables &t, Keys keys, int *d_status, hipStream_t stream)
{
    if (!d_status) return VGA_OK;
    hipLaunchKernelGGL(adx_keyed_status_kernel, dim3((t.files + 255) / 256), dim3(256), 0, stream, t.files, keys, d_status);
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

}  // namespace

int launch_write_keyed(const adxf::DeviceTables &t, bool general, const uint8_t *d_audio, const int16_t *d_history, Keys keys,
                       uint8_t *d_images, int *d_status, hipStream_t stream)
{
    if (t.files <= 0) return VGA_OK;
    const int k = general ? 1 : 0, span = general ? 0 : t.span_items;
    if (int rc = adxf::launch_write_headers(t, d_history, d_images, stream)) return rc;
    if (span > 0) {
        hipLaunchKernelGGL(adx_keyed_interleave_span_kernel, dim3(span), dim3(256), 0, stream, t.tab, t.row_off, t.items[k], d_audio, d_images, keys);
        VGA_HIP_TRY(hipGetLastError());
    }
    if (int rc = adxf::launch_write_general(t, general, d_audio, d_images, stream)) return rc;
    if (t.cipher_count[k] > 0) {
        hipLaunchKernelGGL(adx_keyed_cipher_kernel<false>, dim3(t.cipher_count[k]), dim3(256), 0, stream, t.tab, t.row_off, t.cipher_items[k],
                           d_images, keys);
        VGA_HIP_TRY(hipGetLastError());
    }
    if (int rc = adxf::launch_write_footers(t, d_images, stream)) return rc;
    return launch_status(t, keys, d_status, stream);
}

int launch_read_keyed(const adxf::DeviceTables &t, bool general, const uint8_t *d_images, Keys keys, uint8_t *d_audio,
                      int16_t *d_history_out, int *d_status, hipStream_t stream)
{
    if (t.files <= 0) return VGA_OK;
    const int k = general ? 1 : 0, span = general ? 0 : t.span_items;
    if (t.channels > 0) {
        if (int rc = adxf::launch_read_history(t, d_history_out, stream)) return rc;
        if (span > 0) {
            hipLaunchKernelGGL(adx_keyed_deinterleave_span_kernel, dim3(span), dim3(256), 0, stream, t.tab, t.row_off, t.items[k], d_images, d_audio,
                               keys);
            VGA_HIP_TRY(hipGetLastError());
        }
        if (int rc = adxf::launch_read_general(t, general, d_images, d_audio, stream)) return rc;
        if (t.cipher_count[k] > 0) {
            hipLaunchKernelGGL(adx_keyed_cipher_kernel<true>, dim3(t.cipher_count[k]), dim3(256), 0, stream, t.tab, t.row_off, t.cipher_items[k],
                               d_audio, keys);
            VGA_HIP_TRY(hipGetLastError());
        }
    }
    return launch_status(t, keys, d_status, stream);
}

int launch_find_keys(const adxf::DeviceTables &t, const uint8_t *d_images, const vga_adx_key *d_keys, int nkeys8, int nkeys9,
                     int *d_key_index_out, uint32_t *d_bits, hipStream_t stream)
{
    if (t.files <= 0) return VGA_OK;
    const int words = (int)find_words_per_file(nkeys8, nkeys9);
    const int64_t total = (int64_t)t.files * words;
    if (total > 0) {
        hipLaunchKernelGGL(adx_find_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, t.tab, t.files, words, nkeys8, nkeys9,
                           d_bits);
        VGA_HIP_TRY(hipGetLastError());
        if (t.find_count > 0) {
            hipLaunchKernelGGL(adx_find_scan_kernel, dim3(t.find_count), dim3(256), 0, stream, t.tab, t.find_items, d_images, d_keys, words, nkeys8,
                               nkeys9, d_bits);
            VGA_HIP_TRY(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(adx_find_resolve_kernel, dim3((t.files + 255) / 256), dim3(256), 0, stream, t.tab, t.files, words, nkeys8, nkeys9, d_bits,
                       d_key_index_out);
    VGA_HIP_TRY(hipGetLastError());
    return VGA_OK;
}

}  // namespace adxk
}  // namespace vga
