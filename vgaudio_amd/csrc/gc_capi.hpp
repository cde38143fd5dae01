// gc_capi.hpp -- what the GC-ADPCM C-ABI files share and that needs HIP types (capi_gcadpcm.hip, capi_gc_channels.hip,
// capi_gcadpcm_v.hip).  The arithmetic without HIP is in gc_host.hpp.
#pragma once
#include "common.hpp"
#include "host_batch.hpp"
#include "gcadpcm_kernels.hpp"
#include "gc_host.hpp"

#include <cstring>
#include <vector>

namespace vga {
namespace gc {

constexpr int GC_MIN_SHARE_CHANNELS = 128;   // channels per share when a call is spread over several GPUs (vga_set_devices): below this one GPU's pipeline is faster

// the device buffers of a host-pointer call
struct GcBatch {
    Stream st;
    DevBuf pcm, coefs, adpcm, h1, h2, ws, status;
    int64_t pcm_pitch = 0, adpcm_pitch = 0;
};

// the per-channel histories a caller handed in; async_on: the call's stream (the equal-length calls), null: synchronous
// copies (the ragged calls)
inline int upload_hist(DevBuf &d_h1, DevBuf &d_h2, int nch, const int16_t *h1, const int16_t *h2, const Stream *async_on)
{
    DevBuf *const dst[2] = {&d_h1, &d_h2};
    const int16_t *const src[2] = {h1, h2};
    for (int k = 0; k < 2; k++) {
        if (!src[k]) continue;
        VGA_HIP_TRY(dst[k]->alloc((size_t)nch * 2));
        if (async_on) VGA_HIP_TRY(hipMemcpyAsync(dst[k]->p, src[k], (size_t)nch * 2, hipMemcpyHostToDevice, async_on->s));
        else VGA_HIP_TRY(hipMemcpy(dst[k]->p, src[k], (size_t)nch * 2, hipMemcpyHostToDevice));
    }
    return VGA_OK;
}

// a decode job's status word as the call's error (run_status_job, host_batch.hpp)
constexpr const char *BAD_PREDICTOR = "a frame header names predictor > 7 (the reference throws IndexOutOfRangeException)";

// Shapes of one group of channels as the kernels index them: the rows' layout (gc_host.hpp) and the work plan, which asks
// the kernel files (coefficient records, five-wave channels, the encoder's pieces).
struct RaggedShape : RaggedLayout {
    std::vector<int64_t> rec_off;
    int solo_channels = 0, solo_usable = 0;   // gc::ragged_solo_count: the coefficient search's five-wave channels
    int64_t records = 0;                       // slots of the coefficient workspace (an empty channel owns one)
    // the encoder's plan (gc::plan_encode_pieces) and, for persistent workgroups, its items biggest first: the queue then
    // ends with the short ones (a channel's partial last piece, the pieces of short files) and little is left to wait for
    Pieces seg;
    int segments = 1;
    bool persistent = false;
    std::vector<uint32_t> items;

    void build(const int *lengths, int n, int64_t pcm_base, int64_t adpcm_base)
    {
        lay_out(lengths, n, pcm_base, adpcm_base);
        rec_off.resize(n);
        records = 0;
        for (int c = 0; c < n; c++) {
            rec_off[c] = records;
            records += coef_record_pitch(((int64_t)length[c] + 13) / 14);
        }
        items.clear();
        solo_channels = solo_usable = 0;
        if (n > 0 && !uniform && max_length > 0) {
            std::vector<int> by_length(n);
            for (int i = 0; i < n; i++) by_length[i] = length[order[i]];
            solo_channels = ragged_solo_count(by_length.data(), n, total_frames, device_cu_count(), &solo_usable);
            const int groups = (int)group_frames.size();
            const int64_t work = std::accumulate(group_frames.begin(), group_frames.end(), (int64_t)0);
            segments = plan_encode_pieces(groups, (max_length + 13) / 14, work, true, &persistent, &seg, encoder_plan_layout(groups, true));
            if (persistent && groups < (1 << 20) && segments <= 4096) {
                struct Item { int size, y, g; };
                std::vector<Item> list;
                for (int y = 0; y < segments; y++)
                    for (int g = 0; g < groups; g++)
                        if (seg.first(y) < group_frames[g])
                            list.push_back({(int)std::min<int64_t>(seg.frames(y), group_frames[g] - seg.first(y)), y, g});
                std::stable_sort(list.begin(), list.end(), [](const Item &a, const Item &b) { return a.size > b.size; });
                items.reserve(list.size());
                for (const Item &it : list) items.push_back(((uint32_t)it.y << 20) | (uint32_t)it.g);
            } else
                persistent = false;
        }
    }
    // bytes of the device image of the tables: order, length (int32), then pcm_off, adpcm_off, rec_off (int64)
    size_t table_bytes() const { return (size_t)round_up((int64_t)count * 8, 16) + (size_t)count * 24 + items.size() * 4; }
    void write_tables(unsigned char *host) const
    {
        int *o = reinterpret_cast<int *>(host);
        int *l = o + count;
        int64_t *p = reinterpret_cast<int64_t *>(host + round_up((int64_t)count * 8, 16));
        for (int c = 0; c < count; c++) {
            o[c] = order[c];
            l[c] = length[c];
            p[c] = pcm_off[c];
            p[count + c] = adpcm_off[c];
            p[2 * count + c] = rec_off[c];
        }
        if (!items.empty()) memcpy(p + 3 * (size_t)count, items.data(), items.size() * 4);
    }
    Ragged device_view(const unsigned char *dev) const
    {
        Ragged r;
        r.order = reinterpret_cast<const int *>(dev);
        r.length = r.order + count;
        r.pcm_off = reinterpret_cast<const int64_t *>(dev + round_up((int64_t)count * 8, 16));
        r.adpcm_off = r.pcm_off + count;
        r.rec_off = r.pcm_off + 2 * count;
        r.max_length = max_length;
        r.total_frames = total_frames;
        r.solo_channels = solo_channels;
        r.solo_usable = solo_usable;
        if (!items.empty()) {
            r.items = reinterpret_cast<const uint32_t *>(r.pcm_off + 3 * (size_t)count);
            r.n_items = (int)items.size();
            r.segments = segments;
            r.persistent = persistent ? 1 : 0;
            r.seg = seg;
        }
        return r;
    }
};

// the three launches on one group of channels, uniform groups through the equal-length kernels
inline int launch_coefs_group(const RaggedShape &sh, const Ragged &rg, const int16_t *d_pcm, int16_t *d_coefs, void *ws, hipStream_t s)
{
    if (sh.count <= 0) return VGA_OK;
    if (sh.uniform)
        return launch_coefs(d_pcm + sh.pcm_off[0], sh.pcm_pitch, sh.count, sh.length[0], d_coefs, ws, s);
    return launch_coefs(d_pcm, 0, sh.count, 0, d_coefs, ws, s, &rg);
}
inline int launch_encode_group(const RaggedShape &sh, const Ragged &rg, const int16_t *d_pcm, const int16_t *d_coefs, const int16_t *h1,
                               const int16_t *h2, uint8_t *d_adpcm, hipStream_t s, void *scratch, size_t scratch_bytes)
{
    if (sh.count <= 0) return VGA_OK;
    if (sh.uniform)
        return launch_encode(d_pcm + sh.pcm_off[0], sh.pcm_pitch, sh.count, sh.length[0], d_coefs, h1, h2, d_adpcm + sh.adpcm_off[0],
                             sh.adpcm_pitch, s, scratch, scratch_bytes);
    return launch_encode(d_pcm, 0, sh.count, 0, d_coefs, h1, h2, d_adpcm, 0, s, scratch, scratch_bytes, &rg);
}
inline int launch_decode_group(const RaggedShape &sh, const Ragged &rg, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *h1,
                               const int16_t *h2, int16_t *d_pcm, int *d_status, hipStream_t s)
{
    if (sh.count <= 0) return VGA_OK;
    if (sh.uniform)
        return launch_decode(d_adpcm + sh.adpcm_off[0], sh.adpcm_pitch, d_coefs, sh.count, sh.length[0], h1, h2, d_pcm + sh.pcm_off[0],
                             sh.pcm_pitch, d_status, s);
    return launch_decode(d_adpcm, 0, d_coefs, sh.count, 0, h1, h2, d_pcm, 0, d_status, s, &rg);
}

}  // namespace gc
}  // namespace vga
