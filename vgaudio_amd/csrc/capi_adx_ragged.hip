// capi_adx_ragged.hip -- device-resident CRI ADX batches of channels of different lengths (include/vgaudio_hip/adx_ragged.h).
// Host side only: the layout and the plan come from adx_host.hpp; create uploads the tables the ragged kernels read
// (adx_kernels.hpp: AdxRaggedTables, AdxRaggedItems), a call checks its pointers and launches.
#include "common.hpp"
#include "adx_kernels.hpp"
#include "adx_host.hpp"

#include <cstdlib>
#include <vector>

using namespace vga;

struct vga_adx_ragged {
    adx::RaggedLayout L;
    adx::RaggedPlan enc, dec;
    adx::AdxDeviceParams enc_params = {}, dec_params = {};
    bool enc_pieces = false, dec_pieces = false;       // the time-piece kernels (else the general lane-per-channel kernel)
    int device = 0, cus = 256;
    void *d_tables = nullptr;
    adx::AdxRaggedTables tables = {};
    adx::AdxRaggedItems enc_items = {}, dec_items = {};
    ~vga_adx_ragged()
    {
        if (d_tables) (void)hipFree(d_tables);
    }
};

namespace {

int upload_tables(vga_adx_ragged &r)
{
    const adx::RaggedLayout &L = r.L;
    if (L.count <= 0) return VGA_OK;
    const int slots = L.slots(), groups = L.groups();
    // one block: [slots] pcm_off, adx_off (int64), [groups] crumb_base (int64), [slots] length, channel (int), the two item tables
    const size_t off_at = 0, adx_at = off_at + (size_t)slots * 8, crumb_at = adx_at + (size_t)slots * 8;
    const size_t len_at = crumb_at + (size_t)groups * 8, ch_at = len_at + (size_t)slots * 4;
    const size_t enc_at = ch_at + (size_t)slots * 4, dec_at = enc_at + r.enc.items.size() * 4;
    const size_t bytes = dec_at + r.dec.items.size() * 4;
    std::vector<unsigned char> host(bytes, 0);
    int64_t *pcm_off = reinterpret_cast<int64_t *>(host.data() + off_at), *adx_off = reinterpret_cast<int64_t *>(host.data() + adx_at);
    int *length = reinterpret_cast<int *>(host.data() + len_at), *channel = reinterpret_cast<int *>(host.data() + ch_at);
    for (int s = 0; s < slots; s++) {
        const int c = s < L.count ? L.order[s] : -1;
        pcm_off[s] = c >= 0 ? L.pcm_off[c] : 0;
        adx_off[s] = c >= 0 ? L.adx_off[c] : 0;
        length[s] = c >= 0 ? L.length[c] : 0;
        channel[s] = c;
    }
    memcpy(host.data() + crumb_at, L.crumb_base.data(), (size_t)groups * 8);
    if (!r.enc.items.empty()) memcpy(host.data() + enc_at, r.enc.items.data(), r.enc.items.size() * 4);
    if (!r.dec.items.empty()) memcpy(host.data() + dec_at, r.dec.items.data(), r.dec.items.size() * 4);
    VGA_HIP_TRY(device_malloc(&r.d_tables, bytes));
    VGA_HIP_TRY(hipMemcpy(r.d_tables, host.data(), bytes, hipMemcpyHostToDevice));
    const unsigned char *d = static_cast<const unsigned char *>(r.d_tables);
    r.tables.pcm_off = reinterpret_cast<const int64_t *>(d + off_at);
    r.tables.adx_off = reinterpret_cast<const int64_t *>(d + adx_at);
    r.tables.crumb_base = reinterpret_cast<const int64_t *>(d + crumb_at);
    r.tables.length = reinterpret_cast<const int *>(d + len_at);
    r.tables.channel = reinterpret_cast<const int *>(d + ch_at);
    r.tables.slots = slots;
    r.tables.nch = L.count;
    r.enc_items = {reinterpret_cast<const int2 *>(d + enc_at), r.enc.item_count(), r.enc.pieces.segments, r.enc.pieces.seg_frames};
    r.dec_items = {reinterpret_cast<const int2 *>(d + dec_at), r.dec.item_count(), r.dec.pieces.segments, r.dec.pieces.seg_frames};
    return VGA_OK;
}

int check_object(const vga_adx_ragged *r, const char *what)
{
    if (!r) { set_error("%s: null vga_adx_ragged", what); return VGA_ERR_ARGUMENT; }
    int device = -1;
    (void)hipGetDevice(&device);
    if (r->L.count > 0 && device != r->device) {
        set_error("%s: the ragged batch was created on device %d, the current one is %d", what, r->device, device);
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}

int check_buffers(const char *what, const void *d_pcm, const void *d_adx, const void *d_workspace, size_t workspace_bytes, size_t need)
{
    if (!d_pcm || !d_adx || (!d_workspace && need > 0)) { set_error("%s: null pointer", what); return VGA_ERR_ARGUMENT; }
    if (((uintptr_t)d_pcm & 15) || ((uintptr_t)d_adx & 15) || ((uintptr_t)d_workspace & 15) || workspace_bytes < need) {
        set_error("bad alignment / workspace for %s (PCM, ADX and workspace need 16-byte alignment, the workspace %zu bytes)", what, need);
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}

}  // namespace

extern "C" {

int vga_adx_ragged_layout_for(const vga_adx_params *p, const int *sample_counts, int nch, int64_t *pcm_offsets_out,
                              int64_t *adx_offsets_out, vga_adx_ragged_totals *totals_out)
{
    if (!pcm_offsets_out && !adx_offsets_out && !totals_out) { set_error("vga_adx_ragged_layout_for: no output"); return VGA_ERR_ARGUMENT; }
    adx::RaggedLayout L;
    if (int rc = adx::make_layout(p, sample_counts, nch, L)) return rc;
    if (pcm_offsets_out) std::copy(L.pcm_off.begin(), L.pcm_off.end(), pcm_offsets_out);
    if (adx_offsets_out) std::copy(L.adx_off.begin(), L.adx_off.end(), adx_offsets_out);
    if (totals_out) *totals_out = L.totals;
    return VGA_OK;
}

int vga_adx_ragged_create(const vga_adx_params *p, const int *sample_counts, int nch, vga_adx_ragged **out)
{
    if (!out) { set_error("null output"); return VGA_ERR_ARGUMENT; }
    *out = nullptr;
    vga_adx_ragged *r = new vga_adx_ragged;
    int rc = adx::make_layout(p, sample_counts, nch, r->L);
    if (!rc && nch > 0) rc = require_device();
    if (!rc && nch > 0) {
        (void)hipGetDevice(&r->device);
        r->cus = device_cu_count();
        r->enc_params = adx::make_device_params(p, true);
        r->dec_params = adx::make_device_params(p, false);
        // (the encoder's arithmetic holds for coefficients of the size the reference can produce: adx_quantise_step)
        r->enc_pieces = r->L.time_pieces && std::abs(r->enc_params.coef0) <= 16384 && std::abs(r->enc_params.coef1) <= 16384;
        r->dec_pieces = r->L.time_pieces;
        r->enc = adx::make_plan(r->L, r->cus, encoder_segments_override(), true);
        r->dec = adx::make_plan(r->L, r->cus, encoder_segments_override(), false);
        rc = upload_tables(*r);
    }
    if (rc) {
        delete r;
        return rc;
    }
    *out = r;
    return VGA_OK;
}

void vga_adx_ragged_destroy(vga_adx_ragged *r) { delete r; }

int vga_adx_ragged_channels(const vga_adx_ragged *r) { return r ? r->L.count : 0; }

int vga_adx_ragged_totals_of(const vga_adx_ragged *r, vga_adx_ragged_totals *out)
{
    if (!r || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    *out = r->L.totals;
    return VGA_OK;
}

int vga_adx_ragged_offsets(const vga_adx_ragged *r, int64_t *pcm_offsets_out, int64_t *adx_offsets_out)
{
    if (!r) { set_error("null vga_adx_ragged"); return VGA_ERR_ARGUMENT; }
    if (pcm_offsets_out) std::copy(r->L.pcm_off.begin(), r->L.pcm_off.end(), pcm_offsets_out);
    if (adx_offsets_out) std::copy(r->L.adx_off.begin(), r->L.adx_off.end(), adx_offsets_out);
    return VGA_OK;
}

int vga_adx_encode_device_v(const vga_adx_ragged *r, const int16_t *d_pcm, uint8_t *d_adx, int16_t *d_history_out, void *d_workspace,
                            size_t workspace_bytes, void *stream)
{
    if (int rc = check_object(r, "vga_adx_encode_device_v")) return rc;
    if (r->L.count == 0) return VGA_OK;
    if (r->L.first_empty >= 0 && r->L.p.version == 4 && r->L.p.padding == 0) {
        set_error("channel %d is empty: the reference reads pcm[0] (CriAdxCodec.cs:71)", r->L.first_empty);
        return VGA_ERR_ARGUMENT;
    }
    const size_t need = r->enc_pieces ? r->L.totals.encode_workspace_bytes : 0;
    if (int rc = check_buffers("vga_adx_encode_device_v", d_pcm, d_adx, d_workspace, workspace_bytes, need)) return rc;
    note_adx_encode_path(r->enc_pieces ? 1 : 2);
    return adx::launch_encode_ragged(d_pcm, r->tables, r->enc_items, r->enc_pieces, r->cus, r->enc_params, d_adx, d_history_out,
                                     d_workspace, (hipStream_t)stream);
}

int vga_adx_decode_device_v(const vga_adx_ragged *r, const uint8_t *d_adx, int16_t *d_pcm, void *d_workspace, size_t workspace_bytes,
                            int *d_status, void *stream)
{
    if (int rc = check_object(r, "vga_adx_decode_device_v")) return rc;
    if (r->L.count == 0) return VGA_OK;
    if (!d_status) { set_error("vga_adx_decode_device_v: null pointer"); return VGA_ERR_ARGUMENT; }
    const size_t need = r->dec_pieces ? r->L.totals.decode_workspace_bytes : 0;
    if (int rc = check_buffers("vga_adx_decode_device_v", d_pcm, d_adx, d_workspace, workspace_bytes, need)) return rc;
    note_adx_decode_path(r->dec_pieces ? 1 : 2);
    return adx::launch_decode_ragged(d_adx, r->tables, r->dec_items, r->dec_pieces, r->dec_params, d_pcm, d_status, d_workspace,
                                     (hipStream_t)stream);
}

int vga_testing_adx_ragged_stats(const void *ragged, long long *out, int n)
{
    const vga_adx_ragged *r = static_cast<const vga_adx_ragged *>(ragged);
    if (!r) return 10;
    const long long v[10] = {(long long)r->L.totals.total_frames, r->L.groups(),
                             r->enc.pieces.segments, r->enc.pieces.seg_frames, r->enc.item_count(),
                             r->dec.pieces.segments, r->dec.pieces.seg_frames, r->dec.item_count(),
                             r->L.count > 0 ? (r->enc_pieces ? 1 : 2) : 0, r->L.count > 0 ? (r->dec_pieces ? 1 : 2) : 0};
    for (int i = 0; out && i < n && i < 10; i++) out[i] = v[i];
    return 10;
}

}  // extern "C"
