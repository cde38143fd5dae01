// capi_nw_files.hip -- sets of BRSTM / BCSTM / BFSTM files on the device: the images of every file written and read in one set
// of launches (include/vgaudio_hip/nw_files.h).  Host side only: checks, layout and work tables come from nw_files_host.hpp;
// create uploads the tables the kernels read (nw_files_kernels.hpp), a call checks its pointers and launches.
#include "common.hpp"
#include "nw_files_kernels.hpp"

#include <cstring>
#include <vector>

using namespace vga;

const char *vga::last_error() { return vga_last_error(); }

struct vga_nw_files {
    nwf::FilesLayout L;
    vga_gcadpcm_ragged *ragged = nullptr;
    void *d_tables = nullptr;
    nwf::DeviceTables tables;
    int device = 0;
    ~vga_nw_files()
    {
        if (ragged) vga_gcadpcm_ragged_destroy(ragged);
        if (d_tables) (void)hipFree(d_tables);
    }
};

namespace {

template <class T> size_t place(size_t &at, const std::vector<T> &v)
{
    const size_t here = at;
    at += (size_t)round_up((int64_t)(v.size() * sizeof(T)), 16);
    return here;
}
template <class T> void fill(std::vector<unsigned char> &host, size_t at, const std::vector<T> &v)
{
    if (!v.empty()) memcpy(host.data() + at, v.data(), v.size() * sizeof(T));
}

// the ragged batch of the rows and the tables in the current device's memory
int finish_create(vga_nw_files *s)
{
    nwf::FilesLayout &L = s->L;
    if (L.totals.files == 0) {                                  // an empty set needs no device; with one it has its (empty) batch
        if (vga_gcadpcm_ragged_create(nullptr, 0, &s->ragged) != VGA_OK) s->ragged = nullptr;
        return VGA_OK;
    }
    if (int rc = require_device()) return rc;
    (void)hipGetDevice(&s->device);
    if (int rc = vga_gcadpcm_ragged_create(L.counts.data(), (int)L.counts.size(), &s->ragged)) return rc;
    if (vga_gcadpcm_ragged_pcm_samples(s->ragged) != L.totals.pcm_samples || vga_gcadpcm_ragged_adpcm_bytes(s->ragged) != L.totals.adpcm_bytes) {
        set_error("internal: the set's rows are not the ragged batch's");
        return VGA_ERR_DEVICE;
    }
    size_t bytes = 0;
    const size_t tab_at = place(bytes, L.tab), rows_at = place(bytes, L.channel), meta_at = place(bytes, L.meta);
    const size_t audio_at = place(bytes, L.audio_items), seek_at = place(bytes, L.seek_items);
    std::vector<unsigned char> host(bytes + 16, 0);
    fill(host, tab_at, L.tab);
    fill(host, rows_at, L.channel);
    fill(host, meta_at, L.meta);
    fill(host, audio_at, L.audio_items);
    fill(host, seek_at, L.seek_items);
    VGA_HIP_TRY(device_malloc(&s->d_tables, host.size()));
    VGA_HIP_TRY(hipMemcpy(s->d_tables, host.data(), host.size(), hipMemcpyHostToDevice));
    const unsigned char *d = static_cast<const unsigned char *>(s->d_tables);
    s->tables.tab = reinterpret_cast<const nwf::FileTab *>(d + tab_at);
    s->tables.rows = reinterpret_cast<const nwf::ChannelRow *>(d + rows_at);
    s->tables.meta = reinterpret_cast<const nwf::ChannelMeta *>(d + meta_at);
    s->tables.audio = reinterpret_cast<const nwf::Item *>(d + audio_at);
    s->tables.seek = reinterpret_cast<const nwf::Item *>(d + seek_at);
    s->tables.files = L.totals.files;
    s->tables.channels = (int)L.channel.size();
    s->tables.audio_items = (int)L.audio_items.size();
    s->tables.seek_items = (int)L.seek_items.size();
    return VGA_OK;
}

int check_object(const vga_nw_files *s, const char *what)
{
    if (!s) { set_error("%s: null vga_nw_files", what); return VGA_ERR_ARGUMENT; }
    int device = -1;
    if (s->L.totals.files > 0) (void)hipGetDevice(&device);
    if (s->L.totals.files > 0 && device != s->device) {
        set_error("%s: the set was created on device %d, the current one is %d", what, s->device, device);
        return VGA_ERR_ARGUMENT;
    }
    return VGA_OK;
}

void copy_offsets(const nwf::FilesLayout &L, int *first_channel_out, int64_t *seek_offsets_out, int64_t *image_offsets_out)
{
    if (first_channel_out) std::copy(L.first_channel.begin(), L.first_channel.end(), first_channel_out);
    if (seek_offsets_out)
        for (size_t c = 0; c < L.channel.size(); c++) seek_offsets_out[c] = L.channel[c].seek_off;
    if (image_offsets_out) std::copy(L.image_off.begin(), L.image_off.end(), image_offsets_out);
}

template <class Make> int create_with(vga_nw_files **out, Make &&make)
{
    if (!out) { set_error("null output"); return VGA_ERR_ARGUMENT; }
    *out = nullptr;
    vga_nw_files *s = new vga_nw_files;
    int rc = make(s->L);
    if (!rc) rc = finish_create(s);
    if (rc) {
        delete s;
        return rc;
    }
    *out = s;
    return VGA_OK;
}

}  // namespace

extern "C" {

int vga_nw_files_layout_for(const vga_nw_file *files, int nfiles, const vga_nw_file_config *config, int *first_channel_out,
                            int64_t *seek_offsets_out, int64_t *image_offsets_out, vga_nw_files_totals *totals_out)
{
    if (!first_channel_out && !seek_offsets_out && !image_offsets_out && !totals_out) { set_error("vga_nw_files_layout_for: no output"); return VGA_ERR_ARGUMENT; }
    nwf::FilesLayout L;
    if (int rc = nwf::make_layout(files, nfiles, config, L)) return rc;
    copy_offsets(L, first_channel_out, seek_offsets_out, image_offsets_out);
    if (totals_out) *totals_out = L.totals;
    return VGA_OK;
}

int vga_nw_files_create(const vga_nw_file *files, int nfiles, const vga_nw_file_config *config, vga_nw_files **out)
{
    return create_with(out, [&](nwf::FilesLayout &L) { return nwf::make_layout(files, nfiles, config, L); });
}

int vga_nw_files_create_from_infos(const vga_nwstm_info *const *infos, int nfiles, const int64_t *image_offsets, vga_nw_files **out)
{
    return create_with(out, [&](nwf::FilesLayout &L) { return nwf::make_layout_from_infos(infos, nfiles, image_offsets, L); });
}

void vga_nw_files_destroy(vga_nw_files *s) { delete s; }

int vga_nw_files_totals_of(const vga_nw_files *s, vga_nw_files_totals *out)
{
    if (!s || !out) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    *out = s->L.totals;
    return VGA_OK;
}

int vga_nw_files_offsets(const vga_nw_files *s, int *first_channel_out, int64_t *seek_offsets_out, int64_t *image_offsets_out)
{
    if (!s) { set_error("null vga_nw_files"); return VGA_ERR_ARGUMENT; }
    copy_offsets(s->L, first_channel_out, seek_offsets_out, image_offsets_out);
    return VGA_OK;
}

int vga_nw_files_gc_files(const vga_nw_files *s, vga_gc_file *out)
{
    if (!s || (s->L.totals.files > 0 && !out)) { set_error("null argument"); return VGA_ERR_ARGUMENT; }
    if (s->L.from_infos) { set_error("vga_nw_files_gc_files: the set was made from parsed headers and has no writer configuration"); return VGA_ERR_INVALID_OP; }
    for (int f = 0; f < s->L.totals.files; f++) out[f] = {s->L.tab[f].h.nch, s->L.sample_rate[f], s->L.layout[f].channel};
    return VGA_OK;
}

const vga_gcadpcm_ragged *vga_nw_files_ragged(const vga_nw_files *s) { return s ? s->ragged : nullptr; }

int vga_nwstm_write_device_v(const vga_nw_files *s, const uint8_t *d_adpcm, const int16_t *d_coefs, const int16_t *d_gain,
                             const int16_t *d_start_context, const int16_t *d_loop_context, const int16_t *d_seek, uint8_t *d_images,
                             void *stream)
{
    if (int rc = check_object(s, "vga_nwstm_write_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = nwf::check_write(s->L, d_adpcm, d_coefs, d_seek, d_images)) return rc;
    return nwf::launch_write_images(s->tables, d_adpcm, d_coefs, d_gain, d_start_context, d_loop_context, d_seek, d_images, (hipStream_t)stream);
}

int vga_nwstm_read_device_v(const vga_nw_files *s, const uint8_t *d_images, uint8_t *d_adpcm, int16_t *d_coefs, int16_t *d_gain,
                            int16_t *d_start_context, int16_t *d_loop_context, void *stream)
{
    if (int rc = check_object(s, "vga_nwstm_read_device_v")) return rc;
    if (s->L.totals.files == 0) return VGA_OK;
    if (int rc = nwf::check_read(s->L, d_images, d_adpcm)) return rc;
    return nwf::launch_read_images(s->tables, d_images, d_adpcm, d_coefs, d_gain, d_start_context, d_loop_context, (hipStream_t)stream);
}

}  // extern "C"
